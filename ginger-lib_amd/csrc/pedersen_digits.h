// pedersen_digits.h -- how the Pedersen kernels (pedersen.hip) cut an input into table digits, free of HIP so that
// tests/host_shim/pedersen_shim.cpp checks the kernels' own digits on the host.
//
// The G generators are flat (window-major); bit b of the input, the least significant bit of each byte first, selects g_b.
// With t table bits (t divides 8: a digit never straddles a byte) position p covers the group of generators
// [p t, min((p + 1) t, G)), and the digit of a row at p is those bits of the row: bit j of the digit selects g_(p t + j).
// Bits at or beyond 8 nbytes read as 0, and so do the bits of a partial last group at or beyond G.  The table holds, per
// position, the 2^t - 1 sums of the non-empty subsets of the group: digit d != 0 reads entry ped_entry(t, p, d).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GH_PED_HD __host__ __device__ __forceinline__
#else
#define GH_PED_HD inline
#endif

namespace gh {

GH_PED_HD bool ped_table_bits_ok(int t) { return t == 1 || t == 2 || t == 4 || t == 8; }
// positions of G generators: the last one is partial if t does not divide G
GH_PED_HD size_t ped_positions(size_t G, int t) { return (G + (size_t)t - 1) / (size_t)t; }
// generators in the group of position p < ped_positions(G, t)
GH_PED_HD int ped_width(size_t G, int t, size_t p) {
    const size_t left = G - p * (size_t)t;
    return left < (size_t)t ? (int)left : t;
}
// the positions a row of nbytes bytes can have a non-zero digit at (8 nbytes <= G)
GH_PED_HD size_t ped_row_positions(size_t nbytes, int t) { return (8 * nbytes + (size_t)t - 1) / (size_t)t; }
GH_PED_HD uint32_t ped_digit(const uint8_t* row, size_t nbytes, size_t G, int t, size_t p) {
    const size_t bit = p * (size_t)t, byte = bit >> 3;
    if (byte >= nbytes || bit >= G) return 0u;
    const uint32_t d = ((uint32_t)row[byte] >> (bit & 7)) & ((1u << t) - 1u);
    return d & ((1u << ped_width(G, t, p)) - 1u);
}
GH_PED_HD size_t ped_entries_per_position(int t) { return ((size_t)1 << t) - 1; }
GH_PED_HD size_t ped_entry(int t, size_t p, uint32_t d) { return p * ped_entries_per_position(t) + d - 1; }

}  // namespace gh
