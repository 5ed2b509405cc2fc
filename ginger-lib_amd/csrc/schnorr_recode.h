// schnorr_recode.h -- the regular signed-window recoding of the variable-base scalar multiplication (schnorr.hip), as GH_HD
// code so that tests/host_shim/schnorr_shim.cpp checks the kernels' own digits on the host.
//
// A scalar k < 2^753 is multiplied as k' = k | 1 (odd), then P is subtracted once if k was even.  k' has M = ceil(753 / W)
// digits d_j, every one odd and non-zero, |d_j| < 2^W, with k' = sum d_j 2^(W j) (Joye-Tunstall).  Every row therefore runs
// the same W (M - 1) doublings and M - 1 additions.  Unrolling the recurrence k_(j+1) = 2 floor(k_j / 2^(W+1)) + 1 gives each
// digit straight from the bits of k, without a carry chain and without reading bit 0:
//   j < M - 1:   b = bits [W j + 1, W j + W] of k,   d_j = 2 b + 1 - 2^W
//   j = M - 1:   b = k >> (W (M - 1) + 1),           d_j = 2 b + 1  (< 2^W because k < 2^(W M))
// The table holds (2 i + 1) P for i < 2^(W-1); d_j selects index i = (|d_j| - 1) / 2 and a sign.
#pragma once
#include <stdint.h>
#include "fp29.h"

namespace gh {

constexpr int VB_BITS = 753;                                 // scalars below 2^753 (both scalar fields' MODULUS_BITS)

template <int W> struct VbWindow {
    static constexpr int M = (VB_BITS + W - 1) / W;          // digits
    static constexpr int E = 1 << (W - 1);                   // table entries (2 i + 1) P
    static constexpr int DOUBLINGS = W * (M - 1);
};

// nb <= 8 bits of the 24-word little-endian integer k starting at bit `bit` (bits at or above 768 read as 0)
GH_HD uint32_t vb_bits(const uint32_t* k, int bit, int nb) {
    const int wi = bit >> 5, sh = bit & 31;
    uint64_t two = wi < 24 ? k[wi] : 0u;
    if (wi + 1 < 24) two |= (uint64_t)k[wi + 1] << 32;
    return (uint32_t)(two >> sh) & ((1u << nb) - 1u);
}

// digit j of k | 1: table index and sign (neg = the digit is negative)
template <int W> GH_HD void vb_digit(const uint32_t* k, int j, uint32_t& idx, bool& neg) {
    constexpr int M = VbWindow<W>::M;
    constexpr uint32_t HALF = 1u << (W - 1), MASK = HALF - 1u;
    if (j == M - 1) {
        idx = vb_bits(k, W * (M - 1) + 1, W - 1);
        neg = false;
        return;
    }
    const uint32_t b = vb_bits(k, W * j + 1, W);
    neg = b < HALF;
    idx = neg ? (~b & MASK) : (b & MASK);
}

}  // namespace gh
