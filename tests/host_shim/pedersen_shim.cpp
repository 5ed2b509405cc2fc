// Host build of ginger-lib_amd/csrc/pedersen_digits.h (g++) for tests/test_pedersen_host.py: the digits and table entries the
// Pedersen kernels read, for one row.  Test infrastructure.
#include "../../ginger-lib_amd/csrc/pedersen_digits.h"

using namespace gh;

extern "C" {

int t_ped_table_bits_ok(int t) { return ped_table_bits_ok(t); }
uint64_t t_ped_positions(uint64_t G, int t) { return ped_positions(G, t); }
uint64_t t_ped_row_positions(uint64_t nbytes, int t) { return ped_row_positions(nbytes, t); }
int t_ped_width(uint64_t G, int t, uint64_t p) { return ped_width(G, t, p); }
uint64_t t_ped_entry(int t, uint64_t p, uint32_t d) { return ped_entry(t, p, d); }
// digits[p] for every position p < ped_positions(G, t) of one row; returns the count
uint64_t t_ped_digits(const uint8_t* row, uint64_t nbytes, uint64_t G, int t, uint32_t* digits) {
    const uint64_t np = ped_positions(G, t);
    for (uint64_t p = 0; p < np; p++) digits[p] = ped_digit(row, nbytes, G, t, p);
    return np;
}

}  // extern "C"
