// Host build of ginger-lib_amd/csrc/schnorr_recode.h (g++) for tests/test_schnorr_host.py: the digits the variable-base kernel
// reads, for one scalar and one window.  Test infrastructure.
#include <stdint.h>
#include "../../ginger-lib_amd/csrc/schnorr_recode.h"

using namespace gh;

template <int W> static int recode(const uint32_t* k, int32_t* digits) {
    constexpr int M = VbWindow<W>::M;
    for (int j = 0; j < M; j++) {
        uint32_t idx;
        bool neg;
        vb_digit<W>(k, j, idx, neg);
        const int32_t d = 2 * (int32_t)idx + 1;
        digits[j] = neg ? -d : d;
    }
    return M;
}

// k: 24 LE words below 2^753; digits: room for 189 entries.  Returns the digit count, or -1 for an unsupported window.
extern "C" int t_vb_recode(int w, const uint32_t* k, int32_t* digits) {
    switch (w) {
        case 4: return recode<4>(k, digits);
        case 5: return recode<5>(k, digits);
        case 6: return recode<6>(k, digits);
    }
    return -1;
}
