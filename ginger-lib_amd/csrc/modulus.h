// modulus.h -- the comparison of an ABI row (12 u64 words, least significant first) with a field's modulus.  Free of HIP: the
// units' host layer (unit_host.h) and the host-tested plans (r1cs_plan.h) both read it.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "fp29.h"

namespace gh {

template <class P> inline const uint64_t* modulus64() {
    static const uint64_t p4[12] = GH_P4_P_64, p6[12] = GH_P6_P_64;
    return std::is_same<P, P6>::value ? p6 : p4;
}
template <class P> inline bool below(const uint64_t* x) {
    const uint64_t* p = modulus64<P>();
    for (int i = 11; i >= 0; i--)
        if (x[i] != p[i]) return x[i] < p[i];
    return false;
}

}  // namespace gh
