// Host build of ginger-lib_amd/csrc/poseidon_perm.h (g++) for tests/test_poseidon_host.py: the permutation the kernels run,
// with the K states in registers (RegStore) or in a slab (SlabStore), on ABI-form inputs.  Test infrastructure.
#include <stdint.h>
#include <vector>
#include "../../ginger-lib_amd/csrc/poseidon_perm.h"

using namespace gh;

template <class P, int K, bool SLAB> static void run(int r_f, int r_p, const uint32_t* cst, uint32_t* states) {
    const int nrc = 3 * (2 * r_f + r_p);
    std::vector<Fp> c(nrc + 13);
    for (int i = 0; i < nrc + 13; i++) c[i] = fp_from_abi<P>(cst + 24 * i);
    const pos::Consts cs{c.data(), c.data() + nrc, c.data() + nrc + 9, c.data() + nrc + 10, r_f, r_p};
    if constexpr (SLAB) {
        const size_t lanes = 3;                                    // a slab of 3 lanes, the states in the middle one
        std::vector<uint32_t> slab(lanes * pos::SlabStore<K>::kSlots * NL, 0xdeadbeefu);
        pos::SlabStore<K> st{slab.data() + 1, lanes};
        for (int k = 0; k < K; k++)
            for (int e = 0; e < 3; e++) st.set(k, e, fp_from_abi<P>(states + (3 * k + e) * 24));
        pos::permute<P, K>(st, cs);
        for (int k = 0; k < K; k++)
            for (int e = 0; e < 3; e++) fp_to_abi<P>(states + (3 * k + e) * 24, st.get(k, e));
    } else {
        pos::RegStore<K> st;
        for (int k = 0; k < K; k++)
            for (int e = 0; e < 3; e++) st.set(k, e, fp_from_abi<P>(states + (3 * k + e) * 24));
        pos::permute<P, K>(st, cs);
        for (int k = 0; k < K; k++)
            for (int e = 0; e < 3; e++) fp_to_abi<P>(states + (3 * k + e) * 24, st.get(k, e));
    }
}

template <class P> static int dispatch(int k, int slab, int r_f, int r_p, const uint32_t* cst, uint32_t* states) {
    switch (k * 2 + (slab ? 1 : 0)) {
        case 2: run<P, 1, false>(r_f, r_p, cst, states); return 0;
        case 3: run<P, 1, true>(r_f, r_p, cst, states); return 0;
        case 4: run<P, 2, false>(r_f, r_p, cst, states); return 0;
        case 5: run<P, 2, true>(r_f, r_p, cst, states); return 0;
        case 8: run<P, 4, false>(r_f, r_p, cst, states); return 0;
        case 9: run<P, 4, true>(r_f, r_p, cst, states); return 0;
        case 17: run<P, 8, true>(r_f, r_p, cst, states); return 0;
    }
    return -1;
}

// fid 4 / 6: the prime (MNT6-753 Fr = p4, MNT4-753 Fr = p6).  cst: rc[3 rounds] | mds[9] | c2 | azp[3], 24 words each
// (12 u64 ABI limbs); states: K x 3 elements, permuted in place.
extern "C" int t_poseidon_perm(int fid, int k, int slab, int r_f, int r_p, const uint32_t* cst, uint32_t* states) {
    return fid == 4 ? dispatch<P4>(k, slab, r_f, r_p, cst, states) : dispatch<P6>(k, slab, r_f, r_p, cst, states);
}
