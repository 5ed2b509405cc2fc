// Host build of ginger-lib_amd/csrc/pairing29_mnt6.h (g++) for tests/test_pairing6_host.py: the GH_HD pairing code the MNT6-753
// kernels run, one row at a time.  Elements cross in the C ABI's form (12 u64 Montgomery limbs; Fq6 in the order
// c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2).  Test infrastructure.
#include <stdint.h>
#include <vector>
#include "../../ginger-lib_amd/csrc/pairing29_mnt6.h"

using namespace gh;
typedef Mnt6Pairing E;

static const int8_t ATE_NAF[] = GH_MNT6_ATE_NAF;
static const int8_t W0_NAF[] = GH_MNT6_W0_NAF;

static Fp ld(const uint64_t* w) { return fp_from_abi<P6>((const uint32_t*)w); }
static Fp3T ld3(const uint64_t* w) { return Fp3T{ld(w), ld(w + 12), ld(w + 24)}; }
static Fq6T ld6(const uint64_t* w) { return Fq6T{ld3(w), ld3(w + 36)}; }
static void st6(uint64_t* w, const Fq6T& a) {
    E::B::to_abi((uint32_t*)w, a.c0);
    E::B::to_abi((uint32_t*)(w + 36), a.c1);
}

// out = final_exp(prod_j miller(P_j, Q_j)), 1 <= k <= 3, the running points Jacobian (the variable-Q steps)
extern "C" int t_pairing6_product(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, int k, uint64_t* out) {
    if (k < 1 || k > 3) return -1;
    E::G1Pre P[3];
    Fp3T qx[3], qy[3];
    bool skip[3];
    for (int j = 0; j < k; j++) {
        P[j] = E::g1_pre(ld(g1_xy + 24 * j), ld(g1_xy + 24 * j + 12));
        qx[j] = ld3(g2_xy + 72 * j);
        qy[j] = ld3(g2_xy + 72 * j + 36);
        skip[j] = g1_inf[j] || g2_inf[j];
    }
    st6(out, E::final_exponentiation(miller_variable<E>(P, qx, qy, skip, k, ATE_NAF), W0_NAF));
    return 0;
}

// the same for one pair through a prepared table (the prepared-Q steps)
extern "C" int t_pairing6_prepared(const uint64_t* g1_xy, const uint64_t* g2_xy, uint64_t* out) {
    std::vector<E::Coeff> tab(E::TABLE_STEPS);
    E::prepare_g2(ld3(g2_xy), ld3(g2_xy + 36), ATE_NAF, tab.data());
    const E::G1Pre P = E::g1_pre(ld(g1_xy), ld(g1_xy + 12));
    Fq6T f = E::one();
    int idx = 0;
    for (int i = 0; i < E::ATE_DIGITS; i++) {
        f = E::sqr(f);
        f = E::mul_by_line(f, E::line_c0(P), E::prepared_line(tab[idx++], P));
        if (ATE_NAF[i] != 0) f = E::mul_by_line(f, E::line_c0(P), E::prepared_line(tab[idx++], P));
    }
    st6(out, E::final_exponentiation(E::miller_end(f), W0_NAF));
    return idx == E::TABLE_STEPS ? 0 : -1;
}

// 0 mul, 1 sqr, 2 inverse, 3 .. 7 Frobenius power 1 .. 5, 8 cyclotomic square, 9 cyclotomic_exp by T,
// 10 mul_by_2345 (b read as c0.c2 and c1), 11 unitary inverse, 12 final exponentiation
extern "C" int t_fq6_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const Fq6T x = ld6(a), y = ld6(b);
    switch (op) {
        case 0: st6(out, E::mul(x, y)); return 0;
        case 1: st6(out, E::sqr(x)); return 0;
        case 2: st6(out, E::inverse(x)); return 0;
        case 3: case 4: case 5: case 6: case 7: st6(out, E::frobenius(x, op - 2)); return 0;
        case 8: st6(out, E::cyclotomic_square(x)); return 0;
        case 9: st6(out, E::cyclotomic_exp(x, W0_NAF, E::W0_DIGITS)); return 0;
        case 10: st6(out, E::mul_by_2345(x, y.c0.c2, y.c1)); return 0;
        case 11: st6(out, E::unitary_inverse(x)); return 0;
        case 12: st6(out, E::final_exponentiation(x, W0_NAF)); return 0;
    }
    return -1;
}
