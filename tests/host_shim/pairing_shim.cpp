// Host build of ginger-lib_amd/csrc/pairing29.h (g++) for tests/test_pairing_host.py: the GH_HD pairing code the kernels of
// pairing.hip run, one row at a time.  Elements cross in the C ABI's form (12 u64 Montgomery limbs; Fq4 in the order
// c0.c0, c0.c1, c1.c0, c1.c1).  Test infrastructure.
#include <stdint.h>
#include <vector>
#include "../../ginger-lib_amd/csrc/pairing29.h"

using namespace gh;
typedef Mnt4Pairing E;

static const int8_t ATE_NAF[] = GH_MNT4_ATE_NAF;
static const int8_t W0_NAF[] = GH_MNT4_W0_NAF;

static Fp ld(const uint64_t* w) { return fp_from_abi<P4>((const uint32_t*)w); }
static Fp2T ld2(const uint64_t* w) { return Fp2T{ld(w), ld(w + 12)}; }
static Fq4T ld4(const uint64_t* w) { return Fq4T{ld2(w), ld2(w + 24)}; }
static void st4(uint64_t* w, const Fq4T& a) {
    fp_to_abi<P4>((uint32_t*)w, a.c0.c0);
    fp_to_abi<P4>((uint32_t*)(w + 12), a.c0.c1);
    fp_to_abi<P4>((uint32_t*)(w + 24), a.c1.c0);
    fp_to_abi<P4>((uint32_t*)(w + 36), a.c1.c1);
}
static E::G1Pre pre(const uint64_t* xy) { return E::g1_pre(ld(xy), ld(xy + 12)); }

// out = final_exp(prod_j miller(P_j, Q_j)), 1 <= k <= 3, the running points Jacobian (the variable-Q steps)
extern "C" int t_pairing_product(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, int k, uint64_t* out) {
    if (k < 1 || k > 3) return -1;
    E::G1Pre P[3];
    Fp2T qx[3], qy[3];
    bool skip[3];
    for (int j = 0; j < k; j++) {
        P[j] = pre(g1_xy + 24 * j);
        qx[j] = ld2(g2_xy + 48 * j);
        qy[j] = ld2(g2_xy + 48 * j + 24);
        skip[j] = g1_inf[j] || g2_inf[j];
    }
    st4(out, E::final_exponentiation(miller_variable<E>(P, qx, qy, skip, k, ATE_NAF), W0_NAF));
    return 0;
}

// the same for one pair through a prepared table (the prepared-Q steps)
extern "C" int t_pairing_prepared(const uint64_t* g1_xy, const uint64_t* g2_xy, uint64_t* out) {
    std::vector<E::Coeff> tab(E::TABLE_STEPS);
    E::prepare_g2(ld2(g2_xy), ld2(g2_xy + 24), ATE_NAF, tab.data());
    const E::G1Pre P = pre(g1_xy);
    Fq4T f = E::one();
    int idx = 0;
    for (int i = 0; i < E::ATE_DIGITS; i++) {
        f = E::sqr(f);
        f = E::mul_by_line(f, E::line_c0(P), E::prepared_line(tab[idx++], P));
        if (ATE_NAF[i] != 0) f = E::mul_by_line(f, E::line_c0(P), E::prepared_line(tab[idx++], P));
    }
    st4(out, E::final_exponentiation(E::miller_end(f), W0_NAF));
    return idx == E::TABLE_STEPS ? 0 : -1;
}

// 0 mul, 1 sqr, 2 inverse, 3 / 4 / 5 Frobenius power 1 / 2 / 3, 6 cyclotomic square, 7 cyclotomic_exp by T - 1,
// 8 mul_by_023 (b read as c0.c0, -, c1.c0, c1.c1), 9 unitary inverse, 10 final exponentiation
extern "C" int t_fq4_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const Fq4T x = ld4(a), y = ld4(b);
    switch (op) {
        case 0: st4(out, E::mul(x, y)); return 0;
        case 1: st4(out, E::sqr(x)); return 0;
        case 2: st4(out, E::inverse(x)); return 0;
        case 3: case 4: case 5: st4(out, E::frobenius(x, op - 2)); return 0;
        case 6: st4(out, E::cyclotomic_square(x)); return 0;
        case 7: st4(out, E::cyclotomic_exp(x, W0_NAF, E::W0_DIGITS)); return 0;
        case 8: st4(out, E::mul_by_023(x, y.c0.c0, y.c1)); return 0;
        case 9: st4(out, E::unitary_inverse(x)); return 0;
        case 10: st4(out, E::final_exponentiation(x, W0_NAF)); return 0;
    }
    return -1;
}
