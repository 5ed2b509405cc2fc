// Host build of ginger-lib_amd/csrc/pairing29.h and pairing29_mnt6.h (g++) for tests/test_pairing_host.py: the GH_HD pairing
// code the kernels of pairing.hip run, one row at a time, for both engines (0 is MNT4-753, 2 is MNT6-753, as GH_PAIRING_*).
// Elements cross in the C ABI's form (12 u64 Montgomery limbs; a tower coordinate as c0 || c1 (|| c2), Fq4 / Fq6 as c0 || c1 of
// those).  Test infrastructure.
#include <stdint.h>
#include <type_traits>
#include <vector>
#include "../../ginger-lib_amd/csrc/pairing29_mnt6.h"

using namespace gh;

template <class E> struct Naf;
template <> struct Naf<Mnt4Pairing> {
    static const int8_t* ate() { static const int8_t v[] = GH_MNT4_ATE_NAF; return v; }
    static const int8_t* w0() { static const int8_t v[] = GH_MNT4_W0_NAF; return v; }
};
template <> struct Naf<Mnt6Pairing> {
    static const int8_t* ate() { static const int8_t v[] = GH_MNT6_ATE_NAF; return v; }
    static const int8_t* w0() { static const int8_t v[] = GH_MNT6_W0_NAF; return v; }
};

template <class E> static constexpr int half() { return 12 * E::BDEG; }       // u64 words of a tower coordinate
template <class E> static Fp ld(const uint64_t* w) { return fp_from_abi<typename E::PF>((const uint32_t*)w); }
template <class E> static typename E::BT ldb(const uint64_t* w) { return E::B::from_abi((const uint32_t*)w); }
template <class E> static typename E::GT ldt(const uint64_t* w) { return typename E::GT{ldb<E>(w), ldb<E>(w + half<E>())}; }
template <class E> static void stt(uint64_t* w, const typename E::GT& a) {
    E::B::to_abi((uint32_t*)w, a.c0);
    E::B::to_abi((uint32_t*)(w + half<E>()), a.c1);
}

template <class E>
static int product(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, int k, uint64_t* out) {
    if (k < 1 || k > 3) return -1;
    typename E::G1Pre P[3];
    typename E::BT qx[3], qy[3];
    bool skip[3];
    for (int j = 0; j < k; j++) {
        P[j] = E::g1_pre(ld<E>(g1_xy + 24 * j), ld<E>(g1_xy + 24 * j + 12));
        qx[j] = ldb<E>(g2_xy + 2 * half<E>() * j);
        qy[j] = ldb<E>(g2_xy + 2 * half<E>() * j + half<E>());
        skip[j] = g1_inf[j] || g2_inf[j];
    }
    stt<E>(out, E::final_exponentiation(miller_variable<E>(P, qx, qy, skip, k, Naf<E>::ate()), Naf<E>::w0()));
    return 0;
}

template <class E> static int prepared(const uint64_t* g1_xy, const uint64_t* g2_xy, uint64_t* out) {
    const int8_t* naf = Naf<E>::ate();
    std::vector<typename E::Coeff> tab(E::TABLE_STEPS);
    E::prepare_g2(ldb<E>(g2_xy), ldb<E>(g2_xy + half<E>()), naf, tab.data());
    const typename E::G1Pre P = E::g1_pre(ld<E>(g1_xy), ld<E>(g1_xy + 12));
    typename E::GT f = E::one();
    int idx = 0;
    for (int i = 0; i < E::ATE_DIGITS; i++) {
        f = E::sqr(f);
        f = E::mul_by_line(f, E::line_c0(P), E::prepared_line(tab[idx++], P));
        if (naf[i] != 0) f = E::mul_by_line(f, E::line_c0(P), E::prepared_line(tab[idx++], P));
    }
    stt<E>(out, E::final_exponentiation(E::miller_end(f), Naf<E>::w0()));
    return idx == E::TABLE_STEPS ? 0 : -1;
}

template <class E> static int gt_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const typename E::GT x = ldt<E>(a), y = ldt<E>(b);
    if (op > 8 && op < 8 + 2 * E::BDEG) {
        stt<E>(out, E::frobenius(x, op - 8));
        return 0;
    }
    switch (op) {
        case 0: stt<E>(out, E::mul(x, y)); return 0;
        case 1: stt<E>(out, E::sqr(x)); return 0;
        case 2: stt<E>(out, E::inverse(x)); return 0;
        case 3: stt<E>(out, E::cyclotomic_square(x)); return 0;
        case 4: stt<E>(out, E::cyclotomic_exp(x, Naf<E>::w0(), E::W0_DIGITS)); return 0;
        case 5:
            if constexpr (std::is_same<E, Mnt4Pairing>::value) stt<E>(out, E::mul_by_023(x, y.c0.c0, y.c1));   // b read as c0.c0, -, c1
            else stt<E>(out, E::mul_by_2345(x, y.c0.c2, y.c1));                                                // b read as c0.c2 and c1
            return 0;
        case 6: stt<E>(out, E::unitary_inverse(x)); return 0;
        case 7: stt<E>(out, E::final_exponentiation(x, Naf<E>::w0())); return 0;
    }
    return -1;
}

// out = final_exp(prod_j miller(P_j, Q_j)), 1 <= k <= 3, the running points Jacobian (the variable-Q steps)
extern "C" int t_pairing_product(int engine, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, int k,
                                 uint64_t* out) {
    if (engine == 0) return product<Mnt4Pairing>(g1_xy, g1_inf, g2_xy, g2_inf, k, out);
    if (engine == 2) return product<Mnt6Pairing>(g1_xy, g1_inf, g2_xy, g2_inf, k, out);
    return -1;
}
// the same for one pair through a prepared table (the prepared-Q steps)
extern "C" int t_pairing_prepared(int engine, const uint64_t* g1_xy, const uint64_t* g2_xy, uint64_t* out) {
    if (engine == 0) return prepared<Mnt4Pairing>(g1_xy, g2_xy, out);
    if (engine == 2) return prepared<Mnt6Pairing>(g1_xy, g2_xy, out);
    return -1;
}
// 0 mul, 1 sqr, 2 inverse, 3 cyclotomic square, 4 cyclotomic_exp by W0, 5 the engine's sparse product (mul_by_023 / mul_by_2345),
// 6 unitary inverse, 7 final exponentiation, 8 + j Frobenius power j for j in 1 .. k - 1
extern "C" int t_gt_op(int engine, int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    if (engine == 0) return gt_op<Mnt4Pairing>(op, a, b, out);
    if (engine == 2) return gt_op<Mnt6Pairing>(op, a, b, out);
    return -1;
}
