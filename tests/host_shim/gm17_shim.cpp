// Host build of ginger-lib_amd/csrc/gm17_sum.h (g++) for tests/test_gm17_verify_host.py: the GH_HD group additions that
// gm17_sums_kernel runs, for both engines, and one row of the GM17 verdict composed from them with the Miller loop and the final
// exponentiation of pairing29.h / pairing29_mnt6.h.  Elements cross in the C ABI's form (12 u64 Montgomery limbs, a tower
// coordinate as c0 || c1 (|| c2)); engine 0 is MNT4-753, 2 is MNT6-753.  Test infrastructure.
#include <stdint.h>
#include "../../ginger-lib_amd/csrc/gm17_sum.h"

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

template <class E> static Gm17Point<Fp> ld1(const uint64_t* w, int inf) {
    return Gm17Point<Fp>{fp_from_abi<typename E::PF>((const uint32_t*)w), fp_from_abi<typename E::PF>((const uint32_t*)(w + 12)), inf != 0};
}
template <class E> static Gm17Point<typename E::B::T> ld2(const uint64_t* w, int inf) {
    typedef typename E::B B;
    return Gm17Point<typename B::T>{B::from_abi((const uint32_t*)w), B::from_abi((const uint32_t*)(w + 12 * E::BDEG)), inf != 0};
}

template <class E> static int sum_g1(const uint64_t* p, int p_inf, const uint64_t* q, int q_inf, uint64_t* out, uint8_t* out_inf) {
    const Gm17Point<Fp> s = gm17_add<Gm17G1<E>>(ld1<E>(p, p_inf), ld1<E>(q, q_inf));
    fp_to_abi<typename E::PF>((uint32_t*)out, s.x);
    fp_to_abi<typename E::PF>((uint32_t*)(out + 12), s.y);
    *out_inf = s.inf;
    return 0;
}
template <class E> static int sum_g2(const uint64_t* p, int p_inf, const uint64_t* q, int q_inf, uint64_t* out, uint8_t* out_inf) {
    typedef typename E::B B;
    const Gm17Point<typename B::T> s = gm17_add<Gm17G2<E>>(ld2<E>(p, p_inf), ld2<E>(q, q_inf));
    B::to_abi((uint32_t*)out, s.x);
    B::to_abi((uint32_t*)(out + 12 * E::BDEG), s.y);
    *out_inf = s.inf;
    return 0;
}

template <class E> struct Pairs {
    typename E::G1Pre P[3];
    typename E::B::T qx[3], qy[3];
    bool skip[3];
    int k = 0;
    void push(const Gm17Point<Fp>& p, const Gm17Point<typename E::B::T>& q) {
        P[k] = E::g1_pre(p.x, p.y);
        qx[k] = q.x;
        qy[k] = q.y;
        skip[k] = p.inf || q.inf;
        k++;
    }
    typename E::GT value() const { return E::final_exponentiation(miller_variable<E>(P, qx, qy, skip, k, Naf<E>::ate()), Naf<E>::w0()); }
};

// verifier.rs:24-76 for one row whose points are on their curves; g_psi is the caller's.  -> 1 both tests hold, 0 not;
// *tests: bit 0 test1, bit 1 test2
template <class E>
static int row(const uint64_t* g_alpha, const uint64_t* h_beta, const uint64_t* g_gamma, const uint64_t* h_gamma, const uint64_t* h,
               const uint64_t* a, int a_inf, const uint64_t* b, int b_inf, const uint64_t* c, int c_inf, const uint64_t* psi, int psi_inf, int* tests) {
    typedef typename E::B::T BT;
    const Gm17Point<Fp> A = ld1<E>(a, a_inf), GA = ld1<E>(g_alpha, 0);
    const Gm17Point<BT> Bq = ld2<E>(b, b_inf), HB = ld2<E>(h_beta, 0), HG = ld2<E>(h_gamma, 0);
    Pairs<E> key;                                            // e(-g_alpha, h_beta)
    key.push(gm17_neg<Gm17G1<E>>(GA), HB);
    Pairs<E> t1;
    t1.push(gm17_neg<Gm17G1<E>>(gm17_add<Gm17G1<E>>(A, GA)), gm17_add<Gm17G2<E>>(Bq, HB));
    t1.push(ld1<E>(psi, psi_inf), HG);
    t1.push(ld1<E>(c, c_inf), ld2<E>(h, 0));
    Pairs<E> t2;
    t2.push(A, HG);
    t2.push(ld1<E>(g_gamma, 0), gm17_neg<Gm17G2<E>>(Bq));
    const bool ok1 = E::eq(t1.value(), key.value()), ok2 = E::eq(t2.value(), E::one());
    *tests = (ok1 ? 1 : 0) | (ok2 ? 2 : 0);
    return ok1 && ok2;
}

extern "C" int t_gm17_sum_g1(int engine, const uint64_t* p, int p_inf, const uint64_t* q, int q_inf, uint64_t* out, uint8_t* out_inf) {
    if (engine == 0) return sum_g1<Mnt4Pairing>(p, p_inf, q, q_inf, out, out_inf);
    if (engine == 2) return sum_g1<Mnt6Pairing>(p, p_inf, q, q_inf, out, out_inf);
    return -1;
}
extern "C" int t_gm17_sum_g2(int engine, const uint64_t* p, int p_inf, const uint64_t* q, int q_inf, uint64_t* out, uint8_t* out_inf) {
    if (engine == 0) return sum_g2<Mnt4Pairing>(p, p_inf, q, q_inf, out, out_inf);
    if (engine == 2) return sum_g2<Mnt6Pairing>(p, p_inf, q, q_inf, out, out_inf);
    return -1;
}
extern "C" int t_gm17_row(int engine, const uint64_t* g_alpha, const uint64_t* h_beta, const uint64_t* g_gamma, const uint64_t* h_gamma,
                          const uint64_t* h, const uint64_t* a, int a_inf, const uint64_t* b, int b_inf, const uint64_t* c, int c_inf,
                          const uint64_t* psi, int psi_inf, int* tests) {
    if (engine == 0) return row<Mnt4Pairing>(g_alpha, h_beta, g_gamma, h_gamma, h, a, a_inf, b, b_inf, c, c_inf, psi, psi_inf, tests);
    if (engine == 2) return row<Mnt6Pairing>(g_alpha, h_beta, g_gamma, h_gamma, h, a, a_inf, b, b_inf, c, c_inf, psi, psi_inf, tests);
    return -1;
}
