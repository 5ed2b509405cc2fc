// pairing29_mnt6.h -- the MNT6-753 reduced ate pairing: the engine Mnt6Pairing over the PairingTower of pairing29.h, whose
// header carries the tower, the line formulas and the product counts of both engines.  Plain GH_HD code: the same text runs in
// the kernels of pairing_impl.h and, compiled by g++, in tests/host_shim/pairing6_shim.cpp.  DESIGN.md section 14a.
#pragma once
#include "pairing29.h"

namespace gh {

struct Mnt6Pairing : PairingTower<Mnt6Pairing, F3<P6, 11, false>> {
    typedef P6 PF;
    typedef Mnt6G1 G1;
    typedef Mnt6G2 G2;
    static constexpr int ATE_DIGITS = GH_MNT6_ATE_DIGITS;
    static constexpr int W0_DIGITS = GH_MNT6_W0_DIGITS;
    static constexpr int TABLE_STEPS = GH_MNT6_ATE_DIGITS + GH_MNT6_ATE_NONZERO;    // 499 entries of 3 Fq3

    static GH_HD Fp mul11(const Fp& a) { return fp_mul_small<P6, 11>(a); }
    // times u, the generator of Fq3: the non-residue of Fq6 over Fq3 and the twist      (fp6_2over3.rs:69-77)
    static GH_HD Fp3T mul_nr(const Fp3T& a) { return Fp3T{mul11(a.c2), a.c0, a.c1}; }
    static GH_HD Fp3T mul_u2(const Fp3T& a) { return Fp3T{mul11(a.c1), mul11(a.c2), a.c0}; }
    static GH_HD Fp3T mul_fp(const Fp3T& a, const Fp& s) { return Fp3T{B::mulx(a.c0, s), B::mulx(a.c1, s), B::mulx(a.c2, s)}; }
    // 1 / a by the norm to Fq and one inversion there; zero gives zero                  (fp3.rs inverse)
    static GH_HD Fp3T inv(const Fp3T& a) {
        const Fp s0 = fp_sub<P6>(B::sqrx(a.c0), mul11(B::mulx(a.c1, a.c2)));
        const Fp s1 = fp_sub<P6>(mul11(B::sqrx(a.c2)), B::mulx(a.c0, a.c1));
        const Fp s2 = fp_sub<P6>(B::sqrx(a.c1), B::mulx(a.c0, a.c2));
        const Fp n = fp_add<P6>(B::mulx(a.c0, s0), mul11(fp_add<P6>(B::mulx(a.c2, s1), B::mulx(a.c1, s2))));
        const Fp ni = fp_inv<P6>(n);
        return Fp3T{B::mulx(s0, ni), B::mulx(s1, ni), B::mulx(s2, ni)};
    }
    // times a' = 11 u^2, in one-pass small products (Mnt6G2::mul_by_a takes the add chain for 121)
    static GH_HD Fp3T mul_a(const Fp3T& a) { return Fp3T{mul11(mul11(a.c1)), mul11(mul11(a.c2)), mul11(a.c0)}; }
    // x_Q - twist x_P: the twist is u, so x_P leaves coefficient 1
    static GH_HD Fp3T sub_twist_px(const Fp3T& qx, const Fp& px) { return Fp3T{qx.c0, fp_sub<P6>(qx.c1, px), qx.c2}; }
    static GH_HD G1Pre g1_pre(const Fp& x, const Fp& y) { return G1Pre{x, y}; }
    // the c0 of a variable step's line from v y_P: times u^2
    static GH_HD Fp3T line_embed(const Fp3T& v) { return mul_u2(v); }

    // times (c0: [0, 0, b0], c1: b1): 3 + 6 + 6 = 15 products                           (fp6_2over3.rs:110-122)
    static GH_HD Fq6T mul_by_2345(const Fq6T& a, const Fp& b0, const Fp3T& b1) {
        const Fp3T v0 = mul_u2(mul_fp(a.c0, b0)), v1 = B::mul(a.c1, b1);
        const Fp3T s = B::mul(B::add(a.c0, a.c1), Fp3T{b1.c0, b1.c1, fp_add<P6>(b1.c2, b0)});
        return Fq6T{B::add(v0, mul_nr(v1)), B::sub(B::sub(s, v0), v1)};
    }
    // times a prepared step's line (c0: [0, 0, b0], c1: b1)
    static GH_HD Fq6T mul_by_line(const Fq6T& a, const Fp& b0, const Fp3T& b1) { return mul_by_2345(a, b0, b1); }
    // the trace is positive: nothing follows the Miller loop                            (mod.rs:217-219)
    static GH_HD Fq6T miller_end(const Fq6T& f) { return f; }
    // 11^((p^k - 1)/3), its square and 11^((p^k - 1)/6)
    static GH_HD Fp frob3_c1(int k) {
        switch (k % 3) {
            case 1: { const uint32_t c[NL] = GH_MNT6_FROB3_C1_1_I29; return fp_const<P6>(c); }
            case 2: { const uint32_t c[NL] = GH_MNT6_FROB3_C1_2_I29; return fp_const<P6>(c); }
        }
        return fp_one<P6>();
    }
    static GH_HD Fp frob3_c2(int k) {
        switch (k % 3) {
            case 1: { const uint32_t c[NL] = GH_MNT6_FROB3_C2_1_I29; return fp_const<P6>(c); }
            case 2: { const uint32_t c[NL] = GH_MNT6_FROB3_C2_2_I29; return fp_const<P6>(c); }
        }
        return fp_one<P6>();
    }
    static GH_HD Fp frob6_coeff(int k) {
        switch (k % 6) {
            case 1: { const uint32_t c[NL] = GH_MNT6_FROB6_C1_1_I29; return fp_const<P6>(c); }
            case 2: { const uint32_t c[NL] = GH_MNT6_FROB6_C1_2_I29; return fp_const<P6>(c); }
            case 3: { const uint32_t c[NL] = GH_MNT6_FROB6_C1_3_I29; return fp_const<P6>(c); }
            case 4: { const uint32_t c[NL] = GH_MNT6_FROB6_C1_4_I29; return fp_const<P6>(c); }
            case 5: { const uint32_t c[NL] = GH_MNT6_FROB6_C1_5_I29; return fp_const<P6>(c); }
        }
        return fp_one<P6>();
    }
    static GH_HD Fp3T frob3(const Fp3T& a, int k) {                                               // fp3.rs frobenius_map
        if (k % 3 == 0) return a;
        return Fp3T{a.c0, B::mulx(a.c1, frob3_c1(k)), B::mulx(a.c2, frob3_c2(k))};
    }
    // a^(p^k), k >= 0                                                                   (fp6_2over3.rs:227-232)
    static GH_HD Fq6T frobenius(const Fq6T& a, int k) {
        Fq6T r{frob3(a.c0, k), frob3(a.c1, k)};
        if (k % 6) r.c1 = mul_fp(r.c1, frob6_coeff(k));
        return r;
    }
    // f^((p^6 - 1)/r) by the reference's split (mod.rs:224-272): (p^3 - 1)(p + 1), then p + w0 with w0 = +T on the element
    // itself.  w0naf: the W0_DIGITS signed digits of T.  f = 0 gives 0.
    static GH_HD Fq6T final_exponentiation(const Fq6T& f, const int8_t* w0naf);
};

GH_HD Fq6T Mnt6Pairing::final_exponentiation(const Fq6T& f, const int8_t* w0naf) {
    const Fq6T fi = inverse(f);
    const Fq6T g = gt_mul_call<Mnt6Pairing>(frobenius(f, 3), fi);            // f^(p^3 - 1)
    const Fq6T elt = gt_mul_call<Mnt6Pairing>(frobenius(g, 1), g);           // ... ^(p + 1)
    const Fq6T w1 = frobenius(elt, 1);                                       // m1 = 1
    const Fq6T w0 = cyclotomic_exp(elt, w0naf, W0_DIGITS);
    return gt_mul_call<Mnt6Pairing>(w1, w0);
}

}  // namespace gh
