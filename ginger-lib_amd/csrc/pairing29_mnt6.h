// pairing29_mnt6.h -- the MNT6-753 reduced ate pairing: the engine policy Mnt6Pairing with the interface of Mnt4Pairing
// (pairing29.h).  Plain GH_HD code: the same text runs in the kernels of pairing_impl.h and, compiled by g++, in
// tests/host_shim/pairing6_shim.cpp.  DESIGN.md section 14.
//
// Reference: algebra/src/curves/models/mnt6/mod.rs (Miller loop :158-222, final exponentiation :224-272),
// algebra/src/fields/models/fp6_2over3.rs, fp3.rs, parameters algebra/src/curves/mnt6753/mod.rs:27-104.
//
//   Fq6 = Fq3[Y]/(Y^2 - u), Fq3 = Fq[u]/(u^3 - 11); twist = u = (0, 1, 0); a' = 11 u^2 = (0, 0, 11).
//   Lines, in the reference's scaling (mod.rs:173-191): for the running point S = (x', y') of the twist and the slope gamma,
//       l(P) = ( y_P u^2 ,  gamma x' - gamma u x_P - y' )  in Fq3 x Fq3.
//   The loop count T = p - r is positive: nothing follows the Miller loop, and the last chunk of the final exponent is
//   p + T with T applied to the element itself.  Any factor from Fq3 on a line is removed by the exponent's p^3 - 1.
//   prepared Q: the table holds the reference's (r_y, gamma, gamma_x) per step (mod.rs:101-155) with the sign of an addition
//       step folded into r_y; the line's c0 = (0, 0, y_P) is sparse: 3 products for gamma u x_P and the 15-product
//       mul_by_2345.  18 products per step.
//   variable Q: Jacobian (X, Y, Z, T = Z^2) over Fq3 with the formulas of pairing29.h; an Fq3 product is 6 products, a square 5.
//       doubling   11 S + 1 M = 61, the line 6, the full Fq6 product 18: 85.
//                  The line is  (y_P u^2 2 Z3 T ,  2 F X - 2 F T u x_P - 4 Y^2): c0 is a full Fq3 element here.
//       addition   7 M + 4 S = 62, the line 15 (L1 (x_Q - u x_P) - y_Q Z3 ; y_P u^2 Z3), the Fq6 product 18: 95.
//   376 x 85 + 123 x 95 = 43.6 K products per variable pair, 376 x 12 = 4.5 K for the squarings of f.
#pragma once
#include "pairing29.h"

namespace gh {

struct Fq6T { Fp3T c0, c1; };

struct Mnt6Pairing {
    typedef P6 PF;
    typedef F3<P6, 11, false> B;          // the base of the tower: Fq3 with out-of-line Fq products
    typedef Fq6T GT;
    typedef Mnt6G1 G1;
    typedef Mnt6G2 G2;
    static constexpr int ATE_DIGITS = GH_MNT6_ATE_DIGITS;
    static constexpr int W0_DIGITS = GH_MNT6_W0_DIGITS;
    static constexpr int TABLE_STEPS = GH_MNT6_ATE_DIGITS + GH_MNT6_ATE_NONZERO;    // 499 entries of 3 Fq3
    static constexpr int BDEG = 3;

    static GH_HD Fp mul11(const Fp& a) { return fp_mul_small<P6, 11>(a); }
    // times u, the generator of Fq3: the non-residue of Fq6 over Fq3 and the twist      (fp6_2over3.rs:69-77)
    static GH_HD Fp3T mul_u(const Fp3T& a) { return Fp3T{mul11(a.c2), a.c0, a.c1}; }
    static GH_HD Fp3T mul_u2(const Fp3T& a) { return Fp3T{mul11(a.c1), mul11(a.c2), a.c0}; }
    // times a' = 11 u^2, in one-pass small products (Mnt6G2::mul_by_a takes the add chain for 121)
    static GH_HD Fp3T mul_a(const Fp3T& a) { return Fp3T{mul11(mul11(a.c1)), mul11(mul11(a.c2)), mul11(a.c0)}; }
    static GH_HD Fp3T mul_fp(const Fp3T& a, const Fp& s) { return Fp3T{B::mulx(a.c0, s), B::mulx(a.c1, s), B::mulx(a.c2, s)}; }
    // 1 / a by the norm to Fq and one inversion there; zero gives zero                  (fp3.rs inverse)
    static GH_HD Fp3T inv3(const Fp3T& a) {
        const Fp s0 = fp_sub<P6>(B::sqrx(a.c0), mul11(B::mulx(a.c1, a.c2)));
        const Fp s1 = fp_sub<P6>(mul11(B::sqrx(a.c2)), B::mulx(a.c0, a.c1));
        const Fp s2 = fp_sub<P6>(B::sqrx(a.c1), B::mulx(a.c0, a.c2));
        const Fp n = fp_add<P6>(B::mulx(a.c0, s0), mul11(fp_add<P6>(B::mulx(a.c2, s1), B::mulx(a.c1, s2))));
        const Fp ni = fp_inv<P6>(n);
        return Fp3T{B::mulx(s0, ni), B::mulx(s1, ni), B::mulx(s2, ni)};
    }

    // ------------------------------------------------------------------------------------------------ Fq6
    static GH_HD Fq6T one() { return Fq6T{B::one(), B::zero()}; }
    static GH_HD bool eq(const Fq6T& a, const Fq6T& b) { return B::eq(a.c0, b.c0) && B::eq(a.c1, b.c1); }
    // Karatsuba over Fq3: 3 Fq3 products = 18 products                                  (fp6_2over3.rs mul_assign)
    static GH_HD Fq6T mul(const Fq6T& a, const Fq6T& b) {
        const Fp3T v0 = B::mul(a.c0, b.c0), v1 = B::mul(a.c1, b.c1);
        const Fp3T s = B::mul(B::add(a.c0, a.c1), B::add(b.c0, b.c1));
        return Fq6T{B::add(v0, mul_u(v1)), B::sub(B::sub(s, v0), v1)};
    }
    // 2 Fq3 products = 12 products                                                      (fp6_2over3.rs:178-195)
    static GH_HD Fq6T sqr(const Fq6T& a) {
        const Fp3T ab = B::mul(a.c0, a.c1);
        const Fp3T t = B::mul(B::add(mul_u(a.c1), a.c0), B::add(a.c0, a.c1));
        return Fq6T{B::sub(B::sub(t, ab), mul_u(ab)), B::dbl(ab)};
    }
    // times (c0: [0, 0, b0], c1: b1): 3 + 6 + 6 = 15 products                           (fp6_2over3.rs:110-122)
    static GH_HD Fq6T mul_by_2345(const Fq6T& a, const Fp& b0, const Fp3T& b1) {
        const Fp3T v0 = mul_u2(mul_fp(a.c0, b0)), v1 = B::mul(a.c1, b1);
        const Fp3T s = B::mul(B::add(a.c0, a.c1), Fp3T{b1.c0, b1.c1, fp_add<P6>(b1.c2, b0)});
        return Fq6T{B::add(v0, mul_u(v1)), B::sub(B::sub(s, v0), v1)};
    }
    static GH_HD Fq6T mul_by_line(const Fq6T& a, const Fp& b0, const Fp3T& b1) { return mul_by_2345(a, b0, b1); }
    // zero gives zero                                                                   (fp6_2over3.rs:197-216)
    static GH_HD Fq6T inverse(const Fq6T& a) {
        const Fp3T t = inv3(B::sub(B::sqr(a.c0), mul_u(B::sqr(a.c1))));
        return Fq6T{B::mul(a.c0, t), B::neg(B::mul(a.c1, t))};
    }
    static GH_HD Fq6T unitary_inverse(const Fq6T& a) { return Fq6T{a.c0, B::neg(a.c1)}; }         // fp6_2over3.rs:79-81
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
    // for a of norm one over Fq3 (after the easy part), c0^2 - u c1^2 = 1: 2 Fq3 squarings = 10 products
    static GH_HD Fq6T cyclotomic_square(const Fq6T& s) {
        const Fp3T a = B::sqr(s.c1);
        const Fp3T c = B::sub(B::sqr(B::add(s.c1, s.c0)), a);
        const Fp3T d = mul_u(a);
        const Fp3T e = B::sub(c, d);
        return Fq6T{B::add(B::dbl(d), B::one()), B::sub(e, B::one())};
    }

    // ------------------------------------------------------------------------------------------------ Miller steps
    // what a pair brings to every step: x_P, y_P
    struct G1Pre { Fp px, py; };
    static GH_HD G1Pre g1_pre(const Fp& x, const Fp& y) { return G1Pre{x, y}; }
    static GH_HD const Fp& line_c0(const G1Pre& P) { return P.py; }
    // the running point of a variable Q: Jacobian, t = z^2
    struct G2Run { Fp3T x, y, z, t; };
    // one entry of a prepared table: the reference's G2PreparedCoefficients, r_y being -+y_Q in an addition step
    struct Coeff { Fp3T r_y, gamma, gamma_x; };

    // twist x_P v
    static GH_HD Fp3T twist_px(const Fp3T& v, const Fp& px) { return mul_u(mul_fp(v, px)); }

    // R <- 2 R, returns the tangent's value at P (scaled by 2 Z3 T): 85 products with the Fq6 product that follows
    static GH_HD Fq6T dbl_step(G2Run& R, const G1Pre& P) {
        const Fp3T A = B::sqr(R.t), Bq = B::sqr(R.x), C = B::sqr(R.y), D = B::sqr(C);
        const Fp3T E = B::sub(B::sub(B::sqr(B::add(R.x, C)), Bq), D);
        const Fp3T F = B::add(B::add(B::dbl(Bq), Bq), mul_a(A));
        const Fp3T G = B::sqr(F);
        const Fp3T E2 = B::dbl(E);
        const Fp3T x3 = B::sub(G, B::dbl(E2));
        const Fp3T D8 = B::dbl(B::dbl(B::dbl(D)));
        const Fp3T y3 = B::sub(B::mul(F, B::sub(E2, x3)), D8);
        const Fp3T z3 = B::sub(B::sub(B::sqr(B::add(R.y, R.z)), C), R.t);
        const Fp3T t3 = B::sqr(z3);
        const Fp3T cH = B::sub(B::sub(B::sqr(B::add(z3, R.t)), t3), A);        // 2 Z3 T
        const Fp3T cJ = B::sub(B::sub(B::sqr(B::add(F, R.t)), G), A);          // 2 F T
        const Fp3T cL = B::sub(B::sub(B::sqr(B::add(F, R.x)), G), Bq);         // 2 F X
        Fq6T l;
        l.c0 = mul_u2(mul_fp(cH, P.py));
        l.c1 = B::sub(B::sub(cL, twist_px(cJ, P.px)), B::dbl(B::dbl(C)));
        R = G2Run{x3, y3, z3, t3};
        return l;
    }
    // R <- R + Q for Q = (qx, qy) affine (qy negated by the caller for a digit -1), returns the chord's value at P (scaled
    // by Z3): 95 products with the Fq6 product that follows.  R = +-Q gives Z3 = 0 and a zero line: never for a point of order r.
    static GH_HD Fq6T add_step(G2Run& R, const Fp3T& qx, const Fp3T& qy, const G1Pre& P) {
        const Fp3T H = B::sub(B::mul(qx, R.t), R.x);
        const Fp3T S2 = B::mul(B::mul(qy, R.z), R.t);
        const Fp3T I = B::sqr(H);
        const Fp3T E = B::dbl(B::dbl(I));
        const Fp3T J = B::mul(H, E);
        const Fp3T V = B::mul(R.x, E);
        const Fp3T L1 = B::dbl(B::sub(S2, R.y));
        const Fp3T x3 = B::sub(B::sub(B::sqr(L1), J), B::dbl(V));
        const Fp3T y3 = B::sub(B::mul(L1, B::sub(V, x3)), B::dbl(B::mul(R.y, J)));
        const Fp3T z3 = B::sub(B::sub(B::sqr(B::add(R.z, H)), R.t), I);
        const Fp3T t3 = B::sqr(z3);
        Fq6T l;
        l.c0 = mul_u2(mul_fp(z3, P.py));
        l.c1 = B::sub(B::mul(L1, Fp3T{qx.c0, fp_sub<P6>(qx.c1, P.px), qx.c2}), B::mul(qy, z3));
        R = G2Run{x3, y3, z3, t3};
        return l;
    }
    // the line of a table entry at P: c0 = (0, 0, y_P), c1 returned
    static GH_HD Fp3T prepared_line(const Coeff& c, const G1Pre& P) {
        return B::sub(B::sub(c.gamma_x, twist_px(c.gamma, P.px)), c.r_y);
    }
    // the reference's ate_precompute_g2 (mod.rs:101-155) for Q = (qx, qy) not at infinity: TABLE_STEPS entries.  naf: the
    // ATE_DIGITS signed digits of the loop count, most significant first.  A zero denominator inverts to zero.
    static GH_HD void prepare_g2(const Fp3T& qx, const Fp3T& qy, const int8_t* naf, Coeff* out) {
        Fp3T sx = qx, sy = qy;
        const Fp3T a = mul_a(B::one());
        int idx = 0;
        for (int i = 0; i < ATE_DIGITS; i++) {
            const Fp3T xx = B::sqr(sx);
            Fp3T gamma = B::mul(B::add(B::add(B::dbl(xx), xx), a), inv3(B::dbl(sy)));
            Fp3T nx = B::sub(B::sqr(gamma), B::dbl(sx));
            Fp3T ny = B::sub(B::mul(gamma, B::sub(sx, nx)), sy);
            out[idx++] = Coeff{sy, gamma, B::mul(gamma, sx)};
            sx = nx;
            sy = ny;
            const int n = naf[i];
            if (n != 0) {
                const Fp3T y = n > 0 ? qy : B::neg(qy);
                gamma = B::mul(B::sub(sy, y), inv3(B::sub(sx, qx)));
                nx = B::sub(B::sqr(gamma), B::add(sx, qx));
                ny = B::sub(B::mul(gamma, B::sub(sx, nx)), sy);
                out[idx++] = Coeff{y, gamma, B::mul(gamma, qx)};
                sx = nx;
                sy = ny;
            }
        }
    }

    // ------------------------------------------------------------------------------------------------ final exponentiation
    // signed-digit square and multiply for an element of norm one; digits most significant first, the first one non-zero
    // (fp6_2over3.rs:83-107)
    static GH_HD Fq6T cyclotomic_exp(const Fq6T& a, const int8_t* naf, int digits);
    // f^((p^6 - 1)/r) by the reference's split (mod.rs:224-272): (p^3 - 1)(p + 1), then p + w0 with w0 = +T on the element
    // itself.  w0naf: the W0_DIGITS signed digits of T.  f = 0 gives 0.
    static GH_HD Fq6T final_exponentiation(const Fq6T& f, const int8_t* w0naf);
};

GH_HD Fq6T Mnt6Pairing::cyclotomic_exp(const Fq6T& a, const int8_t* naf, int digits) {
    const Fq6T ai = unitary_inverse(a);
    Fq6T res = naf[0] > 0 ? a : ai;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int i = 1; i < digits; i++) {
        res = gt_cyclo_sqr_call<Mnt6Pairing>(res);
        const int n = naf[i];
        if (n != 0) res = gt_mul_call<Mnt6Pairing>(res, n > 0 ? a : ai);
    }
    return res;
}

GH_HD Fq6T Mnt6Pairing::final_exponentiation(const Fq6T& f, const int8_t* w0naf) {
    const Fq6T fi = inverse(f);
    const Fq6T g = gt_mul_call<Mnt6Pairing>(frobenius(f, 3), fi);            // f^(p^3 - 1)
    const Fq6T elt = gt_mul_call<Mnt6Pairing>(frobenius(g, 1), g);           // ... ^(p + 1)
    const Fq6T w1 = frobenius(elt, 1);                                       // m1 = 1
    const Fq6T w0 = cyclotomic_exp(elt, w0naf, W0_DIGITS);
    return gt_mul_call<Mnt6Pairing>(w1, w0);
}

}  // namespace gh
