// pairing29.h -- the MNT4-753 reduced ate pairing over the fields of fp29.h: the target-field tower, the two kinds of Miller
// step and the final exponentiation.  Plain GH_HD code: the same text runs in the kernels of pairing.hip and, compiled by
// g++, in tests/host_shim/pairing_shim.cpp.  DESIGN.md section 14.
//
// Reference: algebra/src/curves/models/mnt4/mod.rs (Miller loop :157-224, final exponentiation :226-269),
// algebra/src/fields/models/fp4.rs, parameters algebra/src/curves/mnt4753/mod.rs:27-103.
//
// The reduced pairing is unique: any correct Miller function followed by the full exponent (p^4 - 1)/r gives the reference's
// value, and a line may be scaled by any factor from Fq2 (the exponent's factor p^2 - 1 removes it).  So the device is free to
// choose its line formulas; parity with the reference is defined on the value after the final exponentiation only.
//
//   Fq4 = Fq2[Y]/(Y^2 - X), Fq2 = Fq[X]/(X^2 - 13); twist = X = (0, 1); a' = (26, 0).
//   Lines, in the reference's scaling (mod.rs:172-189): for the running point S = (x', y') of the twist and the slope gamma,
//       l(P) = ( 13 y_P ,  gamma x' - gamma twist x_P - y' )  in Fq2 x Fq2.
//   prepared Q: the table holds the reference's (r_y, gamma, gamma_x) per step (mod.rs:100-154) with the sign of an addition
//       step folded into r_y; the line's c0 = (13 y_P, 0) is sparse: 2 products for gamma twist x_P and the 8-product
//       mul_by_023.  10 products per step.
//   variable Q: the running point is Jacobian (X, Y, Z, T = Z^2) and the line is scaled by its denominator, so no inversion:
//       doubling   dbl-2007-bl with the line's three products read off as squarings: 11 S + 1 M in Fq2 = 25 products, the line
//                  4, the full Fq4 product 9: 38.   The line is  (13 y_P 2 Z3 T ,  2 F X - 2 F T twist x_P - 4 Y^2).
//       addition   madd-2007-bl: 28 products, the line 8 (L1 (x_Q - twist x_P) - y_Q Z3 ; 13 y_P Z3; twist x_P = (0, x_P)), the Fq4 product 9: 45.
//   The affine alternative (the reference's own, with one Fq2 inversion per step: 2 S + 2 M + a safegcd inversion of ~42
//   products) costs 69 per doubling and 66 per addition, so 376 x 69 + 123 x 66 = 34.1 K products per variable pair against
//   376 x 38 + 123 x 45 = 19.8 K for the Jacobian form, which is the one built.  (Squarings counted as products.)
//
// The MNT6-753 engine (pairing29_mnt6.h) is an Fq6 tower over F3 with the interface of Mnt4Pairing below and its own step
// functions; the kernels of pairing_impl.h are templates over the engine and take every width from it.
#pragma once
#include "ec29.h"
#include "pairing_constants_gen.h"

namespace gh {

struct Fq4T { Fp2T c0, c1; };

struct Mnt4Pairing {
    typedef P4 PF;
    typedef F2<P4, 13, false> B;          // the base of the tower: Fq2 with out-of-line Fq products
    typedef Fq4T GT;
    typedef Mnt4G1 G1;
    typedef Mnt4G2 G2;
    static constexpr int ATE_DIGITS = GH_MNT4_ATE_DIGITS;
    static constexpr int W0_DIGITS = GH_MNT4_W0_DIGITS;
    static constexpr int TABLE_STEPS = GH_MNT4_ATE_DIGITS + GH_MNT4_ATE_NONZERO;    // 499 entries of 3 Fq2
    static constexpr int BDEG = 2;                   // Fq coefficients of a tower coordinate (of G2, of half a GT)

    static GH_HD Fp mul13(const Fp& a) { return fp_mul_small<P4, 13>(a); }
    // times X, the generator of Fq2: the non-residue of Fq4 over Fq2 and the twist       (fp4.rs:64-68)
    static GH_HD Fp2T mul_x(const Fp2T& a) { return Fp2T{mul13(a.c1), a.c0}; }
    static GH_HD Fp2T mul_fp(const Fp2T& a, const Fp& s) { return Fp2T{B::mulx(a.c0, s), B::mulx(a.c1, s)}; }
    // 1 / (a0 + a1 X) = (a0 - a1 X) / (a0^2 - 13 a1^2); zero gives zero       (fp2.rs inverse)
    static GH_HD Fp2T inv2(const Fp2T& a) {
        const Fp n = fp_sub<P4>(B::sqrx(a.c0), mul13(B::sqrx(a.c1)));
        const Fp ni = fp_inv<P4>(n);
        return Fp2T{B::mulx(a.c0, ni), fp_neg<P4>(B::mulx(a.c1, ni))};
    }

    // ------------------------------------------------------------------------------------------------ Fq4
    static GH_HD Fq4T one() { return Fq4T{B::one(), B::zero()}; }
    static GH_HD bool eq(const Fq4T& a, const Fq4T& b) { return B::eq(a.c0, b.c0) && B::eq(a.c1, b.c1); }
    // Karatsuba over Fq2: 3 Fq2 products = 9 products                                   (fp4.rs mul_assign)
    static GH_HD Fq4T mul(const Fq4T& a, const Fq4T& b) {
        const Fp2T v0 = B::mul(a.c0, b.c0), v1 = B::mul(a.c1, b.c1);
        const Fp2T s = B::mul(B::add(a.c0, a.c1), B::add(b.c0, b.c1));
        return Fq4T{B::add(v0, mul_x(v1)), B::sub(B::sub(s, v0), v1)};
    }
    // 2 Fq2 products = 6 products                                                       (fp4.rs:183-199)
    static GH_HD Fq4T sqr(const Fq4T& a) {
        const Fp2T ab = B::mul(a.c0, a.c1);
        const Fp2T t = B::mul(B::add(mul_x(a.c1), a.c0), B::add(a.c0, a.c1));
        return Fq4T{B::sub(B::sub(t, ab), mul_x(ab)), B::dbl(ab)};
    }
    // times (c0: [b0, 0], c1: b1): 2 + 3 + 3 = 8 products                               (fp4.rs:112-126)
    static GH_HD Fq4T mul_by_023(const Fq4T& a, const Fp& b0, const Fp2T& b1) {
        const Fp2T v0 = mul_fp(a.c0, b0), v1 = B::mul(a.c1, b1);
        const Fp2T s = B::mul(B::add(a.c0, a.c1), Fp2T{fp_add<P4>(b0, b1.c0), b1.c1});
        return Fq4T{B::add(v0, mul_x(v1)), B::sub(B::sub(s, v0), v1)};
    }
    // times a prepared step's line (c0: [b0, 0], c1: b1), the name every engine has
    static GH_HD Fq4T mul_by_line(const Fq4T& a, const Fp& b0, const Fp2T& b1) { return mul_by_023(a, b0, b1); }
    // zero gives zero                                                                   (fp4.rs:201-217)
    static GH_HD Fq4T inverse(const Fq4T& a) {
        const Fp2T t = inv2(B::sub(B::sqr(a.c0), mul_x(B::sqr(a.c1))));
        return Fq4T{B::mul(a.c0, t), B::neg(B::mul(a.c1, t))};
    }
    static GH_HD Fq4T unitary_inverse(const Fq4T& a) { return Fq4T{a.c0, B::neg(a.c1)}; }         // fp4.rs:70-72
    // what follows the Miller loop: the trace is negative                               (mod.rs:219-221)
    static GH_HD Fq4T miller_end(const Fq4T& f) { return unitary_inverse(f); }
    static GH_HD Fp frob4_coeff(int k) {
        switch (k & 3) {
            case 1: { const uint32_t c[NL] = GH_MNT4_FROB4_C1_1_I29; return fp_const<P4>(c); }
            case 2: { const uint32_t c[NL] = GH_MNT4_FROB4_C1_2_I29; return fp_const<P4>(c); }
            case 3: { const uint32_t c[NL] = GH_MNT4_FROB4_C1_3_I29; return fp_const<P4>(c); }
        }
        return fp_one<P4>();
    }
    // a^(p^k): the Fq2 Frobenius coefficients are 1 and -1                             (fp2.rs / fp4.rs frobenius_map)
    static GH_HD Fq4T frobenius(const Fq4T& a, int k) {
        Fq4T r = a;
        if (k & 1) { r.c0.c1 = fp_neg<P4>(r.c0.c1); r.c1.c1 = fp_neg<P4>(r.c1.c1); }
        if (k & 3) r.c1 = mul_fp(r.c1, frob4_coeff(k));
        return r;
    }
    // for a of norm one over Fq2 (after the easy part): 2 Fq2 squarings = 4 products    (fp4.rs:74-81)
    static GH_HD Fq4T cyclotomic_square(const Fq4T& s) {
        const Fp2T a = B::sqr(s.c1);
        const Fp2T c = B::sub(B::sqr(B::add(s.c1, s.c0)), a);
        const Fp2T d = mul_x(a);
        const Fp2T e = B::sub(c, d);
        return Fq4T{B::add(B::dbl(d), B::one()), B::sub(e, B::one())};
    }

    // ------------------------------------------------------------------------------------------------ Miller steps
    // what a pair brings to every step: x_P, 13 y_P
    struct G1Pre { Fp px, py13; };
    static GH_HD G1Pre g1_pre(const Fp& x, const Fp& y) { return G1Pre{x, mul13(y)}; }
    static GH_HD const Fp& line_c0(const G1Pre& P) { return P.py13; }
    // the running point of a variable Q: Jacobian, t = z^2
    struct G2Run { Fp2T x, y, z, t; };
    // one entry of a prepared table: the reference's G2PreparedCoefficients, r_y being -+y_Q in an addition step
    struct Coeff { Fp2T r_y, gamma, gamma_x; };

    // twist x_P v
    static GH_HD Fp2T twist_px(const Fp2T& v, const Fp& px) { return mul_x(mul_fp(v, px)); }

    // R <- 2 R, returns the tangent's value at P (scaled by 2 Z3 T): 38 products with the Fq4 product that follows
    static GH_HD Fq4T dbl_step(G2Run& R, const G1Pre& P) {
        const Fp2T A = B::sqr(R.t), Bq = B::sqr(R.x), C = B::sqr(R.y), D = B::sqr(C);
        const Fp2T E = B::sub(B::sub(B::sqr(B::add(R.x, C)), Bq), D);
        const Fp2T F = B::add(B::add(B::dbl(Bq), Bq), G2::mul_by_a(A));
        const Fp2T G = B::sqr(F);
        const Fp2T E2 = B::dbl(E);
        const Fp2T x3 = B::sub(G, B::dbl(E2));
        const Fp2T D8 = B::dbl(B::dbl(B::dbl(D)));
        const Fp2T y3 = B::sub(B::mul(F, B::sub(E2, x3)), D8);
        const Fp2T z3 = B::sub(B::sub(B::sqr(B::add(R.y, R.z)), C), R.t);
        const Fp2T t3 = B::sqr(z3);
        const Fp2T cH = B::sub(B::sub(B::sqr(B::add(z3, R.t)), t3), A);        // 2 Z3 T
        const Fp2T cJ = B::sub(B::sub(B::sqr(B::add(F, R.t)), G), A);          // 2 F T
        const Fp2T cL = B::sub(B::sub(B::sqr(B::add(F, R.x)), G), Bq);         // 2 F X
        Fq4T l;
        l.c0 = mul_fp(cH, P.py13);
        l.c1 = B::sub(B::sub(cL, twist_px(cJ, P.px)), B::dbl(B::dbl(C)));
        R = G2Run{x3, y3, z3, t3};
        return l;
    }
    // R <- R + Q for Q = (qx, qy) affine (qy negated by the caller for a digit -1), returns the chord's value at P (scaled
    // by Z3): 45 products with the Fq4 product that follows.  R = +-Q gives Z3 = 0 and a zero line: never for a point of order r.
    static GH_HD Fq4T add_step(G2Run& R, const Fp2T& qx, const Fp2T& qy, const G1Pre& P) {
        const Fp2T H = B::sub(B::mul(qx, R.t), R.x);
        const Fp2T S2 = B::mul(B::mul(qy, R.z), R.t);
        const Fp2T I = B::sqr(H);
        const Fp2T E = B::dbl(B::dbl(I));
        const Fp2T J = B::mul(H, E);
        const Fp2T V = B::mul(R.x, E);
        const Fp2T L1 = B::dbl(B::sub(S2, R.y));
        const Fp2T x3 = B::sub(B::sub(B::sqr(L1), J), B::dbl(V));
        const Fp2T y3 = B::sub(B::mul(L1, B::sub(V, x3)), B::dbl(B::mul(R.y, J)));
        const Fp2T z3 = B::sub(B::sub(B::sqr(B::add(R.z, H)), R.t), I);
        const Fp2T t3 = B::sqr(z3);
        Fq4T l;
        l.c0 = mul_fp(z3, P.py13);
        l.c1 = B::sub(B::mul(L1, Fp2T{qx.c0, fp_sub<P4>(qx.c1, P.px)}), B::mul(qy, z3));
        R = G2Run{x3, y3, z3, t3};
        return l;
    }
    // the line of a table entry at P: c0 = (13 y_P, 0), c1 returned
    static GH_HD Fp2T prepared_line(const Coeff& c, const G1Pre& P) {
        return B::sub(B::sub(c.gamma_x, twist_px(c.gamma, P.px)), c.r_y);
    }
    // the reference's ate_precompute_g2 (mod.rs:100-154) for Q = (qx, qy) not at infinity: TABLE_STEPS entries.  naf: the
    // ATE_DIGITS signed digits of the loop count, most significant first.  A zero denominator inverts to zero.
    static GH_HD void prepare_g2(const Fp2T& qx, const Fp2T& qy, const int8_t* naf, Coeff* out) {
        Fp2T sx = qx, sy = qy;
        int idx = 0;
        for (int i = 0; i < ATE_DIGITS; i++) {
            const Fp2T xx = B::sqr(sx);
            Fp2T a = B::zero();
            a.c0 = fp_one<P4>();
            Fp2T gamma = B::mul(B::add(B::add(B::dbl(xx), xx), G2::mul_by_a(a)), inv2(B::dbl(sy)));
            Fp2T nx = B::sub(B::sqr(gamma), B::dbl(sx));
            Fp2T ny = B::sub(B::mul(gamma, B::sub(sx, nx)), sy);
            out[idx++] = Coeff{sy, gamma, B::mul(gamma, sx)};
            sx = nx;
            sy = ny;
            const int n = naf[i];
            if (n != 0) {
                const Fp2T y = n > 0 ? qy : B::neg(qy);
                gamma = B::mul(B::sub(sy, y), inv2(B::sub(sx, qx)));
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
    // (fp4.rs:83-109)
    static GH_HD Fq4T cyclotomic_exp(const Fq4T& a, const int8_t* naf, int digits);
    // f^((p^4 - 1)/r) by the reference's split (mod.rs:226-269): (p^2 - 1), then p + w0 with w0 = -(T - 1) on the inverse.
    // w0naf: the W0_DIGITS signed digits of T - 1.  f = 0 gives 0.
    static GH_HD Fq4T final_exponentiation(const Fq4T& f, const int8_t* w0naf);
};

// out-of-line instances: one body per operation instead of one per use (the long-branch note of ec29.h)
template <class E> GH_HD_NOINLINE typename E::GT gt_mul_call(const typename E::GT& a, const typename E::GT& b) { return E::mul(a, b); }
template <class E> GH_HD_NOINLINE typename E::GT gt_sqr_call(const typename E::GT& a) { return E::sqr(a); }
template <class E> GH_HD_NOINLINE typename E::GT gt_cyclo_sqr_call(const typename E::GT& a) { return E::cyclotomic_square(a); }
template <class E> GH_HD_NOINLINE typename E::GT gt_mul_by_line_call(const typename E::GT& a, const Fp& b0, const typename E::B::T& b1) {
    return E::mul_by_line(a, b0, b1);
}
template <class E> GH_HD_NOINLINE typename E::GT dbl_step_call(typename E::G2Run& R, const typename E::G1Pre& P) { return E::dbl_step(R, P); }
template <class E>
GH_HD_NOINLINE typename E::GT add_step_call(typename E::G2Run& R, const typename E::B::T& qx, const typename E::B::T& qy, const typename E::G1Pre& P) {
    return E::add_step(R, qx, qy, P);
}

GH_HD Fq4T Mnt4Pairing::cyclotomic_exp(const Fq4T& a, const int8_t* naf, int digits) {
    const Fq4T ai = unitary_inverse(a);
    Fq4T res = naf[0] > 0 ? a : ai;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int i = 1; i < digits; i++) {
        res = gt_cyclo_sqr_call<Mnt4Pairing>(res);
        const int n = naf[i];
        if (n != 0) res = gt_mul_call<Mnt4Pairing>(res, n > 0 ? a : ai);
    }
    return res;
}

GH_HD Fq4T Mnt4Pairing::final_exponentiation(const Fq4T& f, const int8_t* w0naf) {
    const Fq4T fi = inverse(f);
    const Fq4T elt = gt_mul_call<Mnt4Pairing>(frobenius(f, 2), fi);          // f^(p^2 - 1)
    const Fq4T elt_inv = gt_mul_call<Mnt4Pairing>(frobenius(fi, 2), f);
    const Fq4T w1 = frobenius(elt, 1);                           // m1 = 1
    const Fq4T w0 = cyclotomic_exp(elt_inv, w0naf, W0_DIGITS);
    return gt_mul_call<Mnt4Pairing>(w1, w0);
}

// final_exp(prod_j miller(P_j, Q_j)) over k variable pairs of one row, on the host or in one thread: what the kernels of
// pairing.hip compute with the running points in a slab.  skip[j]: the pair contributes one (a point at infinity).
template <class E>
GH_HD typename E::GT miller_variable(const typename E::G1Pre* P, const typename E::B::T* qx, const typename E::B::T* qy, const bool* skip, int k,
                                     const int8_t* naf) {
    typename E::G2Run R[3];
    for (int j = 0; j < k; j++) R[j] = typename E::G2Run{qx[j], qy[j], E::B::one(), E::B::one()};
    typename E::GT f = E::one();
    for (int i = 0; i < E::ATE_DIGITS; i++) {
        f = gt_sqr_call<E>(f);
        for (int j = 0; j < k; j++)
            if (!skip[j]) f = gt_mul_call<E>(f, dbl_step_call<E>(R[j], P[j]));
        const int n = naf[i];
        if (n != 0)
            for (int j = 0; j < k; j++)
                if (!skip[j]) f = gt_mul_call<E>(f, add_step_call<E>(R[j], qx[j], n > 0 ? qy[j] : E::B::neg(qy[j]), P[j]));
    }
    return E::miller_end(f);
}
GH_HD Fq4T mnt4_miller_variable(const Mnt4Pairing::G1Pre* P, const Fp2T* qx, const Fp2T* qy, const bool* skip, int k, const int8_t* naf) {
    return miller_variable<Mnt4Pairing>(P, qx, qy, skip, k, naf);
}

}  // namespace gh
