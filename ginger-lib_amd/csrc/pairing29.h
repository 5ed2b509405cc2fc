// pairing29.h -- the reduced ate pairings of MNT4-753 and MNT6-753 over the fields of fp29.h: the target-field tower, the two
// kinds of Miller step and the final exponentiation, written once as PairingTower over a base policy B, and the MNT4-753
// engine Mnt4Pairing.  The MNT6-753 engine Mnt6Pairing is pairing29_mnt6.h.  Plain GH_HD code: the same text runs in the
// kernels of pairing_impl.h and, compiled by g++, in tests/host_shim/pairing_shim.cpp and pairing6_shim.cpp.  DESIGN.md section 14.
//
// Reference: algebra/src/curves/models/mnt4/mod.rs (Miller loop :157-224, final exponentiation :226-269),
// algebra/src/fields/models/fp4.rs, parameters algebra/src/curves/mnt4753/mod.rs:27-103; for MNT6-753
// algebra/src/curves/models/mnt6/mod.rs (Miller loop :158-222, final exponentiation :224-272),
// algebra/src/fields/models/fp6_2over3.rs, fp3.rs, parameters algebra/src/curves/mnt6753/mod.rs:27-104.
//
// The reduced pairing is unique: any correct Miller function followed by the full exponent (p^k - 1)/r gives the reference's
// value, and a line may be scaled by any factor from the tower's base (the exponent's factor p^2 - 1 on MNT4, p^3 - 1 on MNT6,
// removes it).  So the device is free to choose its line formulas; parity with the reference is defined on the value after the
// final exponentiation only.
//
//   The tower is GT = B[Y]/(Y^2 - w) over the base B = Fq[w]/(w^D - nr); the twist is w = (0, 1, ..):
//       MNT4-753   Fq4 over Fq2 = Fq[X]/(X^2 - 13), w = X;   a' = (26, 0)
//       MNT6-753   Fq6 over Fq3 = Fq[u]/(u^3 - 11), w = u;   a' = 11 u^2 = (0, 0, 11)
//   Lines, in the reference's scaling (mnt4/mod.rs:172-189, mnt6/mod.rs:173-191): for the running point S = (x', y') of the
//   twist and the slope gamma,
//       l(P) = ( c ,  gamma x' - gamma w x_P - y' )  in B x B,   c = 13 y_P on MNT4, y_P u^2 on MNT6.
//   After the loop: the MNT4 loop count is negative, so the unitary inverse follows, and the last chunk of the final exponent
//   is p + w0 with w0 = -(T - 1) applied to the inverse; the MNT6 count T = p - r is positive: nothing follows the loop, and
//   the chunk is p + T with T applied to the element itself.
//   prepared Q: the table holds the reference's (r_y, gamma, gamma_x) per step (mnt4/mod.rs:100-154, mnt6/mod.rs:101-155)
//       with the sign of an addition step folded into r_y; the line's c0 is sparse, (13 y_P, 0) or (0, 0, y_P): D products
//       for gamma w x_P and the sparse product, the 8-product mul_by_023 or the 15-product mul_by_2345.  10 / 18 products per step.
//   variable Q: the running point is Jacobian (X, Y, Z, T = Z^2) and the line is scaled by its denominator, so no inversion.
//       A product in B is 3 / 6 products, a square 2 / 5; the full GT product 9 / 18.
//       doubling   dbl-2007-bl with the line's three products read off as squarings: 11 S + 1 M in B = 25 / 61 products, the
//                  line 4 / 6, the GT product: 38 / 85.   The line is  (c 2 Z3 T ,  2 F X - 2 F T w x_P - 4 Y^2); on MNT6
//                  its c0 is a full Fq3 element.
//       addition   madd-2007-bl, 7 M + 4 S: 28 / 62 products, the line 8 / 15 (L1 (x_Q - w x_P) - y_Q Z3 ; c Z3; w x_P =
//                  (0, x_P, ..)), the GT product: 45 / 95.
//   The affine alternative (the reference's own, with one Fq2 inversion per step: 2 S + 2 M + a safegcd inversion of ~42
//   products) costs 69 per doubling and 66 per addition on MNT4, so 376 x 69 + 123 x 66 = 34.1 K products per variable pair
//   against 376 x 38 + 123 x 45 = 19.8 K for the Jacobian form, which is the one built.  On MNT6 the Jacobian form takes
//   376 x 85 + 123 x 95 = 43.6 K products per variable pair, 376 x 12 = 4.5 K for the squarings of f.  (Squarings counted
//   as products.)
//
// An engine is `struct E : PairingTower<E, B>` and supplies what differs, under these names: PF, G1, G2 and the digit counts;
// mul_nr (times w), mul_fp, inv (1 / a in B), mul_a (times a'), sub_twist_px (x_Q - w x_P), g1_pre and line_embed (the line's
// Fq factor and how its product with an element of B enters c0), mul_by_line over its sparse product, frobenius, miller_end
// and final_exponentiation.  The kernels of pairing_impl.h are templates over the engine and take every width from it.
#pragma once
#include "ec29.h"
#include "pairing_constants_gen.h"

namespace gh {

// an element of the target field over the base element BT
template <class BT> struct TowerGT { BT c0, c1; };
typedef TowerGT<Fp2T> Fq4T;
typedef TowerGT<Fp3T> Fq6T;

template <class E, class Base> struct PairingTower {
    typedef Base B;                       // the base of the tower, with out-of-line Fq products
    typedef typename B::T BT;
    typedef TowerGT<BT> GT;
    static constexpr int BDEG = B::DEG;   // Fq coefficients of a tower coordinate (of G2, of half a GT)

    // ------------------------------------------------------------------------------------------------ GT
    static GH_HD GT one() { return GT{B::one(), B::zero()}; }
    static GH_HD bool eq(const GT& a, const GT& b) { return B::eq(a.c0, b.c0) && B::eq(a.c1, b.c1); }
    // Karatsuba over B: 3 products in B = 9 / 18 products                  (fp4.rs, fp6_2over3.rs mul_assign)
    static GH_HD GT mul(const GT& a, const GT& b) {
        const BT v0 = B::mul(a.c0, b.c0), v1 = B::mul(a.c1, b.c1);
        const BT s = B::mul(B::add(a.c0, a.c1), B::add(b.c0, b.c1));
        return GT{B::add(v0, E::mul_nr(v1)), B::sub(B::sub(s, v0), v1)};
    }
    // 2 products in B = 6 / 12 products                                    (fp4.rs:183-199, fp6_2over3.rs:178-195)
    static GH_HD GT sqr(const GT& a) {
        const BT ab = B::mul(a.c0, a.c1);
        const BT t = B::mul(B::add(E::mul_nr(a.c1), a.c0), B::add(a.c0, a.c1));
        return GT{B::sub(B::sub(t, ab), E::mul_nr(ab)), B::dbl(ab)};
    }
    // zero gives zero                                                      (fp4.rs:201-217, fp6_2over3.rs:197-216)
    static GH_HD GT inverse(const GT& a) {
        const BT t = E::inv(B::sub(B::sqr(a.c0), E::mul_nr(B::sqr(a.c1))));
        return GT{B::mul(a.c0, t), B::neg(B::mul(a.c1, t))};
    }
    static GH_HD GT unitary_inverse(const GT& a) { return GT{a.c0, B::neg(a.c1)}; }         // fp4.rs:70-72, fp6_2over3.rs:79-81
    // for a of norm one over B (after the easy part), c0^2 - w c1^2 = 1: 2 squarings in B = 4 / 10 products    (fp4.rs:74-81)
    static GH_HD GT cyclotomic_square(const GT& s) {
        const BT a = B::sqr(s.c1);
        const BT c = B::sub(B::sqr(B::add(s.c1, s.c0)), a);
        const BT d = E::mul_nr(a);
        const BT e = B::sub(c, d);
        return GT{B::add(B::dbl(d), B::one()), B::sub(e, B::one())};
    }

    // ------------------------------------------------------------------------------------------------ Miller steps
    // what a pair brings to every step: x_P and the line's Fq factor (E::g1_pre: 13 y_P on MNT4, y_P on MNT6)
    struct G1Pre { Fp px, c0; };
    static GH_HD const Fp& line_c0(const G1Pre& P) { return P.c0; }
    // the running point of a variable Q: Jacobian, t = z^2
    struct G2Run { BT x, y, z, t; };
    // one entry of a prepared table: the reference's G2PreparedCoefficients, r_y being -+y_Q in an addition step
    struct Coeff { BT r_y, gamma, gamma_x; };

    // twist x_P v
    static GH_HD BT twist_px(const BT& v, const Fp& px) { return E::mul_nr(E::mul_fp(v, px)); }

    // R <- 2 R, returns the tangent's value at P (scaled by 2 Z3 T): 38 / 85 products with the GT product that follows
    static GH_HD GT dbl_step(G2Run& R, const G1Pre& P) {
        const BT A = B::sqr(R.t), Bq = B::sqr(R.x), C = B::sqr(R.y), D = B::sqr(C);
        const BT E_ = B::sub(B::sub(B::sqr(B::add(R.x, C)), Bq), D);
        const BT F = B::add(B::add(B::dbl(Bq), Bq), E::mul_a(A));
        const BT G = B::sqr(F);
        const BT E2 = B::dbl(E_);
        const BT x3 = B::sub(G, B::dbl(E2));
        const BT D8 = B::dbl(B::dbl(B::dbl(D)));
        const BT y3 = B::sub(B::mul(F, B::sub(E2, x3)), D8);
        const BT z3 = B::sub(B::sub(B::sqr(B::add(R.y, R.z)), C), R.t);
        const BT t3 = B::sqr(z3);
        const BT cH = B::sub(B::sub(B::sqr(B::add(z3, R.t)), t3), A);        // 2 Z3 T
        const BT cJ = B::sub(B::sub(B::sqr(B::add(F, R.t)), G), A);          // 2 F T
        const BT cL = B::sub(B::sub(B::sqr(B::add(F, R.x)), G), Bq);         // 2 F X
        GT l;
        l.c0 = E::line_embed(E::mul_fp(cH, P.c0));
        l.c1 = B::sub(B::sub(cL, twist_px(cJ, P.px)), B::dbl(B::dbl(C)));
        R = G2Run{x3, y3, z3, t3};
        return l;
    }
    // R <- R + Q for Q = (qx, qy) affine (qy negated by the caller for a digit -1), returns the chord's value at P (scaled
    // by Z3): 45 / 95 products with the GT product that follows.  R = +-Q gives Z3 = 0 and a zero line: never for a point of order r.
    static GH_HD GT add_step(G2Run& R, const BT& qx, const BT& qy, const G1Pre& P) {
        const BT H = B::sub(B::mul(qx, R.t), R.x);
        const BT S2 = B::mul(B::mul(qy, R.z), R.t);
        const BT I = B::sqr(H);
        const BT E_ = B::dbl(B::dbl(I));
        const BT J = B::mul(H, E_);
        const BT V = B::mul(R.x, E_);
        const BT L1 = B::dbl(B::sub(S2, R.y));
        const BT x3 = B::sub(B::sub(B::sqr(L1), J), B::dbl(V));
        const BT y3 = B::sub(B::mul(L1, B::sub(V, x3)), B::dbl(B::mul(R.y, J)));
        const BT z3 = B::sub(B::sub(B::sqr(B::add(R.z, H)), R.t), I);
        const BT t3 = B::sqr(z3);
        GT l;
        l.c0 = E::line_embed(E::mul_fp(z3, P.c0));
        l.c1 = B::sub(B::mul(L1, E::sub_twist_px(qx, P.px)), B::mul(qy, z3));
        R = G2Run{x3, y3, z3, t3};
        return l;
    }
    // the line of a table entry at P: c0 is sparse (line_c0 in its one place), c1 returned
    static GH_HD BT prepared_line(const Coeff& c, const G1Pre& P) {
        return B::sub(B::sub(c.gamma_x, twist_px(c.gamma, P.px)), c.r_y);
    }
    // the reference's ate_precompute_g2 for Q = (qx, qy) not at infinity: TABLE_STEPS entries.  naf: the ATE_DIGITS signed
    // digits of the loop count, most significant first.  A zero denominator inverts to zero.
    static GH_HD void prepare_g2(const BT& qx, const BT& qy, const int8_t* naf, Coeff* out) {
        BT sx = qx, sy = qy;
        int idx = 0;
        for (int i = 0; i < E::ATE_DIGITS; i++) {
            const BT xx = B::sqr(sx);
            BT gamma = B::mul(B::add(B::add(B::dbl(xx), xx), E::mul_a(B::one())), E::inv(B::dbl(sy)));
            BT nx = B::sub(B::sqr(gamma), B::dbl(sx));
            BT ny = B::sub(B::mul(gamma, B::sub(sx, nx)), sy);
            out[idx++] = Coeff{sy, gamma, B::mul(gamma, sx)};
            sx = nx;
            sy = ny;
            const int n = naf[i];
            if (n != 0) {
                const BT y = n > 0 ? qy : B::neg(qy);
                gamma = B::mul(B::sub(sy, y), E::inv(B::sub(sx, qx)));
                nx = B::sub(B::sqr(gamma), B::add(sx, qx));
                ny = B::sub(B::mul(gamma, B::sub(sx, nx)), sy);
                out[idx++] = Coeff{y, gamma, B::mul(gamma, qx)};
                sx = nx;
                sy = ny;
            }
        }
    }

    // signed-digit square and multiply for an element of norm one; digits most significant first, the first one non-zero
    // (fp4.rs:83-109, fp6_2over3.rs:83-107)
    static GH_HD GT cyclotomic_exp(const GT& a, const int8_t* naf, int digits);
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

template <class E, class Base>
GH_HD typename PairingTower<E, Base>::GT PairingTower<E, Base>::cyclotomic_exp(const GT& a, const int8_t* naf, int digits) {
    const GT ai = unitary_inverse(a);
    GT res = naf[0] > 0 ? a : ai;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int i = 1; i < digits; i++) {
        res = gt_cyclo_sqr_call<E>(res);
        const int n = naf[i];
        if (n != 0) res = gt_mul_call<E>(res, n > 0 ? a : ai);
    }
    return res;
}

// miller_end(prod_j miller(P_j, Q_j)) over k variable pairs of one row, on the host or in one thread: what the kernels of
// pairing_impl.h compute with the running points in a slab.  skip[j]: the pair contributes one (a point at infinity).
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

// ---------------------------------------------------------------------------------------------------- MNT4-753
struct Mnt4Pairing : PairingTower<Mnt4Pairing, F2<P4, 13, false>> {
    typedef P4 PF;
    typedef Mnt4G1 G1;
    typedef Mnt4G2 G2;
    static constexpr int ATE_DIGITS = GH_MNT4_ATE_DIGITS;
    static constexpr int W0_DIGITS = GH_MNT4_W0_DIGITS;
    static constexpr int TABLE_STEPS = GH_MNT4_ATE_DIGITS + GH_MNT4_ATE_NONZERO;    // 499 entries of 3 Fq2

    static GH_HD Fp mul13(const Fp& a) { return fp_mul_small<P4, 13>(a); }
    // times X, the generator of Fq2: the non-residue of Fq4 over Fq2 and the twist       (fp4.rs:64-68)
    static GH_HD Fp2T mul_nr(const Fp2T& a) { return Fp2T{mul13(a.c1), a.c0}; }
    static GH_HD Fp2T mul_fp(const Fp2T& a, const Fp& s) { return Fp2T{B::mulx(a.c0, s), B::mulx(a.c1, s)}; }
    // 1 / (a0 + a1 X) = (a0 - a1 X) / (a0^2 - 13 a1^2); zero gives zero       (fp2.rs inverse)
    static GH_HD Fp2T inv(const Fp2T& a) {
        const Fp n = fp_sub<P4>(B::sqrx(a.c0), mul13(B::sqrx(a.c1)));
        const Fp ni = fp_inv<P4>(n);
        return Fp2T{B::mulx(a.c0, ni), fp_neg<P4>(B::mulx(a.c1, ni))};
    }
    static GH_HD Fp2T mul_a(const Fp2T& a) { return G2::mul_by_a(a); }
    // x_Q - twist x_P: the twist is X, so x_P leaves coefficient 1
    static GH_HD Fp2T sub_twist_px(const Fp2T& qx, const Fp& px) { return Fp2T{qx.c0, fp_sub<P4>(qx.c1, px)}; }
    static GH_HD G1Pre g1_pre(const Fp& x, const Fp& y) { return G1Pre{x, mul13(y)}; }
    // the c0 of a variable step's line from v (13 y_P): as it is
    static GH_HD const Fp2T& line_embed(const Fp2T& v) { return v; }

    // times (c0: [b0, 0], c1: b1): 2 + 3 + 3 = 8 products                               (fp4.rs:112-126)
    static GH_HD Fq4T mul_by_023(const Fq4T& a, const Fp& b0, const Fp2T& b1) {
        const Fp2T v0 = mul_fp(a.c0, b0), v1 = B::mul(a.c1, b1);
        const Fp2T s = B::mul(B::add(a.c0, a.c1), Fp2T{fp_add<P4>(b0, b1.c0), b1.c1});
        return Fq4T{B::add(v0, mul_nr(v1)), B::sub(B::sub(s, v0), v1)};
    }
    // times a prepared step's line (c0: [b0, 0], c1: b1)
    static GH_HD Fq4T mul_by_line(const Fq4T& a, const Fp& b0, const Fp2T& b1) { return mul_by_023(a, b0, b1); }
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
    // f^((p^4 - 1)/r) by the reference's split (mod.rs:226-269): (p^2 - 1), then p + w0 with w0 = -(T - 1) on the inverse.
    // w0naf: the W0_DIGITS signed digits of T - 1.  f = 0 gives 0.
    static GH_HD Fq4T final_exponentiation(const Fq4T& f, const int8_t* w0naf);
};

GH_HD Fq4T Mnt4Pairing::final_exponentiation(const Fq4T& f, const int8_t* w0naf) {
    const Fq4T fi = inverse(f);
    const Fq4T elt = gt_mul_call<Mnt4Pairing>(frobenius(f, 2), fi);          // f^(p^2 - 1)
    const Fq4T elt_inv = gt_mul_call<Mnt4Pairing>(frobenius(fi, 2), f);
    const Fq4T w1 = frobenius(elt, 1);                           // m1 = 1
    const Fq4T w0 = cyclotomic_exp(elt_inv, w0naf, W0_DIGITS);
    return gt_mul_call<Mnt4Pairing>(w1, w0);
}

}  // namespace gh
