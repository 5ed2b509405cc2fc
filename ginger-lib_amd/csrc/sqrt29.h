// sqrt29.h -- square roots in Fq, Fq2 and Fq3 over the fields of fp29.h, and what point validation builds on them: parity,
// the subgroup test r P = infinity by a fixed signed-digit chain, and one row of compress / decompress.  Plain GH_HD code: the
// same text runs in the kernels of points.hip and, compiled by g++, in tests/host_shim/points_shim.cpp.  DESIGN.md section 15.
//
// Reference: algebra/src/fields/macros.rs:52-105 (sqrt_impl: Tonelli-Shanks), fields/models/fp2.rs:186-214 (the complex
// method), curves/models/short_weierstrass_projective.rs:82-121, :205-268 (get_point_from_x_and_parity, compress, decompress).
//
// Bounded loops.  The reference's Tonelli-Shanks asks for the Legendre symbol first and then loops `while !b.is_one()`.  Here
// nothing waits for the input to behave: every loop has a compile-time trip count, every input -- a non-residue, zero -- runs
// the same S - 1 rounds, and whether a root exists is read off at the end from x^2 == a.  With q - 1 = 2^S t:
//     w = a^((t-1)/2),  x = a w,  b = x w = a^t,  z = c^t for a non-residue c (order 2^S);   invariant x^2 = a b
//     for i = S-1 .. 1:  if b^(2^(i-1)) != 1 { x *= z; b *= z^2 }   z = z^2            (b^(2^i) = 1 going in, if a is a square)
// A square ends with b = 1 and x^2 = a; a non-residue keeps b of order 2^S / 2^i and ends with x^2 = a b != a.  So "a root
// exists" is exactly the reference's Legendre answer, and zero gives the root zero as sqrt_impl's `Zero => Some(self)`.
// Which of +-x comes out depends on the choice of c and is not the reference's; decompression normalises by parity.
// Cost: EBITS squarings and about EBITS / 2 products for the power, (S-1)(S-2)/2 squarings and at most 2 (S-1) products after it.
//
// Fq2, the reference's quirk (fp2.rs:188-190): an element with c1 = 0 is rooted in Fq only.  A c0 that is a non-residue of
// Fq does have a root in Fq2 (sqrt(c0 / 13) X), but the reference returns None, and so does fq2_sqrt: the statuses of
// decompression are the reference's.
#pragma once
#include "ec29.h"
#include "sqrt_constants_gen.h"

namespace gh {

// ---------------------------------------------------------------------------------------------------- canonical values, parity
// the integer itself in 26 limbs (out of the Montgomery form)
template <class P> GH_HD Fp fp_canon(const Fp& a) {
    Fp one = fp_zero();
    one.l[0] = 1;
    return fp_mul_call<P>(a, one);
}
// an integer of 24 LE words below p?  (26 x 29 = 754 bits: anything above them is not)
template <class P> GH_HD bool fp_words_below_p(const uint32_t* w) {
    if (w[23] >> 18) return false;
    const Fp a = fp_unpack(w);
    int32_t bw = 0;
    GH_UNROLL for (int i = 0; i < NL; i++) bw = ((int32_t)a.l[i] - (int32_t)P::P[i] + bw) >> 31;
    return bw != 0;
}
// an integer below p (24 LE words) -> internal Montgomery, and back
template <class P> GH_HD Fp fp_from_canon_words(const uint32_t* w) { return fp_mul_call<P>(fp_unpack(w), fp_const<P>(P::R2I)); }
template <class P> GH_HD void fp_to_canon_words(uint32_t* w, const Fp& a) { fp_pack(w, fp_canon<P>(a)); }

// is_odd of the canonical value; for a tower the parity of the highest non-zero coefficient (fp2.rs:101-103, fp3.rs:135-139)
template <class F, class P> GH_HD bool f_is_odd(const typename F::T& a) {
    bool odd = false, found = false;
    GH_UNROLL for (int i = F::DEG - 1; i >= 0; i--) {
        const Fp& c = F::comp(a, i);
        if (!found && (i == 0 || !fp_is_zero(c))) {
            odd = (fp_canon<P>(c).l[0] & 1u) != 0;
            found = true;
        }
    }
    return odd;
}

// ---------------------------------------------------------------------------------------------------- Tonelli-Shanks
// one out-of-line body per field and operation (the long-branch note of ec29.h); Fq's own products are out of line already
template <class F> GH_HD_NOINLINE typename F::T f_mul_call(const typename F::T& a, const typename F::T& b) { return F::mul(a, b); }
template <class F> GH_HD_NOINLINE typename F::T f_sqr_call(const typename F::T& a) { return F::sqr(a); }
template <class F> GH_HD typename F::T fx_mul(const typename F::T& a, const typename F::T& b) {
    if constexpr (F::DEG == 1) return F::mul(a, b);
    else return f_mul_call<F>(a, b);
}
template <class F> GH_HD typename F::T fx_sqr(const typename F::T& a) {
    if constexpr (F::DEG == 1) return F::sqr(a);
    else return f_sqr_call<F>(a);
}

// a^e for the EBITS-bit exponent e (32-bit words, least significant first, bit EBITS - 1 set)
template <class F, int EBITS> GH_HD typename F::T f_pow_bits(const typename F::T& a, const uint32_t* e) {
    typename F::T r = a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int i = EBITS - 2; i >= 0; i--) {
        r = fx_sqr<F>(r);
        if ((e[i >> 5] >> (i & 31)) & 1u) r = fx_mul<F>(r, a);
    }
    return r;
}

// the root of a (either one) and whether it is one; z0: an element of order 2^S, e: (t - 1) / 2.  See the note at the top.
template <class F, int S, int EBITS>
GH_HD typename F::T f_sqrt_ts(const typename F::T& a, const typename F::T& z0, const uint32_t* e, bool& ok) {
    typedef typename F::T T;
    const T one = F::one();
    const T w = f_pow_bits<F, EBITS>(a, e);
    T x = fx_mul<F>(a, w);
    T b = fx_mul<F>(x, w);
    T z = z0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int i = S - 1; i >= 1; i--) {
        T t = b;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
        for (int j = 0; j < i - 1; j++) t = fx_sqr<F>(t);
        const bool fix = !F::eq(t, one);
        if (fix) x = fx_mul<F>(x, z);
        z = fx_sqr<F>(z);
        if (fix) b = fx_mul<F>(b, z);
    }
    ok = F::eq(fx_sqr<F>(x), a);
    return x;
}

// ---------------------------------------------------------------------------------------------------- the three fields
template <class P> struct SqrtFq;
template <> struct SqrtFq<P4> {
    static constexpr int S = GH_P4_SQRT_S, EBITS = GH_P4_SQRT_EBITS;
    static GH_HD Fp z() { const uint32_t c[NL] = GH_P4_SQRT_Z_I29; return fp_const<P4>(c); }
    static GH_HD Fp half() { const uint32_t c[NL] = GH_P4_HALF_I29; return fp_const<P4>(c); }
};
template <> struct SqrtFq<P6> {
    static constexpr int S = GH_P6_SQRT_S, EBITS = GH_P6_SQRT_EBITS;
    static GH_HD Fp z() { const uint32_t c[NL] = GH_P6_SQRT_Z_I29; return fp_const<P6>(c); }
    static GH_HD Fp half() { const uint32_t c[NL] = GH_P6_HALF_I29; return fp_const<P6>(c); }
};
constexpr int SQRT_E_WORDS_P4 = (GH_P4_SQRT_EBITS + 31) / 32, SQRT_E_WORDS_P6 = (GH_P6_SQRT_EBITS + 31) / 32,
              SQRT_E_WORDS_P6Q3 = (GH_P6Q3_SQRT_EBITS + 31) / 32;

struct FpRoot {
    Fp v;
    bool ok;
};
// Fq: e = the words of GH_P4_SQRT_E32 / GH_P6_SQRT_E32.  Out of line: fq2_sqrt calls it three times.
template <class P> GH_HD_NOINLINE FpRoot fq_sqrt_call(const Fp& a, const uint32_t* e) {
    FpRoot r;
    r.v = f_sqrt_ts<F1<P, false>, SqrtFq<P>::S, SqrtFq<P>::EBITS>(a, SqrtFq<P>::z(), e, r.ok);
    return r;
}

// Fq2 over p4 by the complex method (fp2.rs:186-214; eprint 2012/685 algorithm 8), e = GH_P4_SQRT_E32:
//     c1 == 0: the root of c0 in Fq or none (the quirk at the top)
//     alpha = sqrt(norm a), none if the norm is a non-residue;  delta = (alpha + c0) / 2, or delta - alpha if that is a
//     non-residue;  root = (sqrt(delta), c1 / (2 sqrt(delta)))
// Where the reference asks for Legendre symbols, the root is attempted and its verdict used: at most three Fq roots.
GH_HD Fp2T fq2_sqrt(const Fp2T& a, const uint32_t* e, bool& ok) {
    typedef F1<P4, false> F;
    const bool real = fp_is_zero(a.c1);
    const Fp norm = fp_sub<P4>(F::sqr(a.c0), fp_mul_small<P4, 13>(F::sqr(a.c1)));
    const FpRoot alpha = fq_sqrt_call<P4>(real ? a.c0 : norm, e);
    ok = alpha.ok;
    if (real) return Fp2T{alpha.v, fp_zero()};
    Fp delta = F::mul(fp_add<P4>(alpha.v, a.c0), SqrtFq<P4>::half());
    FpRoot r{fp_zero(), false};
    for (int k = 0; k < 2; k++) {
        if (ok && !r.ok) {
            if (k) delta = fp_sub<P4>(delta, alpha.v);
            r = fq_sqrt_call<P4>(delta, e);
        }
    }
    ok = ok && r.ok;
    const Fp c1 = F::mul(F::mul(a.c1, SqrtFq<P4>::half()), fp_inv<P4>(r.v));
    return Fp2T{r.v, c1};
}

// Fq3 over p6: Tonelli-Shanks in Fq3 as the reference's sqrt_impl!, e = GH_P6Q3_SQRT_E32
GH_HD Fp3T fq3_sqrt(const Fp3T& a, const uint32_t* e, bool& ok) {
    const uint32_t z0[NL] = GH_P6Q3_SQRT_Z0_I29, z1[NL] = GH_P6Q3_SQRT_Z1_I29, z2[NL] = GH_P6Q3_SQRT_Z2_I29;
    const Fp3T z{fp_const<P6>(z0), fp_const<P6>(z1), fp_const<P6>(z2)};
    return f_sqrt_ts<F3<P6, 11, false>, GH_P6Q3_SQRT_S, GH_P6Q3_SQRT_EBITS>(a, z, e, ok);
}

// ---------------------------------------------------------------------------------------------------- per curve
// what validation needs of a curve: the root in its base field (e: that field's exponent words), the digits of its order,
// whether the curve equation decides membership (G1: cofactor 1, the group has order r), and the coefficient b (host side:
// the kernels take it as an argument)
template <class C> struct PointCurve;
#define GH_PT_W(m) ([] { static const uint64_t w[12] = m; return (const uint32_t*)w; }())
template <> struct PointCurve<Mnt4G1> {
    static Fp b() { return fp_from_abi<P4>(GH_PT_W(GH_MNT4753_G1_B0_M_64)); }
    static constexpr int R_DIGITS = GH_MNT4_R_DIGITS, E_WORDS = SQRT_E_WORDS_P4;
    static constexpr bool PRIME_ORDER = true;
    static GH_HD Fp sqrt(const Fp& a, const uint32_t* e, bool& ok) { const FpRoot r = fq_sqrt_call<P4>(a, e); ok = r.ok; return r.v; }
};
template <> struct PointCurve<Mnt6G1> {
    static Fp b() { return fp_from_abi<P6>(GH_PT_W(GH_MNT6753_G1_B0_M_64)); }
    static constexpr int R_DIGITS = GH_MNT6_R_DIGITS, E_WORDS = SQRT_E_WORDS_P6;
    static constexpr bool PRIME_ORDER = true;
    static GH_HD Fp sqrt(const Fp& a, const uint32_t* e, bool& ok) { const FpRoot r = fq_sqrt_call<P6>(a, e); ok = r.ok; return r.v; }
};
template <> struct PointCurve<Mnt4G2> {
    static Fp2T b() { return Fp2T{fp_from_abi<P4>(GH_PT_W(GH_MNT4753_G2_B0_M_64)), fp_from_abi<P4>(GH_PT_W(GH_MNT4753_G2_B1_M_64))}; }
    static constexpr int R_DIGITS = GH_MNT4_R_DIGITS, E_WORDS = SQRT_E_WORDS_P4;
    static constexpr bool PRIME_ORDER = false;
    static GH_HD Fp2T sqrt(const Fp2T& a, const uint32_t* e, bool& ok) { return fq2_sqrt(a, e, ok); }
};
template <> struct PointCurve<Mnt6G2> {
    static Fp3T b() {
        return Fp3T{fp_from_abi<P6>(GH_PT_W(GH_MNT6753_G2_B0_M_64)), fp_from_abi<P6>(GH_PT_W(GH_MNT6753_G2_B1_M_64)),
                    fp_from_abi<P6>(GH_PT_W(GH_MNT6753_G2_B2_M_64))};
    }
    static constexpr int R_DIGITS = GH_MNT6_R_DIGITS, E_WORDS = SQRT_E_WORDS_P6Q3;
    static constexpr bool PRIME_ORDER = false;
    static GH_HD Fp3T sqrt(const Fp3T& a, const uint32_t* e, bool& ok) { return fq3_sqrt(a, e, ok); }
};

template <class C> GH_HD typename C::FC::T curve_rhs(const typename C::FC::T& x, const typename C::FC::T& b) {
    typedef typename C::FC F;
    return F::add(F::add(F::mul(F::sqr(x), x), C::mul_by_a(x)), b);
}
template <class C> GH_HD bool aff_on_curve(const Aff<C>& p, const typename C::FC::T& b) {
    return C::FC::eq(C::FC::sqr(p.y), curve_rhs<C>(p.x, b));
}

// r P == infinity for an affine P on the curve, by the signed digits of r (most significant first, the leading 1 kept):
// R_DIGITS - 1 doublings and one mixed addition of +-P per non-zero digit.  The steps are the complete ones of ec29.h
// (an accumulator at infinity, P = +-Q, y = 0 all have their case), so the value is r P in the group of the whole curve:
// the verdict of the reference's mul_bits(r).is_zero() for every on-curve input (swp.rs:118-121).
template <class C> GH_HD bool r_times_is_zero(const Aff<C>& p, const int8_t* rnaf) {
    const Aff<C> np = aff_neg<C>(p);
    Proj<C> q{p.x, p.y, C::FC::one()};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int d = 1; d < PointCurve<C>::R_DIGITS; d++) {
        q = proj_dbl_call<C>(q);
        const int n = rnaf[d];
        if (n != 0) q = proj_madd_call<C>(q, n > 0 ? p : np);
    }
    return proj_is_zero(q);
}
// GroupAffine::group_membership_test for a point not at infinity
template <class C> GH_HD bool aff_is_member(const Aff<C>& p, const typename C::FC::T& b, const int8_t* rnaf) {
    if (!aff_on_curve<C>(p, b)) return false;
    if constexpr (PointCurve<C>::PRIME_ORDER) return true;
    else return r_times_is_zero<C>(p, rnaf);
}

// ---------------------------------------------------------------------------------------------------- rows
constexpr uint8_t PT_FLAG_INFINITY = 1, PT_FLAG_PARITY = 2;
enum : uint8_t { PT_OK = 0, PT_INVALID_FIELD_ELEMENT = 1, PT_INVALID_FLAGS = 2, PT_NOT_ON_CURVE = 3, PT_NOT_PRIME_ORDER = 4 };

// FromCompressedBits::decompress of one row (swp.rs:227-268).  xw: DEG x 24 LE words, the canonical coefficients of x as
// read_bits sees them before from_repr; flags: bit 0 infinity, bit 1 parity.  The status in the reference's order; on PT_OK
// p and inf hold the point (infinity as GroupAffine::zero() = (0, 1)), otherwise p is zero and inf clear.
template <class C>
GH_HD uint8_t decompress_row(const uint32_t* xw, uint8_t flags, const typename C::FC::T& b, const uint32_t* e, const int8_t* rnaf, Aff<C>& p,
                             bool& inf) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    p = Aff<C>{F::zero(), F::zero()};
    inf = false;
    bool below = true;
    GH_UNROLL for (int c = 0; c < F::DEG; c++) below = below && fp_words_below_p<PF>(xw + 24 * c);
    if (!below) return PT_INVALID_FIELD_ELEMENT;
    typename F::T x = F::zero();
    GH_UNROLL for (int c = 0; c < F::DEG; c++) F::comp(x, c) = fp_from_canon_words<PF>(xw + 24 * c);
    const bool want_inf = (flags & PT_FLAG_INFINITY) != 0, parity = (flags & PT_FLAG_PARITY) != 0;
    if ((flags & ~(PT_FLAG_INFINITY | PT_FLAG_PARITY)) || (want_inf && (parity || !F::is_zero(x)))) return PT_INVALID_FLAGS;
    if (want_inf) {
        p.y = F::one();
        inf = true;
        return PT_OK;
    }
    bool ok;
    typename F::T y = PointCurve<C>::sqrt(curve_rhs<C>(x, b), e, ok);
    if (!ok) return PT_NOT_ON_CURVE;
    if (f_is_odd<F, PF>(y) != parity) y = F::neg(y);
    const Aff<C> q{x, y};
    if constexpr (!PointCurve<C>::PRIME_ORDER)
        if (!r_times_is_zero<C>(q, rnaf)) return PT_NOT_PRIME_ORDER;
    p = q;
    return PT_OK;
}

// ToCompressedBits::compress of one row (swp.rs:205-225): canonical x (zero for the point at infinity) and the two flags
template <class C> GH_HD uint8_t compress_row(const Aff<C>& p, bool inf, uint32_t* xw) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    GH_UNROLL for (int c = 0; c < F::DEG; c++) fp_to_canon_words<PF>(xw + 24 * c, inf ? fp_zero() : F::comp(p.x, c));
    if (inf) return PT_FLAG_INFINITY;
    return f_is_odd<F, PF>(p.y) ? PT_FLAG_PARITY : 0;
}

}  // namespace gh
