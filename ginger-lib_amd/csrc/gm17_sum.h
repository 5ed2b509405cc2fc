// gm17_sum.h -- the complete affine group addition of the GM17 verifier: S1 = A + g_alpha in G1 and S2 = B + h_beta in G2
// (proof-systems/src/gm17/verifier.rs:40-45).  Plain GH_HD code over the fields of fp29.h and the towers of pairing29.h and
// pairing29_mnt6.h: the same text runs in gm17_sums_kernel (gm17_verify_impl.h) and, compiled by g++, in
// tests/host_shim/gm17_shim.cpp.  DESIGN.md section 14b.
//
// One sum is one chord-or-tangent step with ONE inversion of the denominator (safegcd in Fq, after the norm to Fq for a tower
// element), chosen over a projective sum plus a batched normalisation because the result feeds pair_setup_kernel in affine
// ABI form at once and because every case is then decided by three zero tests on the inputs:
//     P1 at infinity -> P2;  P2 at infinity -> P1;
//     x1 != x2       -> lambda = (y2 - y1) / (x2 - x1)
//     x1 == x2, y1 == y2, y1 != 0 -> lambda = (3 x1^2 + a) / (2 y1)         (a doubling: A = g_alpha, B = h_beta)
//     x1 == x2 otherwise           -> infinity                             (opposite points; a point of order two doubled)
//     x3 = lambda^2 - x1 - x2,  y3 = lambda (x1 - x3) - y1.
// The numerator and the denominator are selected first and the one inversion runs for every row (the inverse of zero is
// zero), so no loop depends on the data and the lanes of a wave diverge nowhere.
// Products, squarings counted as products, in units of the point's field: 1 S (x1^2, computed for every row) + 1 M + 1 S + 1 M
// = 4 and the inversion.  G1: 4 + ~42 (fp_inv: ~40 and two products) = 46 Fq products.  G2 on MNT4-753: 4 Fq2 operations
// = 10 Fq products, Mnt4Pairing::inv = 2 + 42 + 2: 56.  G2 on MNT6-753: 4 Fq3 operations = 22, Mnt6Pairing::inv = 9 + 42 + 3: 76.
#pragma once
#include "pairing29_mnt6.h"

namespace gh {

// what the sum needs of a group: F the field policy of a coordinate, a the curve's coefficient, inv the inverse
template <class E> struct Gm17G1 {
    typedef typename E::G1::FC F;
    static GH_HD Fp a() { return E::G1::mul_by_a(F::one()); }
    static GH_HD Fp inv(const Fp& v) { return fp_inv<typename E::PF>(v); }
};
template <class E> struct Gm17G2 {
    typedef typename E::B F;
    static GH_HD typename F::T a() { return E::G2::mul_by_a(F::one()); }
    static GH_HD typename F::T inv(const typename F::T& v) { return E::inv(v); }
};

template <class T> struct Gm17Point {
    T x, y;
    bool inf;
};

// P1 + P2, complete (the cases above).  The coordinates of a point at infinity are not read for the result; a result at
// infinity carries zero coordinates.
template <class G> GH_HD Gm17Point<typename G::F::T> gm17_add(const Gm17Point<typename G::F::T>& p1, const Gm17Point<typename G::F::T>& p2) {
    typedef typename G::F F;
    typedef typename F::T T;
    const T dx = F::sub(p2.x, p1.x), dy = F::sub(p2.y, p1.y);
    const bool same_x = F::is_zero(dx);
    const bool dbl = same_x && F::is_zero(dy) && !F::is_zero(p1.y);
    const T xx = F::sqr(p1.x);
    const T num = dbl ? F::add(F::add(F::dbl(xx), xx), G::a()) : dy;
    const T den = dbl ? F::dbl(p1.y) : dx;
    const T lambda = F::mul(num, G::inv(den));
    const T x3 = F::sub(F::sub(F::sqr(lambda), p1.x), p2.x);
    const T y3 = F::sub(F::mul(lambda, F::sub(p1.x, x3)), p1.y);
    if (p1.inf) return Gm17Point<T>{p2.inf ? F::zero() : p2.x, p2.inf ? F::zero() : p2.y, p2.inf};
    if (p2.inf) return p1;
    if (same_x && !dbl) return Gm17Point<T>{F::zero(), F::zero(), true};
    return Gm17Point<T>{x3, y3, false};
}

template <class G> GH_HD Gm17Point<typename G::F::T> gm17_neg(const Gm17Point<typename G::F::T>& p) {
    return Gm17Point<typename G::F::T>{p.x, G::F::neg(p.y), p.inf};
}

}  // namespace gh
