// poly_kernels.h -- the per-lane arithmetic of the polynomial unit (include/ginger_hip_poly.h), free of HIP: poly.hip's
// kernels are these functions behind a thread index, and the CPU tests run the same text on the host
// (tests/host_shim/poly_shim.cpp, poly_check.cpp under the host sanitizers).  DESIGN.md section 17.
//
// Forms.  A vector is rows of 24 words in the ABI's Montgomery form (x 2^768), canonical.  Unpacked, such a row is the internal
// form (x 2^754) of 2^14 x, and the internal product of that with a factor in the internal form is 2^14 x f again: sums,
// differences and products by a point, a root of unity or a scale factor are all formed on the unpacked ABI limbs, and no
// conversion product is spent on either side.  Intermediate vectors (the upper levels of a fold or a scan) are rows of Fp,
// the same values left unpacked.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fp29.h"
#include "poly_plan.h"

namespace gh {

GH_HD Fp poly_ld_row(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t w[24];
    const uint4* q = reinterpret_cast<const uint4*>(p);
    GH_UNROLL for (int i = 0; i < 6; i++) { const uint4 v = q[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
    return fp_unpack(w);
#else
    return fp_unpack(p);
#endif
}
GH_HD void poly_st_row(uint32_t* p, const Fp& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t w[24];
    fp_pack(w, a);
    uint4* q = reinterpret_cast<uint4*>(p);
    GH_UNROLL for (int i = 0; i < 6; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
#else
    fp_pack(p, a);
#endif
}
GH_HD bool poly_row_is_zero(const uint32_t* p) {
    uint32_t o = 0;
    GH_UNROLL for (int i = 0; i < 24; i++) o |= p[i];
    return o == 0;
}

// a^e, a in the internal form: the factor of a level (z^G, mu^L)
template <class P> GH_HD Fp poly_pow(const Fp& a, uint64_t e) {
    Fp r = fp_one<P>(), b = a;
    for (; e; e >>= 1) {
        if (e & 1) r = fp_mul<P>(r, b);
        b = fp_sqr<P>(b);
    }
    return r;
}

// ---- fold.  Lane g < G of a level of n coefficients: acc[p] = sum_j c_(g + j G) w[p]^j for KP points at once, the
// coefficients read once.  ABI_IN: rows of `abi`; otherwise rows of `fin`.
// (the points are spelled out, not looped over: hipcc leaves a loop around an inlined product rolled, and acc then lives in scratch)
template <class P, int KP, bool ABI_IN>
GH_HD void poly_fold_lane(uint64_t n, uint64_t G, uint64_t g, const uint32_t* abi, const Fp* fin, const Fp* w, Fp* acc) {
    static_assert(KP >= 1 && KP <= 4, "one to four points per lane");
    uint64_t j = poly_fold_count(PolyFoldLevel{n, G}, g);
    if (!j) {
        GH_UNROLL for (int p = 0; p < KP; p++) acc[p] = fp_zero();
        return;
    }
    j--;
    const Fp top = ABI_IN ? poly_ld_row(abi + (g + j * G) * 24) : fin[g + j * G];
    GH_UNROLL for (int p = 0; p < KP; p++) acc[p] = top;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    while (j-- > 0) {
        const Fp c = ABI_IN ? poly_ld_row(abi + (g + j * G) * 24) : fin[g + j * G];
        acc[0] = fp_add<P>(fp_mul<P>(acc[0], w[0]), c);
        if (KP > 1) acc[KP > 1 ? 1 : 0] = fp_add<P>(fp_mul<P>(acc[KP > 1 ? 1 : 0], w[KP > 1 ? 1 : 0]), c);
        if (KP > 2) acc[KP > 2 ? 2 : 0] = fp_add<P>(fp_mul<P>(acc[KP > 2 ? 2 : 0], w[KP > 2 ? 2 : 0]), c);
        if (KP > 3) acc[KP > 3 ? 3 : 0] = fp_add<P>(fp_mul<P>(acc[KP > 3 ? 3 : 0], w[KP > 3 ? 3 : 0]), c);
    }
}

// ---- scan (poly_plan.h).  MUL = false: mu is one and no product is formed (the strided suffix sum).
// pass 1: the outgoing value of lane t's segment, carry-in zero
template <class P, bool ABI_IN, bool MUL>
GH_HD Fp poly_scan_seg_lane(const PolyScanLevel& lv, uint64_t t, const uint32_t* abi, const Fp* fin, const Fp& mu) {
    const uint64_t r = t % lv.N, s = t / lv.N;
    uint64_t k0, k1;
    lv.span(r, s, k0, k1);
    Fp acc = fp_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint64_t k = k1; k-- > k0;) {
        const uint64_t i = r + k * lv.N;
        const Fp x = ABI_IN ? poly_ld_row(abi + i * 24) : fin[i];
        acc = (MUL && k + 1 != k1) ? fp_add<P>(fp_mul<P>(acc, mu), x) : fp_add<P>(acc, x);
    }
    return acc;
}
// pass 2 (or the whole of a final level): T_i for the elements of lane t's segment, from the carry at element (s + 1) N + r
// of `carry` (the scanned vector of the next level; null on a final level).  ABI: x from `abi`, T_i to row i of lo where
// i < split and to row i - split of hi otherwise; else x from `fio` and T_i over it.
template <class P, bool ABI, bool MUL>
GH_HD void poly_scan_write_lane(const PolyScanLevel& lv, uint64_t t, const uint32_t* abi, Fp* fio, const Fp& mu, const Fp* carry, uint64_t split,
                                uint32_t* lo, uint32_t* hi) {
    const uint64_t r = t % lv.N, s = t / lv.N;
    uint64_t k0, k1;
    lv.span(r, s, k0, k1);
    Fp acc = (carry && s + 1 < lv.S) ? carry[(s + 1) * lv.N + r] : fp_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint64_t k = k1; k-- > k0;) {
        const uint64_t i = r + k * lv.N;
        const Fp x = ABI ? poly_ld_row(abi + i * 24) : fio[i];
        acc = MUL ? fp_add<P>(fp_mul<P>(acc, mu), x) : fp_add<P>(acc, x);
        if (ABI) poly_st_row(i < split ? lo + i * 24 : hi + (i - split) * 24, acc);
        else fio[i] = acc;
    }
}

// ---- elementwise.  Row i < max(na, nb) of a op b, the shorter operand read as zeros: op 0 a + b, 1 a - b, 2 a + f b
// (f in the internal form), 3 -a
enum { POLY_ADD = 0, POLY_SUB = 1, POLY_ADD_SCALED = 2, POLY_NEG = 3 };
template <class P>
GH_HD void poly_axpy_lane(int op, uint64_t i, const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb, const Fp& f, uint32_t* out) {
    const Fp x = i < na ? poly_ld_row(a + i * 24) : fp_zero();
    Fp y = (op != POLY_NEG && i < nb) ? poly_ld_row(b + i * 24) : fp_zero();
    if (op == POLY_ADD_SCALED) y = fp_mul<P>(y, f);
    poly_st_row(out + i * 24, op == POLY_NEG ? fp_neg<P>(x) : (op == POLY_SUB ? fp_sub<P>(x, y) : fp_add<P>(x, y)));
}

// row i < n + N of p (x^N - 1) (dense.rs:134-139): in[i - N] - in[i], what lies outside the n rows read as zero
template <class P> GH_HD void poly_mul_vanishing_lane(uint64_t i, const uint32_t* in, uint64_t n, uint64_t N, uint32_t* out) {
    const Fp lo = (i >= N && i - N < n) ? poly_ld_row(in + (i - N) * 24) : fp_zero();
    const Fp hi = i < n ? poly_ld_row(in + i * 24) : fp_zero();
    poly_st_row(out + i * 24, fp_sub<P>(lo, hi));
}

// row i of the domain's elements (domain.rs:234-240): tw[i] = g^i in the internal form; null: the domain of size one
template <class P> GH_HD void poly_elements_lane(uint64_t i, const Fp* tw, uint32_t* out) {
    fp_to_abi<P>(out + i * 24, tw ? tw[i] : fp_one<P>());
}

// row i < 2^log_n of a sparse polynomial over the domain (polynomial/mod.rs:147-154): sum_j c_j g^((i e_j) mod N).  exps: e_j
// already reduced mod N; coeffs: t unpacked ABI rows
template <class P>
GH_HD void poly_sparse_lane(uint64_t i, uint32_t log_n, const Fp* tw, const uint64_t* exps, const Fp* coeffs, uint64_t t, uint32_t* out) {
    const uint64_t mask = ((uint64_t)1 << log_n) - 1;
    Fp acc = fp_zero();
    for (uint64_t j = 0; j < t; j++) {
        const uint64_t e = (i * exps[j]) & mask;             // below 2^60: both factors are below 2^30
        acc = fp_add<P>(acc, (tw && e) ? fp_mul<P>(coeffs[j], tw[e]) : coeffs[j]);
    }
    poly_st_row(out + i * 24, acc);
}

// ---- reductions.  The rows i0, i0 + step, ... < n: index of the last non-zero one plus one (or 0), or the number of zero rows
GH_HD uint64_t poly_last_nonzero(const uint32_t* rows, uint64_t n, uint64_t i0, uint64_t step) {
    uint64_t best = 0;
    for (uint64_t i = i0; i < n; i += step)
        if (!poly_row_is_zero(rows + i * 24)) best = i + 1;
    return best;
}
GH_HD uint64_t poly_count_zero(const uint32_t* rows, uint64_t n, uint64_t i0, uint64_t step) {
    uint64_t c = 0;
    for (uint64_t i = i0; i < n; i += step) c += poly_row_is_zero(rows + i * 24) ? 1 : 0;
    return c;
}

}  // namespace gh
