// msm_fold.h -- the host-side point work of the MSM: the fold of the device's window sums into the result, and the few
// single-point operations of the C ABI.  Host code on ec29.h and host_math.h only (no HIP): tests/test_msm_host.py runs the
// folds against their definition with g++ alone (tests/host_shim/msm_host_shim.cpp).
#pragma once
#include <string.h>
#include <vector>
#include "../../include/ginger_hip.h"
#include "ec29.h"
#include "host_math.h"

namespace gh_rt {
using namespace gh;

template <class C> void proj_to_abi_host(uint64_t* out, const Proj<C>& p) {
    typedef typename C::F F;
    uint32_t* w = reinterpret_cast<uint32_t*>(out);
    F::to_abi(w, p.x);
    F::to_abi(w + 24 * F::DEG, p.y);
    F::to_abi(w + 48 * F::DEG, p.z);
}
template <class C> Proj<C> proj_from_abi_host(const uint64_t* in) {
    typedef typename C::F F;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(in);
    Proj<C> p;
    p.x = F::from_abi(w);
    p.y = F::from_abi(w + 24 * F::DEG);
    p.z = F::from_abi(w + 48 * F::DEG);
    return p;
}

// Horner over windows, high to low (variable_base.rs:73-82).  Per window the device delivers
// (T, PW, PS, PA, PB) with  R_w = PW 2^(u+sw) + PS 2^u + PA 2^sw + PB  and T = plain sum of the
// window's buckets; the terms of acc * 2^c + R_w are folded by descending exponent so that the
// powers of two cost no doubling beyond the c per window that the Horner step needs anyway:
//   acc*2^c + R_w = (((acc*2^(c-u-6) + PW)*2^6 + PS)*2^(u-6) + PA)*2^6 + PB        (sw = 6, c >= u + 6)
// with U = 2^u = tpw L1 (msm_plan.h fold_u) and
//   PW, PS = (A, Bv) of the weighted level-2 program over the runW's, PA = sum A, PB = sum Bv.
// top_unsigned: window W-1 is "region b" of window W-2 (slot offset 2^(c-1)):
//   R_top = R_(W-2) + R_(W-1) + 2^(c-1) T_(W-1),  weight 2^(c (W-2)).
// Layout of hw (9 RW points, RW = W here): point (which * RW + w) * 3 + k with which = 0: (T, PW, PS), 1: PA at k = 0, 2: PB at k = 0.
// HC is the curve policy the fold runs on: the 64-bit-limb host field (host_math.h HostCurveOf).
template <class HC> struct FoldTerm { int ex; const Proj<HC>* pt; };

template <class HC>
Proj<HC> fold_terms(FoldTerm<HC>* t, int nt) {   // sum pt * 2^ex
    for (int a = 1; a < nt; a++) for (int b = a; b > 0 && t[b].ex > t[b - 1].ex; b--) { FoldTerm<HC> x = t[b]; t[b] = t[b - 1]; t[b - 1] = x; }
    Proj<HC> val = *t[0].pt;
    int cur = t[0].ex;
    for (int k = 1; k < nt; k++) {
        for (int d = 0; d < cur - t[k].ex; d++) val = proj_dbl<HC>(val);
        cur = t[k].ex;
        val = proj_add<HC>(val, *t[k].pt);
    }
    for (int d = 0; d < cur; d++) val = proj_dbl<HC>(val);
    return val;
}

template <class HC>
Proj<HC> fold_generic(const std::vector<Proj<HC>>& hw, int W, int c, int u, int sw, int top_unsigned) {
    auto PT = [&](int which, int w, int k) { return &hw[(size_t)(which * W + w) * 3 + k]; };
    auto window_terms = [&](int w, FoldTerm<HC>* t) {
        t[0] = FoldTerm<HC>{u + sw, PT(0, w, 1)};  // PW   (sw = log2 of the items per wave: 6, or 5 / 4 for G2)
        t[1] = FoldTerm<HC>{u, PT(0, w, 2)};       // PS
        t[2] = FoldTerm<HC>{sw, PT(1, w, 0)};      // PA
        t[3] = FoldTerm<HC>{0, PT(2, w, 0)};       // PB
    };
    Proj<HC> acc = proj_zero<HC>();
    int w = W - 1;
    if (top_unsigned) {
        FoldTerm<HC> t[9];
        window_terms(W - 2, t);
        window_terms(W - 1, t + 4);
        t[8] = FoldTerm<HC>{c - 1, PT(0, W - 1, 0)};   // 2^(c-1) * T_(W-1)
        acc = fold_terms<HC>(t, 9);
        w = W - 3;
    }
    for (; w >= 0; w--) {
        FoldTerm<HC> t[5];
        window_terms(w, t);
        t[4] = FoldTerm<HC>{c, &acc};
        Proj<HC> val = fold_terms<HC>(t, 5);
        acc = val;
    }
    if (proj_is_zero<HC>(acc)) acc = proj_zero<HC>();   // canonical (0, 1, 0) like the reference's zero()
    return acc;
}

// Merged windows (precomputed shift table): ONE bucket set of nb = 2^(c-1) slots (slot s = digit magnitude s + 1), cut
// into Wp pseudo-windows of Q = 2^q slots for the two-level wave reduction; slot s = w' Q + k, so
//   sum_s s B_s = sum_w' R_w' + Q sum_w' w' T_w'
// with R_w' as above and T_w' the plain sum of pseudo-window w'.
// With a PARTIAL table the buckets form `sets` such sets (set g: the windows w = j sets + g, weight 2^(c g) on top of the
// rows' own 2^(c sets j)): every set is folded as above over its Wp / sets pseudo-windows, then Horner over the sets.
template <class HC>
Proj<HC> fold_merged_generic(const std::vector<Proj<HC>>& hw, int Wp_all, int q, int u, int sw, int sets, int c) {
    Proj<HC> total_acc = proj_zero<HC>();
    const int Wp = Wp_all / sets;
    for (int gset = sets - 1; gset >= 0; gset--) {
        const int w0 = gset * Wp;
        auto PT = [&](int which, int w, int k) -> const Proj<HC>& { return hw[(size_t)(which * Wp_all + w0 + w) * 3 + k]; };
        Proj<HC> spw = proj_zero<HC>(), sps = proj_zero<HC>(), spa = proj_zero<HC>(), spb = proj_zero<HC>();
        Proj<HC> run = proj_zero<HC>(), st = proj_zero<HC>();
        for (int w = Wp - 1; w >= 0; w--) {
            spw = proj_add<HC>(spw, PT(0, w, 1));
            sps = proj_add<HC>(sps, PT(0, w, 2));
            spa = proj_add<HC>(spa, PT(1, w, 0));
            spb = proj_add<HC>(spb, PT(2, w, 0));
            if (w >= 1) { run = proj_add<HC>(run, PT(0, w, 0)); st = proj_add<HC>(st, run); }   // sum_w' w' T_w'
        }
        // slot s carries digit magnitude s + 1: sum (s + 1) B_s = sum s B_s + sum_w' T_w'   (run holds T_1 + .. + T_(Wp-1) here)
        spb = proj_add<HC>(spb, proj_add<HC>(run, PT(0, 0, 0)));
        FoldTerm<HC> t[6] = {{u + sw, &spw}, {u, &sps}, {sw, &spa}, {0, &spb}, {q, &st}, {c, &total_acc}};   // (sets above this one) * 2^c + this set
        Proj<HC> acc = fold_terms<HC>(t, gset == sets - 1 ? 5 : 6);
        total_acc = acc;
    }
    if (proj_is_zero<HC>(total_acc)) total_acc = proj_zero<HC>();
    return total_acc;
}

// The lean form of the reduction (msm_impl.h launch_reduce) delivers, per window, (T_w, A2, Bv2) for the lanes' run and
// PA' = sum of the lanes' wacc:
//   R_w = 64 PA' + 64 L1 A2 + Bv2   ->   the fold's slots PW = 0, PS = A2 (weight 2^u = 64 L1), PA = PA', PB = Bv2
template <class HC>
void lean_reslot(std::vector<Proj<HC>>& hw, int RW) {
    for (int w = 0; w < RW; w++) {
        const Proj<HC> a2 = hw[(size_t)w * 3 + 1], bv2 = hw[(size_t)w * 3 + 2];
        hw[(size_t)w * 3 + 1] = proj_zero<HC>();
        hw[(size_t)w * 3 + 2] = a2;
        hw[(size_t)(2 * RW + w) * 3] = bv2;       // T_w and PA' are where the fold reads them
    }
}

// the window sums as the device wrote them (internal form) -> the host curve's representation == ABI Montgomery limbs
template <class C>
std::vector<Proj<typename HostCurveOf<C>::type>> to_host_curve(const Proj<C>* hw, size_t count) {
    static_assert(HostCurveOf<C>::fast, "host curve on ABI limbs");
    std::vector<Proj<typename HostCurveOf<C>::type>> h64(count);
    for (size_t i = 0; i < count; i++) proj_to_abi_host<C>(reinterpret_cast<uint64_t*>(&h64[i]), hw[i]);
    return h64;
}
template <class C>
void fold_windows(const std::vector<Proj<typename HostCurveOf<C>::type>>& h64, int W, int c, int u, int sw, int top_unsigned, uint64_t* out_xyz) {
    const auto acc = fold_generic<typename HostCurveOf<C>::type>(h64, W, c, u, sw, top_unsigned);
    memcpy(out_xyz, &acc, sizeof(acc));
}
template <class C>
void fold_merged(const std::vector<Proj<typename HostCurveOf<C>::type>>& h64, int Wp, int q, int u, int sw, int sets, int c, uint64_t* out_xyz) {
    const auto acc = fold_merged_generic<typename HostCurveOf<C>::type>(h64, Wp, q, u, sw, sets, c);
    memcpy(out_xyz, &acc, sizeof(acc));
}

// ---- single points of the C ABI (gh_proj_add, gh_proj_mul, gh_proj_neg, gh_proj_to_affine)
template <class C> int proj_add_host(uint64_t* acc_xyz, const uint64_t* p_xyz) {
    Proj<C> a = proj_from_abi_host<C>(acc_xyz), b = proj_from_abi_host<C>(p_xyz);
    proj_to_abi_host<C>(acc_xyz, proj_add<C>(a, b));
    return GH_OK;
}

// out = k * p for one point (the prover's r * delta_g1, s * g_a, ... of prover.rs:278-330): double-and-add
// from the top bit like GroupProjective::mul_assign (short_weierstrass_projective.rs:521-540), on the
// 64-bit-limb host field.  Host side; ~1 ms.
template <class C> int proj_mul_host(const uint64_t* p_xyz, const uint64_t* scalar12, uint64_t* out_xyz) {
    typedef typename HostCurveOf<C>::type HC;
    static_assert(HostCurveOf<C>::fast, "host curve on ABI limbs");
    Proj<HC> p, res = proj_zero<HC>();
    memcpy(&p, p_xyz, sizeof(p));
    bool found_one = false;
    for (int bit = 767; bit >= 0; bit--) {
        const bool b = (scalar12[bit >> 6] >> (bit & 63)) & 1u;
        if (found_one) res = proj_dbl<HC>(res);
        if (b) { res = proj_add<HC>(res, p); found_one = true; }
    }
    if (proj_is_zero<HC>(res)) res = proj_zero<HC>();
    memcpy(out_xyz, &res, sizeof(res));
    return GH_OK;
}

template <class C> int proj_neg_host(uint64_t* xyz) {   // (X, Y, Z) -> (X, -Y, Z)   (swp.rs Neg)
    typedef typename HostCurveOf<C>::type HC;
    Proj<HC> p;
    memcpy(&p, xyz, sizeof(p));
    if (!proj_is_zero<HC>(p)) p.y = HC::F::neg(p.y);
    memcpy(xyz, &p, sizeof(p));
    return GH_OK;
}

template <class C> int to_affine_host(const uint64_t* xyz, uint64_t* out_xy, uint8_t* is_infinity) {
    typedef typename C::F F;
    Proj<C> p = proj_from_abi_host<C>(xyz);
    uint32_t* w = reinterpret_cast<uint32_t*>(out_xy);
    if (proj_is_zero<C>(p)) {  // GroupAffine::zero() = (0, 1, infinity)  (swp.rs:130-132)
        *is_infinity = 1;
        F::to_abi(w, F::zero());
        F::to_abi(w + 24 * F::DEG, F::one());
        return GH_OK;
    }
    *is_infinity = 0;
    typename F::T zi = host_inv<F>(p.z);
    F::to_abi(w, F::mul(p.x, zi));
    F::to_abi(w + 24 * F::DEG, F::mul(p.y, zi));
    return GH_OK;
}

}  // namespace gh_rt
