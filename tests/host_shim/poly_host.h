// poly_host.h -- the host executor of the polynomial unit: the launch sequences of ginger-lib_amd/csrc/poly.hip with a loop over
// the lanes in place of a kernel launch, over the same level arithmetic (poly_plan.h) and the same lane bodies
// (poly_kernels.h).  poly_shim.cpp puts it behind a C interface for the CPU tests, poly_check.cpp runs it under the host
// sanitizers.  Vectors are rows of 24 words in the ABI's form.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../ginger-lib_amd/csrc/poly_kernels.h"

namespace poly_host {
using namespace gh;

constexpr int FOLD_GROUP = 4, RBLOCK = 256, RITEMS = 8;      // as poly.hip

template <class P> Fp from_abi(const uint32_t* w) { return fp_from_abi<P>(w); }

// evaluate: k points (rows of pts) -> k rows of out.  Level 0 shares the coefficients among groups of FOLD_GROUP points where
// k >= 2, a partial group repeating its last point, as the kernel does.
template <class P> void evaluate(const uint32_t* c, uint64_t n, const uint32_t* pts, uint64_t k, const PolyTuning& t, uint32_t* out) {
    PolyFoldLevel lv[POLY_MAX_LEVELS];
    const int nl = poly_fold_levels(n, t, lv);
    if (!nl) {
        memset(out, 0, k * 96);
        return;
    }
    std::vector<Fp> w((size_t)nl * k);
    for (uint64_t p = 0; p < k; p++)
        for (int l = 0; l < nl; l++) w[(size_t)l * k + p] = poly_pow<P>(from_abi<P>(pts + 24 * p), lv[l].G);
    std::vector<Fp> in, cur;
    for (int l = 0; l < nl; l++) {
        const uint64_t G = lv[l].G;
        cur.assign((size_t)G * k, fp_zero());
        if (l == 0 && k >= 2) {
            for (uint64_t p0 = 0; p0 < k; p0 += FOLD_GROUP) {
                Fp ws[FOLD_GROUP], acc[FOLD_GROUP];
                for (int p = 0; p < FOLD_GROUP; p++) ws[p] = w[p0 + p < k ? p0 + p : k - 1];
                for (uint64_t g = 0; g < G; g++) {
                    poly_fold_lane<P, FOLD_GROUP, true>(lv[l].n, G, g, c, nullptr, ws, acc);
                    for (int p = 0; p < FOLD_GROUP && p0 + p < k; p++) cur[(p0 + p) * G + g] = acc[p];
                }
            }
        } else {
            for (uint64_t p = 0; p < k; p++)
                for (uint64_t g = 0; g < G; g++) {
                    Fp acc;
                    if (l == 0) poly_fold_lane<P, 1, true>(lv[l].n, G, g, c, nullptr, &w[(size_t)l * k + p], &acc);
                    else poly_fold_lane<P, 1, false>(lv[l].n, G, g, nullptr, in.data() + p * lv[l].n, &w[(size_t)l * k + p], &acc);
                    cur[p * G + g] = acc;
                }
        }
        in.swap(cur);
    }
    for (uint64_t p = 0; p < k; p++) poly_st_row(out + 24 * p, in[p]);
}

// T_i = x_i + mu T_(i + N) over the m rows of x: T_i to row i of lo where i < split, to row i - split of hi otherwise
template <class P, bool MUL>
void scan(const uint32_t* x, uint64_t m, uint64_t N, uint32_t L, uint32_t limit, const Fp& mu0, uint64_t split, uint32_t* lo, uint32_t* hi) {
    PolyScanLevel lv[POLY_MAX_LEVELS];
    const int nl = poly_scan_levels(m, N, L, limit, lv);
    if (!nl) return;
    std::vector<std::vector<Fp>> vec((size_t)nl);
    std::vector<Fp> mu((size_t)nl, mu0);
    for (int l = 1; l < nl; l++) {
        vec[l].assign((size_t)lv[l].m, fp_zero());
        if (MUL) mu[l] = poly_pow<P>(mu[l - 1], lv[l - 1].L);
    }
    for (int l = 0; l + 1 < nl; l++)
        for (uint64_t t = 0; t < lv[l].lanes(); t++)
            vec[l + 1][t] = l == 0 ? poly_scan_seg_lane<P, true, MUL>(lv[l], t, x, nullptr, mu[l]) : poly_scan_seg_lane<P, false, MUL>(lv[l], t, nullptr, vec[l].data(), mu[l]);
    for (int l = nl - 1; l >= 0; l--) {
        const Fp* carry = l == nl - 1 ? nullptr : vec[l + 1].data();
        for (uint64_t t = 0; t < lv[l].lanes(); t++) {
            if (l == 0) poly_scan_write_lane<P, true, MUL>(lv[l], t, x, nullptr, mu[l], carry, split, lo, hi);
            else poly_scan_write_lane<P, false, MUL>(lv[l], t, nullptr, vec[l].data(), mu[l], carry, 0, nullptr, nullptr);
        }
    }
}

// q: max(n, 1) - 1 rows, rem: one row
template <class P> void divide_linear(const uint32_t* c, uint64_t n, const uint32_t* z, const PolyTuning& t, uint32_t* q, uint32_t* rem) {
    if (!n) {
        memset(rem, 0, 96);
        return;
    }
    scan<P, true>(c, n, 1, t.run_len, t.direct_max, from_abi<P>(z), 1, rem, q);
}
// q: max(n, N) - N rows, r: N rows
template <class P> void divide_vanishing(const uint32_t* c, uint64_t n, uint32_t log_n, const PolyTuning& t, uint32_t* q, uint32_t* r) {
    const uint64_t N = (uint64_t)1 << log_n;
    if (n < N) memset(r + n * 24, 0, (N - n) * 96);
    scan<P, false>(c, n, N, t.seg_max, t.seg_max, fp_zero(), N, r, q);
}

template <class P> void axpy(int op, const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb, const uint32_t* f, uint32_t* out) {
    const Fp fi = f ? from_abi<P>(f) : fp_zero();
    for (uint64_t i = 0; i < (na > nb ? na : nb); i++) poly_axpy_lane<P>(op, i, a, na, b, nb, fi, out);
}
template <class P> void mul_vanishing(const uint32_t* c, uint64_t n, uint32_t log_n, uint32_t* out) {
    const uint64_t N = (uint64_t)1 << log_n;
    for (uint64_t i = 0; i < n + N; i++) poly_mul_vanishing_lane<P>(i, c, n, N, out);
}
// the reduction as the kernel cuts it: blocks of RBLOCK lanes over RBLOCK * RITEMS rows, the per-block results finished here
inline uint64_t reduce(const uint32_t* rows, uint64_t n, bool count) {
    uint64_t res = 0;
    for (uint64_t first = 0; first < n; first += RBLOCK * RITEMS) {
        const uint64_t end = first + RBLOCK * RITEMS < n ? first + RBLOCK * RITEMS : n;
        for (uint64_t lane = 0; lane < RBLOCK; lane++) {
            const uint64_t v = count ? poly_count_zero(rows, end, first + lane, RBLOCK) : poly_last_nonzero(rows, end, first + lane, RBLOCK);
            res = count ? res + v : (v > res ? v : res);
        }
    }
    return res;
}
// tw[i] = g^i in the internal form, g: a row in the ABI's form
template <class P> std::vector<Fp> power_table(const uint32_t* g, uint32_t log_n) {
    std::vector<Fp> tw((size_t)1 << log_n);
    const Fp gi = from_abi<P>(g);
    tw[0] = fp_one<P>();
    for (size_t i = 1; i < tw.size(); i++) tw[i] = fp_mul<P>(tw[i - 1], gi);
    return tw;
}
template <class P> void elements(const uint32_t* g, uint32_t log_n, uint32_t* out) {
    const std::vector<Fp> tw = power_table<P>(g, log_n);
    for (uint64_t i = 0; i < tw.size(); i++) poly_elements_lane<P>(i, log_n ? tw.data() : nullptr, out);
}
template <class P> void sparse(const uint32_t* g, const uint64_t* exps, const uint32_t* coeffs, uint64_t t, uint32_t log_n, uint32_t* out) {
    const std::vector<Fp> tw = power_table<P>(g, log_n);
    std::vector<uint64_t> e(t);
    std::vector<Fp> c(t);
    for (uint64_t j = 0; j < t; j++) {
        e[j] = exps[j] & (tw.size() - 1);
        c[j] = fp_unpack(coeffs + 24 * j);
    }
    for (uint64_t i = 0; i < tw.size(); i++) poly_sparse_lane<P>(i, log_n, log_n ? tw.data() : nullptr, e.data(), c.data(), t, out);
}

// ---- the plans: 0 where every level ends, no lane gets more than its bound and every index is read exactly once
inline int fold_cover(uint64_t n, const PolyTuning& t) {
    PolyFoldLevel lv[POLY_MAX_LEVELS];
    const int nl = poly_fold_levels(n, t, lv);
    if ((n == 0) != (nl == 0)) return 1;
    const uint64_t direct = t.direct_max > t.run_len ? t.direct_max : t.run_len;
    uint64_t expect = n;
    for (int l = 0; l < nl; l++) {
        if (lv[l].n != expect || !lv[l].G) return 2;
        const bool last = l == nl - 1;
        if (last != (lv[l].G == 1 && lv[l].n <= direct)) return 3;
        std::vector<uint8_t> seen((size_t)lv[l].n, 0);
        for (uint64_t g = 0; g < lv[l].G; g++) {
            const uint64_t cnt = poly_fold_count(lv[l], g);
            if (cnt > (last ? direct : t.run_len) || !cnt) return 4;
            for (uint64_t j = 0; j < cnt; j++) {
                const uint64_t i = g + j * lv[l].G;
                if (i >= lv[l].n || seen[i]++) return 5;
            }
        }
        for (uint8_t s : seen)
            if (s != 1) return 6;
        expect = lv[l].G;
    }
    return 0;
}
inline int scan_cover(uint64_t m, uint64_t N, uint32_t L, uint32_t limit) {
    PolyScanLevel lv[POLY_MAX_LEVELS];
    const int nl = poly_scan_levels(m, N, L, limit, lv);
    if ((m == 0) != (nl == 0)) return 1;
    if (limit < L) limit = L;
    uint64_t expect = m;
    for (int l = 0; l < nl; l++) {
        const bool last = l == nl - 1;
        if (lv[l].m != expect || lv[l].N != N || last != (lv[l].S == 1)) return 2;
        std::vector<uint8_t> seen((size_t)lv[l].m, 0);
        for (uint64_t t = 0; t < lv[l].lanes(); t++) {
            uint64_t k0, k1;
            lv[l].span(t % N, t / N, k0, k1);
            if (k1 - k0 > (last ? limit : L)) return 4;
            for (uint64_t k = k0; k < k1; k++) {
                const uint64_t i = t % N + k * N;
                if (i >= lv[l].m || seen[i]++) return 5;
            }
        }
        for (uint8_t s : seen)
            if (s != 1) return 6;
        expect = lv[l].S * N;
    }
    return 0;
}

}  // namespace poly_host
