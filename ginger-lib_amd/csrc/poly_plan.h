// poly_plan.h -- the level arithmetic of the polynomial unit (include/ginger_hip_poly.h), free of HIP: how a Horner fold and a
// strided suffix scan over n elements are cut into levels no lane of which works on more than its run length.  poly.hip
// launches what these functions return, the CPU tests walk the same levels (tests/host_shim/poly_shim.cpp).  DESIGN.md section 17.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GH_PLAN_HD __host__ __device__ inline
#else
#define GH_PLAN_HD inline
#endif

namespace gh {

constexpr uint32_t POLY_RUN_LEN = 32;        // elements a lane folds or scans with products
constexpr uint32_t POLY_DIRECT_MAX = 32;     // a vector this short is finished by one lane
constexpr uint32_t POLY_SEG_MAX = 64;        // additions a lane of the strided suffix sum makes
constexpr int POLY_MAX_LEVELS = 64;          // run lengths are at least 2: a level at least halves its vector

struct PolyTuning {
    uint32_t run_len = POLY_RUN_LEN, direct_max = POLY_DIRECT_MAX, seg_max = POLY_SEG_MAX;
};
// zero: the default.  A run of one element would never shorten a vector.
inline bool poly_tuning_ok(uint32_t run_len, uint32_t seg_max) { return run_len != 1 && seg_max != 1; }

GH_PLAN_HD uint64_t poly_ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// ---- fold (evaluate): level of n coefficients, G lanes; lane g < G folds the coefficients g + j G < n, j descending, in
// w = z^G.  The last level has G = 1: one lane, plain Horner in z.
struct PolyFoldLevel {
    uint64_t n, G;
};
GH_PLAN_HD uint64_t poly_fold_count(const PolyFoldLevel& l, uint64_t g) { return g < l.n ? poly_ceil_div(l.n - g, l.G) : 0; }
// -> number of levels (0 for n = 0; at most POLY_MAX_LEVELS)
inline int poly_fold_levels(uint64_t n, const PolyTuning& t, PolyFoldLevel* out) {
    int c = 0;
    const uint64_t direct = t.direct_max > t.run_len ? t.direct_max : t.run_len;      // a single run is one lane's anyway
    while (n > direct && c < POLY_MAX_LEVELS - 1) {
        const uint64_t G = poly_ceil_div(n, t.run_len);
        out[c++] = PolyFoldLevel{n, G};
        n = G;
    }
    if (n) out[c++] = PolyFoldLevel{n, 1};
    return c;
}

// ---- scan: T_i = x_i + mu T_(i + N), T_i = 0 from i = m on.  The m elements fall into N chains (one per residue r mod N)
// of at most K = ceil(m / N) elements; a chain is cut into S = ceil(K / L) segments of L elements.  Lane t < S N is
// (r = t mod N, s = t / N): elements r + k N for s L <= k < min((s + 1) L, chain length of r).  A level with S = 1 is final:
// its lanes scan their whole chain.  Otherwise pass 1 writes the segment's outgoing value to element s N + r of the next
// level's vector (S N elements, same stride N, multiplier mu^L), the next level is scanned, and pass 2 reruns the segment
// from the carry at element (s + 1) N + r of that vector.
struct PolyScanLevel {
    uint64_t m, N, K, S, L;
    GH_PLAN_HD uint64_t lanes() const { return S * N; }
    GH_PLAN_HD uint64_t chain(uint64_t r) const { return r < m ? poly_ceil_div(m - r, N) : 0; }
    // elements [k0, k1) of chain r that lane (r, s) owns
    GH_PLAN_HD void span(uint64_t r, uint64_t s, uint64_t& k0, uint64_t& k1) const {
        const uint64_t c = chain(r);
        k0 = s * L < c ? s * L : c;
        k1 = (s + 1) * L < c ? (s + 1) * L : c;
    }
};
// L: elements per segment; limit: the longest chain one lane finishes (a single segment is one lane's anyway).  -> number of
// levels (0 for m = 0)
inline int poly_scan_levels(uint64_t m, uint64_t N, uint32_t L, uint32_t limit, PolyScanLevel* out) {
    int c = 0;
    if (!m) return 0;
    if (limit < L) limit = L;
    for (;;) {
        const uint64_t K = poly_ceil_div(m, N);
        if (K <= limit || c == POLY_MAX_LEVELS - 1) {
            out[c++] = PolyScanLevel{m, N, K, 1, K};
            return c;
        }
        const uint64_t S = poly_ceil_div(K, L);
        out[c++] = PolyScanLevel{m, N, K, S, L};
        m = S * N;
    }
}

}  // namespace gh
