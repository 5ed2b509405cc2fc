// poly_shim.cpp -- the host executor of the polynomial unit (poly_host.h) behind a C interface, for tests/test_poly_host.py.
// field: 0 = MNT4-753 Fr, 1 = MNT6-753 Fr, as gh_field_t.  Vectors are rows of 12 u64 in the ABI's form.
#include "poly_host.h"

using namespace poly_host;
typedef const uint32_t* R;
typedef uint32_t* W;
#define BY_FIELD(field, fn, ...) ((field) == 0 ? fn<P6>(__VA_ARGS__) : fn<P4>(__VA_ARGS__))

static PolyTuning tuning(uint32_t run_len, uint32_t direct_max, uint32_t seg_max) {
    PolyTuning t;
    if (run_len) t.run_len = run_len;
    if (direct_max) t.direct_max = direct_max;
    if (seg_max) t.seg_max = seg_max;
    return t;
}

extern "C" {

void poly_shim_evaluate(int field, const void* c, uint64_t n, const void* pts, uint64_t k, uint32_t run_len, uint32_t direct_max, void* out) {
    BY_FIELD(field, evaluate, (R)c, n, (R)pts, k, tuning(run_len, direct_max, 0), (W)out);
}
void poly_shim_divide_linear(int field, const void* c, uint64_t n, const void* z, uint32_t run_len, uint32_t direct_max, void* q, void* rem) {
    BY_FIELD(field, divide_linear, (R)c, n, (R)z, tuning(run_len, direct_max, 0), (W)q, (W)rem);
}
void poly_shim_divide_vanishing(int field, const void* c, uint64_t n, uint32_t log_n, uint32_t seg_max, void* q, void* r) {
    BY_FIELD(field, divide_vanishing, (R)c, n, log_n, tuning(0, 0, seg_max), (W)q, (W)r);
}
void poly_shim_axpy(int field, int op, const void* a, uint64_t na, const void* b, uint64_t nb, const void* f, void* out) {
    BY_FIELD(field, axpy, op, (R)a, na, (R)b, nb, (R)f, (W)out);
}
void poly_shim_mul_vanishing(int field, const void* c, uint64_t n, uint32_t log_n, void* out) { BY_FIELD(field, mul_vanishing, (R)c, n, log_n, (W)out); }
uint64_t poly_shim_trimmed_len(const void* rows, uint64_t n) { return reduce((R)rows, n, false); }
uint64_t poly_shim_count_zero(const void* rows, uint64_t n) { return reduce((R)rows, n, true); }
void poly_shim_elements(int field, const void* g, uint32_t log_n, void* out) { BY_FIELD(field, elements, (R)g, log_n, (W)out); }
void poly_shim_sparse(int field, const void* g, const uint64_t* exps, const void* coeffs, uint64_t t, uint32_t log_n, void* out) {
    BY_FIELD(field, sparse, (R)g, exps, (R)coeffs, t, log_n, (W)out);
}
int poly_shim_fold_cover(uint64_t n, uint32_t run_len, uint32_t direct_max) { return fold_cover(n, tuning(run_len, direct_max, 0)); }
int poly_shim_scan_cover(uint64_t m, uint64_t N, uint32_t L, uint32_t limit) { return scan_cover(m, N, L, limit); }
int poly_shim_fold_levels(uint64_t n, uint32_t run_len, uint32_t direct_max) {
    PolyFoldLevel lv[POLY_MAX_LEVELS];
    return poly_fold_levels(n, tuning(run_len, direct_max, 0), lv);
}

}  // extern "C"
