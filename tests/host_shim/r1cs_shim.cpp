// Host-side shim over ginger-lib_amd/csrc/r1cs_plan.h for tests/test_r1cs_host.py: the validation, the dictionary classes,
// the transposition, the level builder and the host executor of the schedule, compiled by g++ (no GPU, no HIP).
// Build: g++ -O2 -std=c++17 -shared -fPIC -o build/libr1cs_shim.so tests/host_shim/r1cs_shim.cpp.  Test infrastructure.
#include "../../ginger-lib_amd/csrc/r1cs_plan.h"

using namespace gh;

namespace {

template <class P>
int run(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id, const uint64_t* values,
        uint64_t num_coeffs, uint32_t S, int transpose, const uint64_t* x, uint64_t* y) {
    for (uint64_t i = 0; i < num_coeffs; i++)
        if (!r1cs_below<P>(values + 12 * i)) return -1;
    std::vector<Fp> dict;
    std::vector<uint32_t> code;
    uint32_t counts[R1CS_CLASSES];
    r1cs_classify<P>(values, num_coeffs, dict, code, counts);
    R1csPlan plan;
    if (transpose) {
        std::vector<uint64_t> t_ptr;
        std::vector<uint32_t> t_col, t_coeff;
        r1cs_transpose(rows, cols, row_ptr, col, coeff_id, t_ptr, t_col, t_coeff);
        r1cs_build_plan(cols, rows, t_ptr.data(), t_col.data(), t_coeff.data(), code, S, plan);
    } else {
        r1cs_build_plan(rows, cols, row_ptr, col, coeff_id, code, S, plan);
    }
    r1cs_plan_run<P>(plan, dict, x, y);
    return 0;
}

}  // namespace

extern "C" {

// 0, or 1 with *why pointing at what is wrong
int r1cs_shim_check(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id, uint64_t num_coeffs,
                    const char** why) {
    const char* w = r1cs_check_csr(rows, cols, row_ptr, col, coeff_id, num_coeffs);
    if (why) *why = w;
    return w ? 1 : 0;
}

// field: 0 = MNT4-753 Fr (P6), 1 = MNT6-753 Fr (P4), the ids of gh_field_t.  y = M x, or M^T x with transpose
int r1cs_shim_run(int field, uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id,
                  const uint64_t* values, uint64_t num_coeffs, uint32_t S, int transpose, const uint64_t* x, uint64_t* y) {
    if (r1cs_check_csr(rows, cols, row_ptr, col, coeff_id, num_coeffs)) return -1;
    return field == 0 ? run<P6>(rows, cols, row_ptr, col, coeff_id, values, num_coeffs, S, transpose, x, y)
                      : run<P4>(rows, cols, row_ptr, col, coeff_id, values, num_coeffs, S, transpose, x, y);
}

// out_codes[i] = class | payload << 3 of dictionary entry i; counts: entries per class
void r1cs_shim_classify(int field, const uint64_t* values, uint64_t n, uint32_t* out_codes, uint32_t* counts) {
    std::vector<Fp> dict;
    std::vector<uint32_t> code;
    if (field == 0) r1cs_classify<P6>(values, n, dict, code, counts);
    else r1cs_classify<P4>(values, n, dict, code, counts);
    for (uint64_t i = 0; i < n; i++) out_codes[i] = code[i];
}

void r1cs_shim_transpose(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id, uint64_t* t_ptr,
                         uint32_t* t_col, uint32_t* t_coeff) {
    std::vector<uint64_t> p;
    std::vector<uint32_t> c, k;
    r1cs_transpose(rows, cols, row_ptr, col, coeff_id, p, c, k);
    for (size_t i = 0; i < p.size(); i++) t_ptr[i] = p[i];
    for (size_t i = 0; i < c.size(); i++) { t_col[i] = c[i]; t_coeff[i] = k[i]; }
}

uint32_t r1cs_shim_row_levels(uint64_t t, uint32_t S) { return r1cs_row_levels(t, S); }

// The shape of a schedule (every dictionary entry taken as `one`): returns the number of levels; seen[j] is incremented once
// per level-0 segment that covers term j; segs_per_level / partials_per_level receive up to max_levels entries;
// finals[row] counts the segments that close the row, over all levels; *bad is set if a segment is longer than S, a level
// above 0 reads outside the partials of the level below, or does not read each of them exactly once.
uint32_t r1cs_shim_shape(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id, uint64_t num_coeffs,
                         uint32_t S, uint32_t* seen, uint32_t* finals, uint32_t* segs_per_level, uint32_t* partials_per_level, uint32_t max_levels,
                         int* bad) {
    std::vector<uint32_t> code(num_coeffs, (uint32_t)R1CS_ONE | 1u << 3);
    R1csPlan plan;
    r1cs_build_plan(rows, cols, row_ptr, col, coeff_id, code, S, plan);
    *bad = 0;
    for (size_t l = 0; l < plan.levels.size(); l++) {
        const R1csLevel& lv = plan.levels[l];
        if (l < max_levels) { segs_per_level[l] = (uint32_t)lv.segs.size(); partials_per_level[l] = lv.n_partials; }
        std::vector<uint32_t> read(l ? plan.levels[l - 1].n_partials : 0, 0), wrote(lv.n_partials, 0);
        for (const R1csSeg& s : lv.segs) {
            if (s.count > S) *bad = 1;
            for (uint32_t j = s.first; j < s.first + s.count; j++) {
                if (l == 0) seen[j]++;
                else if (j >= read.size()) *bad = 1;
                else read[j]++;
            }
            if (s.out & R1CS_FINAL) finals[s.out & ~R1CS_FINAL]++;
            else if (s.out >= wrote.size()) *bad = 1;
            else wrote[s.out]++;
        }
        for (uint32_t r : read) if (r != 1) *bad = 1;
        for (uint32_t w : wrote) if (w != 1) *bad = 1;
    }
    if (!plan.levels.empty() && plan.levels.back().n_partials) *bad = 1;
    return (uint32_t)plan.levels.size();
}

}  // extern "C"
