// r1cs_plan.h -- the host side of the sparse products of include/ginger_hip_r1cs.h, free of HIP: validation of a CSR matrix
// and its coefficient dictionary, the classes of the dictionary, the transposition, the segmented schedule ("plan") of one
// product, and a host executor of that schedule on fp29.h's host arithmetic.  r1cs.hip uploads exactly these arrays and its
// kernels run exactly this program, so everything but the kernels is checked without a GPU (tests/test_r1cs_host.py through
// tests/host_shim/r1cs_shim.cpp, tests/host_shim/r1cs_check.cpp under the host sanitizers).  DESIGN.md section 16.
//
// The schedule.  y = M x for a sparse M whose rows have 0 .. millions of terms.  A row of t terms is cut into ceil(t / S)
// segments of at most S terms (S: the segment length); one lane sums one segment.  A row with one segment (t <= S, the empty
// row included: it has one segment of no terms) is finished by that lane: it writes y[row].  A row with more segments writes
// one partial per segment, and gets a node on the next level whose terms are those partials -- consecutive entries of the
// level's partial vector, each with coefficient one --, cut into segments in the same way, until one segment is left.  Field
// addition is exact and associative: every schedule gives the same canonical limbs.
//
// A row therefore takes max(1, ceil(log_S t)) levels: 1 for t <= S (a row of one term still needs the lane that applies its
// coefficient), 2 up to S^2, 3 up to S^3; 2^20 terms at S = 32 take four.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <type_traits>
#include <vector>
#include "fp29.h"
#include "modulus.h"

namespace gh {

constexpr uint32_t R1CS_DEFAULT_SEGMENT = 32;
constexpr uint32_t R1CS_FINAL = 0x80000000u;      // Seg::out: the segment closes its row and writes y[out & ~R1CS_FINAL]
constexpr int R1CS_MAX_LEVELS = 32;               // S >= 2 and fewer than 2^31 terms: at most 31 levels

// classes of a dictionary entry; a term's code is class | payload << 3 (payload: the multiplier of a small class, the
// dictionary index of a general one)
enum : uint32_t { R1CS_ZERO = 0, R1CS_ONE = 1, R1CS_MINUS_ONE = 2, R1CS_SMALL = 3, R1CS_MINUS_SMALL = 4, R1CS_GENERAL = 5, R1CS_CLASSES = 6 };
constexpr uint32_t R1CS_SMALL_MAX = 15;           // fp_mul_small_rt takes multipliers below 16

struct R1csSeg {
    uint32_t first, count, out;                   // terms [first, first + count) of the level's source; out: see R1CS_FINAL
};
struct R1csLevel {
    std::vector<R1csSeg> segs;
    uint32_t n_partials = 0;                      // entries this level writes into its partial vector (read by the next level)
};
// One product y = M x: level 0 gathers x through src / code (the matrix's terms in CSR order), the levels above sum the
// partials of the level below.
struct R1csPlan {
    uint32_t rows = 0, n_src = 0, segment = 0, longest = 0;
    std::vector<uint32_t> src, code;              // per term: index into x, class | payload << 3
    std::vector<R1csLevel> levels;                // at least one when rows > 0
    size_t total_partials() const {
        size_t s = 0;
        for (const R1csLevel& l : levels) s += l.n_partials;
        return s;
    }
};

// ---- validation (include/ginger_hip_r1cs.h "refused with GH_E_BAD_ARG"): nullptr, or what is wrong
inline const char* r1cs_check_csr(uint64_t num_rows, uint64_t num_cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id,
                                  uint64_t num_coeffs) {
    if (!row_ptr) return "null row_ptr";
    if (row_ptr[0] != 0) return "row_ptr[0] is not 0";
    for (uint64_t i = 0; i < num_rows; i++)
        if (row_ptr[i + 1] < row_ptr[i]) return "row_ptr is not monotone";
    const uint64_t nnz = row_ptr[num_rows];
    if (nnz >= R1CS_FINAL) return "a matrix holds 2^31 terms or more";
    if (nnz && (!col || !coeff_id)) return "null array with nnz > 0";
    for (uint64_t j = 0; j < nnz; j++) {
        if (col[j] >= num_cols) return "a column index is out of range";
        if (coeff_id[j] >= num_coeffs) return "a coeff_id is out of range";
    }
    return nullptr;
}

// modulus.h under the names the host checks of this header use
template <class P> inline const uint64_t* r1cs_modulus() { return modulus64<P>(); }
template <class P> inline bool r1cs_below(const uint64_t* x) { return below<P>(x); }

// log2 of the QAP domain of EvaluationDomain::new(num_coeffs) (domain.rs:65-72); false where it would be None
template <class P> inline bool r1cs_domain(uint64_t num_coeffs, uint32_t* log_n) {
    constexpr int two_adicity = std::is_same<P, P6>::value ? GH_P6_TWO_ADICITY : GH_P4_TWO_ADICITY;
    uint32_t lg = 0;
    while (lg < 63 && ((uint64_t)1 << lg) < num_coeffs) lg++;
    *log_n = lg;
    return (int)lg < two_adicity;
}

// ---- the dictionary: Montgomery rows (x 2^768) -> internal form, class and payload of every entry
template <class P> inline void r1cs_classify(const uint64_t* coeff_values, size_t num_coeffs, std::vector<Fp>& internal,
                                             std::vector<uint32_t>& code, uint32_t counts[R1CS_CLASSES]) {
    internal.resize(num_coeffs);
    code.resize(num_coeffs);
    for (uint32_t c = 0; c < R1CS_CLASSES; c++) counts[c] = 0;
    Fp mult[R1CS_SMALL_MAX + 1];                  // k in internal form
    mult[0] = fp_zero();
    for (uint32_t k = 1; k <= R1CS_SMALL_MAX; k++) mult[k] = fp_add<P>(mult[k - 1], fp_one<P>());
    for (size_t i = 0; i < num_coeffs; i++) {
        const Fp v = fp_from_abi<P>(reinterpret_cast<const uint32_t*>(coeff_values + 12 * i));
        internal[i] = v;
        uint32_t cls = R1CS_GENERAL, payload = (uint32_t)i;
        if (fp_is_zero(v)) { cls = R1CS_ZERO; payload = 0; }
        else
            for (uint32_t k = 1; k <= R1CS_SMALL_MAX; k++) {
                if (fp_eq(v, mult[k])) { cls = k == 1 ? R1CS_ONE : R1CS_SMALL; payload = k; break; }
                if (fp_eq(v, fp_neg<P>(mult[k]))) { cls = k == 1 ? R1CS_MINUS_ONE : R1CS_MINUS_SMALL; payload = k; break; }
            }
        code[i] = cls | payload << 3;
        counts[cls]++;
    }
}

// ---- transposition: CSR of M (rows x cols) -> CSR of M^T, by a counting sort that is stable in row order
inline void r1cs_transpose(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id,
                           std::vector<uint64_t>& t_ptr, std::vector<uint32_t>& t_col, std::vector<uint32_t>& t_coeff) {
    const uint64_t nnz = row_ptr[rows];
    t_ptr.assign(cols + 1, 0);
    t_col.resize(nnz);
    t_coeff.resize(nnz);
    for (uint64_t j = 0; j < nnz; j++) t_ptr[col[j] + 1]++;
    for (uint64_t c = 0; c < cols; c++) t_ptr[c + 1] += t_ptr[c];
    std::vector<uint64_t> next(t_ptr.begin(), t_ptr.end() - 1);
    for (uint64_t r = 0; r < rows; r++)
        for (uint64_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
            const uint64_t at = next[col[j]]++;
            t_col[at] = (uint32_t)r;
            t_coeff[at] = coeff_id[j];
        }
}

// levels a row of t terms takes at segment length S
inline uint32_t r1cs_row_levels(uint64_t t, uint32_t S) {
    uint32_t l = 1;
    for (uint64_t cap = S; cap < t; cap *= S) l++;
    return l;
}

// ---- the level builder.  The matrix has been validated; dict_code: r1cs_classify's codes.
inline void r1cs_build_plan(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col, const uint32_t* coeff_id,
                            const std::vector<uint32_t>& dict_code, uint32_t S, R1csPlan& plan) {
    const uint64_t nnz = row_ptr[rows];
    plan = R1csPlan();
    plan.rows = (uint32_t)rows;
    plan.n_src = (uint32_t)cols;
    plan.segment = S;
    plan.src.assign(col, col + nnz);
    plan.code.resize(nnz);
    for (uint64_t j = 0; j < nnz; j++) plan.code[j] = dict_code[coeff_id[j]];
    struct Node { uint32_t row, first, count; };
    std::vector<Node> nodes(rows), next;
    for (uint64_t r = 0; r < rows; r++) {
        nodes[r] = Node{(uint32_t)r, (uint32_t)row_ptr[r], (uint32_t)(row_ptr[r + 1] - row_ptr[r])};
        if (nodes[r].count > plan.longest) plan.longest = nodes[r].count;
    }
    while (!nodes.empty()) {
        plan.levels.emplace_back();
        R1csLevel& lv = plan.levels.back();
        next.clear();
        for (const Node& n : nodes) {
            if (n.count <= S) {
                lv.segs.push_back(R1csSeg{n.first, n.count, n.row | R1CS_FINAL});
                continue;
            }
            const uint32_t nseg = (n.count + S - 1) / S;
            next.push_back(Node{n.row, lv.n_partials, nseg});
            for (uint32_t k = 0; k < nseg; k++) {
                const uint32_t c = k + 1 < nseg ? S : n.count - k * S;
                lv.segs.push_back(R1csSeg{n.first + k * S, c, lv.n_partials++});
            }
        }
        nodes.swap(next);
    }
}

// ---- one term and one segment, the text the kernels of r1cs.hip share with the host executor
// acc (+)= coefficient * v for a level-0 term; dict: the dictionary in internal form
template <class P> GH_HD void r1cs_term(Fp& acc, const Fp& v, uint32_t code, const Fp* dict) {
    const uint32_t cls = code & 7u, payload = code >> 3;
    if (cls == R1CS_ZERO) return;
    Fp t = v;                                     // one instance of each operation in the kernel: the classes share add and sub
    if (cls == R1CS_GENERAL) t = fp_mul<P>(v, dict[payload]);
    else if (cls == R1CS_SMALL || cls == R1CS_MINUS_SMALL) t = fp_mul_small_rt<P>(v, payload);
    if (cls == R1CS_MINUS_ONE || cls == R1CS_MINUS_SMALL) acc = fp_sub<P>(acc, t);
    else acc = fp_add<P>(acc, t);
}

// ---- the host executor: the level program on host arithmetic.  x: n_src Montgomery rows, y: rows Montgomery rows.
template <class P> inline void r1cs_plan_run(const R1csPlan& plan, const std::vector<Fp>& dict, const uint64_t* x, uint64_t* y) {
    std::vector<Fp> xs(plan.n_src), below, mine;
    for (uint32_t i = 0; i < plan.n_src; i++) xs[i] = fp_from_abi<P>(reinterpret_cast<const uint32_t*>(x + 12 * (size_t)i));
    for (size_t l = 0; l < plan.levels.size(); l++) {
        const R1csLevel& lv = plan.levels[l];
        mine.assign(lv.n_partials, fp_zero());
        for (const R1csSeg& s : lv.segs) {
            Fp acc = fp_zero();
            for (uint32_t j = s.first; j < s.first + s.count; j++) {
                if (l == 0) r1cs_term<P>(acc, xs[plan.src[j]], plan.code[j], dict.data());
                else acc = fp_add<P>(acc, below[j]);
            }
            if (s.out & R1CS_FINAL) fp_to_abi<P>(reinterpret_cast<uint32_t*>(y + 12 * (size_t)(s.out & ~R1CS_FINAL)), acc);
            else mine[s.out] = acc;
        }
        below.swap(mine);
    }
}

}  // namespace gh
