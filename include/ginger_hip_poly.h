/* ginger_hip_poly.h -- DensePolynomial, SparsePolynomial and Evaluations arithmetic on the device: the part of algebra::fft
 * above the transforms of ginger_hip.h.
 *
 *   algebra/src/fft/polynomial/dense.rs:86-103    evaluate                        -> gh_poly_evaluate*
 *   dense.rs:64-73                                from_coefficients_vec's pops    -> gh_poly_trimmed_len_dev
 *   dense.rs:150-328                              Add / Sub / AddAssign((f, p)) / Neg -> gh_poly_add_dev .. gh_poly_neg_dev
 *   dense.rs:134-139                              mul_by_vanishing_poly           -> gh_poly_mul_by_vanishing_dev
 *   dense.rs:143-147, polynomial/mod.rs:105-132   divide_by_vanishing_poly        -> gh_poly_divide_by_vanishing*
 *   dense.rs:330-339                              Div by a monic linear divisor   -> gh_poly_divide_by_linear*
 *   dense.rs:342-357                              Mul                             -> gh_poly_mul*
 *   evaluations.rs:119-125                        DivAssign                       -> gh_evals_div_dev
 *   domain.rs:234-240                             elements                        -> gh_domain_elements_dev
 *   polynomial/mod.rs:147-154                     a sparse polynomial over a domain -> gh_poly_sparse_evaluate_over_domain_dev
 *
 * A vector is n rows of 12 u64 in Montgomery form (x 2^768), canonical; d_* are device pointers, field scalars cross as
 * 12-u64 host values in the same form.  Everything is exact.  Output vectors must not overlap input vectors unless a function
 * says so.  Status codes, gh_last_error and the threading rules are those of ginger_hip.h; there is no CPU fallback.
 * Argument checks come in this order: unknown field, null pointer with a non-zero length, k = 0, log_n beyond the field's
 * 2-adicity (GH_E_UNSUPPORTED). */
#ifndef GINGER_HIP_POLY_H
#define GINGER_HIP_POLY_H
#include "ginger_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out12[j] = sum_i c_i z_j^i for the k >= 1 points z_j (k rows of 12 u64 each way).  n = 0 or all-zero coefficients give 0;
 * the coefficients need not be trimmed. */
int gh_poly_evaluate_dev(gh_field_t field, const void* d_coeffs, size_t n, const uint64_t* points12, size_t k, uint64_t* out12);
int gh_poly_evaluate(gh_field_t field, const uint64_t* coeffs, size_t n, const uint64_t* points12, size_t k, uint64_t* out12);

/* Vec::resize(n_out, zero): d_out (n_out rows, not d_in) = the first min(n, n_out) rows of d_in, then zeros */
int gh_poly_resize_dev(gh_field_t field, const void* d_in, size_t n, void* d_out, size_t n_out);

/* *len = index of the last non-zero row plus one, 0 if there is none */
int gh_poly_trimmed_len_dev(gh_field_t field, const void* d, size_t n, size_t* len);

/* d_out: max(n_a, n_b) rows; the shorter operand is read as zeros beyond its length.  d_out may be d_a or d_b.
 * add_scaled: a + f b.  neg: n rows. */
int gh_poly_add_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, void* d_out);
int gh_poly_sub_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, void* d_out);
int gh_poly_add_scaled_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, const uint64_t* f12, void* d_out);
int gh_poly_neg_dev(gh_field_t field, const void* d_a, size_t n, void* d_out);

/* p (x^N - 1), N = 2^log_n: d_out holds n + N rows, out[i] = in[i - N] - in[i] */
int gh_poly_mul_by_vanishing_dev(gh_field_t field, const void* d_in, size_t n, uint32_t log_n, void* d_out);

/* p = q (x^N - 1) + r: d_q holds max(n, N) - N rows, d_r holds N rows, both written in full and not trimmed */
int gh_poly_divide_by_vanishing_dev(gh_field_t field, const void* d_in, size_t n, uint32_t log_n, void* d_q, void* d_r);
int gh_poly_divide_by_vanishing(gh_field_t field, const uint64_t* in, size_t n, uint32_t log_n, uint64_t* q, uint64_t* r);

/* p = q (x - z) + rem: d_q holds max(n, 1) - 1 rows, rem12 = p(z).  n = 0 gives rem = 0. */
int gh_poly_divide_by_linear_dev(gh_field_t field, const void* d_in, size_t n, const uint64_t* z12, void* d_q, uint64_t* rem12);
int gh_poly_divide_by_linear(gh_field_t field, const uint64_t* in, size_t n, const uint64_t* z12, uint64_t* q, uint64_t* rem12);

/* Mul.  An operand that trims to length zero gives *n_out = 0 and leaves d_out alone.  Otherwise the domain is that of
 * n_a + n_b coefficients (the lengths given, as the reference takes coeffs.len()): GH_E_UNSUPPORTED if the field has none,
 * GH_E_BAD_ARG if out_cap (rows of d_out) is below its size; d_out then holds the product in its first *n_out rows (trimmed)
 * and zeros up to the domain's size. */
int gh_poly_mul_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, void* d_out, size_t out_cap, size_t* n_out);
int gh_poly_mul(gh_field_t field, const uint64_t* a, size_t n_a, const uint64_t* b, size_t n_b, uint64_t* out, size_t out_cap, size_t* n_out);

/* a[i] /= b[i].  *zero_divisors = the number of zero rows of b; where it is not 0, a is left untouched (the reference panics). */
int gh_evals_div_dev(gh_field_t field, void* d_a, const void* d_b, size_t n, size_t* zero_divisors);

/* out[i] = group_gen^i, i < 2^log_n */
int gh_domain_elements_dev(gh_field_t field, uint32_t log_n, void* d_out);

/* out[i] = sum_j coeffs12[j] group_gen^((i exps[j]) mod N), i < N = 2^log_n; exps, coeffs12 (t rows): host arrays */
int gh_poly_sparse_evaluate_over_domain_dev(gh_field_t field, const uint64_t* exps, const uint64_t* coeffs12, size_t t, uint32_t log_n, void* d_out);

/* Elements a lane folds or scans with products (run_len), the longest vector one lane finishes (direct_max), additions a lane
 * of divide_by_vanishing makes (seg_max).  0 = the default (32, 32, 64); 1 is refused for run_len and seg_max. */
int gh_poly_set_tuning(uint32_t run_len, uint32_t direct_max, uint32_t seg_max);

/* device milliseconds of the last gh_poly_* / gh_evals_* / gh_domain_elements call, first launch to last */
int gh_poly_last_timing(float* ms);

#ifdef __cplusplus
}
#endif
#endif
