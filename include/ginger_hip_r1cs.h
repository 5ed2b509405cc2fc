/* ginger_hip_r1cs.h -- C ABI of the constraint matrices of an R1CS instance, resident on the device, and of the sparse
 * products over them: the first stage of create_proof and the sparse stage of generate_parameters.
 *
 *   proof-systems/src/groth16/r1cs_to_qap.rs:78-119, :141-151   evaluate_constraint over at / bt / ct   -> gh_r1cs_evaluate(_dev)
 *   r1cs_to_qap.rs:71-169                                       R1CStoQAP::witness_map as a whole        -> gh_r1cs_witness_map_dev
 *   r1cs_to_qap.rs:14-69 (the loops :32-65)                     instance_map_with_evaluation             -> gh_r1cs_instance_map(_dev)
 *   y = M x and y = M^T x for one of the three matrices (the piece GM17's R1CStoSAP rows need)          -> gh_r1cs_matvec_dev
 *
 * The matrices are static per circuit, as the proving key is: they are uploaded once (gh_r1cs_upload) and a proof then
 * sends the assignment alone.  Producing the assignment (synthesis) stays with the caller.
 *
 * A matrix is given in CSR form: row_ptr (num_constraints + 1 offsets), col (nnz variable indices: 0 .. num_inputs - 1 are
 * the inputs, 0 the constant one, then the aux variables -- the reference's Index::Input(i) -> i, Index::Aux(i) ->
 * num_inputs + i) and coeff_id (nnz indices into a dictionary of num_coeffs Montgomery rows of 12 u64).  R1CS coefficients
 * are overwhelmingly 1, -1 and a handful of small constants, so a term costs 8 bytes instead of 104; the library sorts the
 * dictionary into classes once (zero, one, minus one, +-2 .. +-15, general) and only a general term costs a product.  A row
 * may be empty, may repeat an index (both occurrences count) and may carry a zero coefficient.
 *
 * Vectors are rows of 12 little-endian u64 limbs in the Montgomery form of ginger_hip.h (x 2^768) unless stated.  Every
 * product is exact: the result rows are the canonical Montgomery limbs of the reference's field elements, whatever the
 * schedule.  Status codes, gh_last_error and the locking rules are those of ginger_hip.h; without a usable gfx950 device
 * every entry point that needs one returns GH_E_NO_DEVICE.  The schedule of the products: csrc/r1cs_plan.h.
 */
#ifndef GINGER_HIP_R1CS_H
#define GINGER_HIP_R1CS_H

#include "ginger_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_r1cs* gh_r1cs_t;

typedef struct {
    const uint64_t* row_ptr;      /* num_constraints + 1, row_ptr[0] = 0, monotone; nnz = row_ptr[num_constraints] */
    const uint32_t* col;          /* nnz, each below num_inputs + num_aux */
    const uint32_t* coeff_id;     /* nnz, each below num_coeffs */
    const uint64_t* coeff_values; /* num_coeffs x 12, Montgomery, each below the modulus */
    size_t num_coeffs;
} gh_r1cs_matrix_t;

typedef struct {
    uint64_t num_inputs, num_aux, num_constraints;
    uint32_t log_n;               /* the QAP domain: 2^log_n >= num_constraints + num_inputs */
    uint32_t segment_terms;       /* the segment length in force */
    /* per matrix (A, B, C) and orientation (0: M, 1: M^T): terms, longest row, levels of the schedule */
    uint64_t nnz[3][2];
    uint32_t longest_row[3][2];
    uint32_t levels[3][2];
    /* dictionary entries by class, over the three matrices: zero, one, minus one, small (2 .. 15), minus small, general */
    uint32_t class_counts[6];
    uint64_t device_bytes;        /* held by the handle (scratch of a call comes from the library's pool) */
} gh_r1cs_info_t;

/* Uploads A, B, C (m[0], m[1], m[2]), builds the transposed form of each on the host (a counting sort, stable in row
 * order) and the schedules of both orientations; all of it lives on the device.  segment_terms: 0 = the default (32), else
 * at least 2: the segment length of this handle's schedules (small values let small matrices reach every level).
 * GH_E_BAD_ARG, before any device call: a null array with nnz > 0, row_ptr[0] != 0 or a non-monotone row_ptr, a column
 * >= num_inputs + num_aux, a coeff_id >= num_coeffs, a dictionary value >= the modulus, num_inputs == 0, segment_terms == 1,
 * an unknown field.  GH_E_UNSUPPORTED where EvaluationDomain::new(num_constraints + num_inputs) would be None. */
int gh_r1cs_upload(gh_field_t field, size_t num_inputs, size_t num_aux, size_t num_constraints, const gh_r1cs_matrix_t* m /* 3 */,
                   uint32_t segment_terms, gh_r1cs_t* out);
int gh_r1cs_free(gh_r1cs_t handle);
int gh_r1cs_info(gh_r1cs_t handle, gh_r1cs_info_t* out);

/* y = M x (x: num_inputs + num_aux rows, y: num_constraints rows) or, with transpose != 0, y = M^T x (lengths swapped) for
 * M = A, B, C (which = 0, 1, 2); device pointers; every row of y is written.  Synchronous on the library stream. */
int gh_r1cs_matvec_dev(gh_r1cs_t handle, int which, int transpose, const void* d_x, void* d_y);

/* r1cs_to_qap.rs:105-119, :141-151 as written.  d_assignment: the full assignment (num_inputs + num_aux rows, row 0 the
 * constant one).  d_a, d_b, d_c: 2^log_n rows each.  Rows [0, num_constraints) are A z, B z, C z; a[num_constraints + i] =
 * one for i = 0 (the constant, not z_0) and z_i for 0 < i < num_inputs; every other row of all three is written as zero. */
int gh_r1cs_evaluate_dev(gh_r1cs_t handle, const void* d_assignment, void* d_a, void* d_b, void* d_c);
int gh_r1cs_evaluate(gh_r1cs_t handle, const uint64_t* assignment, uint64_t* a, uint64_t* b, uint64_t* c);

/* The evaluation followed by what gh_witness_map_dev does with its rows, on the library stream with one wait at the end:
 * d_h receives the 2^log_n + 1 coefficients of h.  d1, d2, d3: Montgomery elements on the host.  d_scalars: null, or
 * num_inputs + num_aux - 1 rows that receive into_repr of z[1 ..] (CANONICAL limbs): the scalar vector input || aux of the
 * MSM stage, so that the assignment crosses to the device once. */
int gh_r1cs_witness_map_dev(gh_r1cs_t handle, const void* d_assignment, const uint64_t* d1, const uint64_t* d2, const uint64_t* d3,
                            void* d_h, void* d_scalars);

/* r1cs_to_qap.rs:32-65.  d_u: 2^log_n rows (the Lagrange coefficients at t); d_a, d_b, d_c: num_inputs + num_aux rows:
 * a = A^T u with a[i] += u[num_constraints + i] for i < num_inputs, b = B^T u, c = C^T u. */
int gh_r1cs_instance_map_dev(gh_r1cs_t handle, const void* d_u, void* d_a, void* d_b, void* d_c);
int gh_r1cs_instance_map(gh_r1cs_t handle, const uint64_t* u, uint64_t* a, uint64_t* b, uint64_t* c);

/* Device milliseconds of the last call on a handle, by HIP events on the library stream: phase 0 the conversion of the input
 * vector, phase 1 + l level l of the schedule (of gh_r1cs_matvec_dev; for the calls of three products, summed over the three),
 * the last phase what follows the products (the tail rows of evaluate, the input rows of instance_map); *total_ms from the
 * first to the last event (gh_r1cs_witness_map_dev: the evaluation part).  Returns the number of entries written (at most
 * max_phases) or a negative status. */
int gh_r1cs_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
