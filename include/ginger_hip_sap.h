/* ginger_hip_sap.h -- C ABI of GM17's R1CS -> SAP maps over the resident constraint matrices of ginger_hip_r1cs.h: the first
 * stage of GM17's create_proof and the sparse stage of its generate_parameters.  Every call takes a gh_r1cs_t; nothing new
 * is uploaded per circuit.
 *
 *   proof-systems/src/gm17/r1cs_to_sap.rs:125-189, :206-232   the rows witness_map starts its transforms from  -> gh_sap_rows(_dev)
 *   r1cs_to_sap.rs:99-245                                     R1CStoSAP::witness_map as a whole                -> gh_sap_r1cs_witness_map_dev
 *   r1cs_to_sap.rs:14-96 (the loops :37-94)                   instance_map_with_evaluation                     -> gh_sap_instance_map(_dev)
 *
 * Sizes.  With ni = num_inputs (the constant one included), na = num_aux, nc = num_constraints, nv = ni + na of the handle:
 * the SAP domain is N = 2^sap_log_n, the smallest power of two >= 2 nc + 2 (ni - 1) + 1, and the SAP instance has
 * sap_nv = 2 (ni - 1) + na + nc variables besides the constant: the assignment z, one extra variable e_i = (Az_i - Bz_i)^2 per
 * constraint and one f_i = (z_i - 1)^2 per input 1 <= i < ni; full = z || e || f has sap_nv + 1 rows.
 *
 * Vectors are rows of 12 little-endian u64 limbs in the Montgomery form of ginger_hip.h (x 2^768) unless stated; every result
 * is exact.  Status codes, gh_last_error, the locking rules and the behaviour without a usable device are those of
 * ginger_hip_r1cs.h.  Every entry point that takes a handle returns GH_E_UNSUPPORTED, before any device call, where
 * EvaluationDomain::new(2 nc + 2 (ni - 1) + 1) would be None.  The per-row arithmetic: csrc/sap_rows.h.
 */
#ifndef GINGER_HIP_SAP_H
#define GINGER_HIP_SAP_H

#include "ginger_hip_r1cs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t sap_log_n;           /* the SAP domain: 2^sap_log_n >= 2 nc + 2 (ni - 1) + 1 */
    uint32_t reserved;
    uint64_t sap_num_variables;   /* sap_nv */
    uint64_t scratch_bytes;       /* the most a call on this handle takes from the library's pool (gh_sap_r1cs_witness_map_dev) */
} gh_sap_info_t;

int gh_sap_info(gh_r1cs_t handle, gh_sap_info_t* out);

/* r1cs_to_sap.rs:125-189, :206-232 as written.  d_assignment: nv rows, row 0 the constant one.  d_a, d_c: N rows each, every
 * one of them written:  a[2i] = Az_i + Bz_i, a[2i + 1] = Az_i - Bz_i, c[2i] = 4 Cz_i + e_i, c[2i + 1] = e_i for i < nc;
 * a[2 nc] = c[2 nc] = one;  a[2 nc + 2i - 1] = z_i + 1, a[2 nc + 2i] = z_i - 1, c[2 nc + 2i - 1] = 4 z_i + f_i,
 * c[2 nc + 2i] = f_i for 1 <= i < ni;  zero from there on.
 * d_scalars: null, or sap_nv rows that receive into_repr of full[1 ..] (CANONICAL limbs).  d_aux_scalars: null, or
 * sap_nv - (ni - 1) rows that receive the same values of full[ni ..] a second time: the c_query_1 MSM pairs the aux part with
 * two scalars of its own behind it, which cannot sit behind the shared vector. */
int gh_sap_rows_dev(gh_r1cs_t handle, const void* d_assignment, void* d_a, void* d_c, void* d_scalars, void* d_aux_scalars);
/* The same over host buffers; full: sap_nv + 1 Montgomery rows, the reference's full_input_assignment. */
int gh_sap_rows(gh_r1cs_t handle, const uint64_t* assignment, uint64_t* a, uint64_t* c, uint64_t* full);

/* The rows followed by what gh_sap_witness_map_dev does with them, on the library stream with one wait at the end: d_h
 * receives the N + 1 coefficients of h.  d1, d2: Montgomery elements on the host.  The vectors a and c come from the
 * library's pool.  d_scalars, d_aux_scalars: as above. */
int gh_sap_r1cs_witness_map_dev(gh_r1cs_t handle, const void* d_assignment, const uint64_t* d1, const uint64_t* d2, void* d_h,
                                void* d_scalars, void* d_aux_scalars);

/* r1cs_to_sap.rs:37-94.  d_u: N rows (the Lagrange coefficients at t); d_a, d_c: sap_nv + 1 rows, every one written.  With
 * p_i = u[2i] + u[2i + 1], m_i = u[2i] - u[2i + 1], q_i = u[2i]:  a[j] = (A^T p)_j + (B^T m)_j and c[j] = 4 (C^T q)_j for
 * j < nv, plus the input rows (a[0] += u[2 nc] + sum (u[2 nc + 2i - 1] - u[2 nc + 2i]), c[0] += u[2 nc]; a[i] += u[2 nc + 2i - 1]
 * + u[2 nc + 2i], c[i] += 4 u[2 nc + 2i - 1]);  a = 0 on the extra variables, c[nv + i] = p_i,
 * c[nv + nc - 1 + i] = u[2 nc + 2i - 1] + u[2 nc + 2i]. */
int gh_sap_instance_map_dev(gh_r1cs_t handle, const void* d_u, void* d_a, void* d_c);
int gh_sap_instance_map(gh_r1cs_t handle, const uint64_t* u, uint64_t* a, uint64_t* c);

/* Device milliseconds of the last call above, in the layout of gh_r1cs_last_timing: phase 0 the conversion of the assignment
 * (rows) or the split of u (instance map), phase 1 + l level l of the three products, the last phase the SAP kernel. */
int gh_sap_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
