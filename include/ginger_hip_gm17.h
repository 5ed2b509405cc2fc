/* ginger_hip_gm17.h -- C ABI of the batched GM17 verifier over the MNT4-753 and MNT6-753 pairings of ginger_hip_pairing.h:
 *
 *   proof-systems/src/gm17/verifier.rs:9-22    prepare_verifying_key -> gh_gm17_vk_create
 *   proof-systems/src/gm17/verifier.rs:24-76   verify_proof          -> gh_gm17_verify
 *
 * Layouts (12 u64 Montgomery limbs per Fq element, G1 x || y, G2 and target-field elements per engine), engine ids
 * (GH_PAIRING_MNT4753, GH_PAIRING_MNT6753; every other id, 1 included, is GH_E_BAD_ARG), status codes, locking, the n == 0
 * no-op and GH_E_NO_DEVICE are those of ginger_hip_pairing.h.  Subgroup membership is the caller's job; no input faults,
 * hangs or loops, and the inverse of zero is taken as zero.
 *
 * Per row, with complete group additions (a doubling, opposite points and a point at infinity included):
 *   S1 = A + g_alpha,  S2 = B + h_beta,  g_psi = query[0] + sum_j inputs[j] query[j + 1]
 *   test1:  final_exponentiation(miller(-S1, S2) miller(g_psi, h_gamma) miller(C, h)) == e(-g_alpha, h_beta)
 *   test2:  final_exponentiation(miller(A, h_gamma) miller(g_gamma, -B)) == 1
 * e(-g_alpha, h_beta) = e(g_alpha, h_beta)^-1 is computed once per key, on the device, on first use: test1 is the reference's
 * test1_exp * alpha_g1_beta_g2 == 1.  The rule of ginger_hip_pairing.h for infinity applies after the additions: a pair with
 * either point at infinity (S1, S2, g_psi, A, B or C) contributes one.
 */
#ifndef GINGER_HIP_GM17_H
#define GINGER_HIP_GM17_H

#include "ginger_hip_pairing.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_gm17_vk* gh_gm17_vk_t;

/* prepare_verifying_key: keeps g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, h_g2 and query (n_query >= 1 affine G1 points).
 * No key point may be at infinity: the arrays carry no infinity byte.  Host only: GH_E_BAD_ARG for a null pointer, an unknown
 * engine, n_query == 0, a coefficient not below the modulus or a point off its curve.  The prepared line tables of h_gamma
 * and h, e(-g_alpha, h_beta) and the fixed-base tables of query[1..] are built on the device on first use. */
int gh_gm17_vk_create(int engine, const uint64_t* g_alpha_g1_xy, const uint64_t* h_beta_g2_xy, const uint64_t* g_gamma_g1_xy,
                      const uint64_t* h_gamma_g2_xy, const uint64_t* h_g2_xy, const uint64_t* query_g1_xy, size_t n_query,
                      gh_gm17_vk_t* out);
int gh_gm17_vk_free(gh_gm17_vk_t h);
/* n proofs (A, B, C) with n_inputs public inputs each (row i at inputs + i * n_inputs * 12, Montgomery form of the engine's
 * Fr); GH_E_BAD_ARG unless n_inputs + 1 == n_query (the reference: MalformedVerifyingKey).  out_status[i]: 1 = Ok(true): both
 * tests hold, 0 = Ok(false), 2 = A, B or C is not on its curve (the row is not evaluated). */
int gh_gm17_verify(gh_gm17_vk_t h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                   const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs,
                   uint8_t* out_status);
/* Of the last gh_gm17_verify: milliseconds of its phases (upload, g_psi, sums, Miller loop of test1, final exponentiation of
 * test1, Miller loop of test2, final exponentiation of test2, compare, download), *total_ms the whole call.  Returns the
 * number of entries written (at most max_phases) or a negative status.  gh_pairing_last_timing does not see this call. */
int gh_gm17_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
