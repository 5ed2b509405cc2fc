/* ginger_hip_pairing.h -- C ABI of the batched MNT4-753 and MNT6-753 reduced ate pairings and of the Groth16 verifier built
 * on them:
 *
 *   algebra/src/curves/models/mnt4/mod.rs:157-269   ate_miller_loop, final_exponentiation (engine GH_PAIRING_MNT4753)
 *   algebra/src/curves/models/mnt6/mod.rs:158-272   the same for MNT6-753                 (engine GH_PAIRING_MNT6753)
 *   PairingEngine::pairing / product_of_pairings    -> gh_pairing_product
 *   proof-systems/src/groth16/verifier.rs:9-16      prepare_verifying_key -> gh_groth16_vk_create
 *   proof-systems/src/groth16/verifier.rs:18-44     verify_proof          -> gh_groth16_verify
 *
 * Field elements are 12 little-endian u64 limbs of the Montgomery form x * 2^768 of MNT4-753 Fq, as in ginger_hip.h.  A G1
 * point is affine x || y (24 words) plus an infinity byte; a G2 point is x.c0 || x.c1 || y.c0 || y.c1 (48 words) plus an
 * infinity byte.  An element of the target field Fq4 is c0.c0 || c0.c1 || c1.c0 || c1.c1 (48 words), the order of Fp4::write:
 * the canonical little-endian bytes of a pairing value are the alpha_g1_beta_g2 of a Parameters::write stream.  Public inputs
 * are in the Montgomery form of MNT4-753 Fr.  Every element must be below its modulus (GH_E_BAD_ARG otherwise, as for a null
 * pointer or an unknown engine).  Status codes, gh_init / gh_last_error and the locking rules are those of ginger_hip.h;
 * n == 0 is a successful no-op; without a usable gfx950 device the compute entry points return GH_E_NO_DEVICE.
 *
 * The value after the final exponentiation is the reference's, word for word.  The Miller value before it is not: the device
 * runs its own line formulas (csrc/pairing29.h), which the full exponent makes equal.
 *
 * Deviation, points at infinity: a pair with either point at infinity contributes one to the product.  The reference's
 * G1Prepared / G2Prepared of the point at infinity compute with the coordinates (0, 1) of GroupAffine::zero() instead, a
 * value without meaning; callers of the reference never pair the point at infinity.
 *
 * Engine GH_PAIRING_MNT6753: the same rules over MNT6-753 Fq.  A G1 point is x || y (24 words); a G2 point is
 * x.c0 || x.c1 || x.c2 || y.c0 || y.c1 || y.c2 (72 words); an element of the target field Fq6 is c0.c0 || c0.c1 || c0.c2 ||
 * c1.c0 || c1.c1 || c1.c2 (72 words), the order of Fp6::write; public inputs are in the Montgomery form of MNT6-753 Fr.  Points at
 * infinity, rows with a point off its curve (status 2), subgroup membership and bad arguments are treated as for MNT4-753.
 *
 * Subgroup membership is the caller's job in this header.  The reference checks it where a point is read (GroupAffine::read),
 * not in the pairing or the verifier; G1 has cofactor 1, so there it is the curve equation.  For a G2 point on the curve but
 * outside the subgroup of order r the value is unspecified; no input faults, hangs or loops, and the inverse of zero is taken
 * as zero.  ginger_hip_points.h does that job on the device: gh_group_membership, and gh_groth16_verify_checked /
 * gh_groth16_verify_compressed, which validate A, B and C before they verify.
 */
#ifndef GINGER_HIP_PAIRING_H
#define GINGER_HIP_PAIRING_H

#include "ginger_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_PAIRING_MNT4753 0
#define GH_PAIRING_MNT6753 2    /* every other engine id, 1 included, is unknown: GH_E_BAD_ARG */

typedef struct gh_groth16_vk* gh_groth16_vk_t;

/* out_gt[i] = final_exponentiation(prod_{j<k} miller_loop(P_ij, Q_ij)), 1 <= k <= 3: PairingEngine::pairing for k = 1,
 * product_of_pairings for k > 1.  Pair j of row i is at index i * k + j of g1_xy / g1_inf / g2_xy / g2_inf. */
int gh_pairing_product(int engine, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                       size_t n, size_t k, uint64_t* out_gt);
/* prepare_verifying_key: keeps alpha_g1_beta_g2, -gamma_g2, -delta_g2 and gamma_abc_g1 (n_abc >= 1 affine points, none at
 * infinity).  Host only: checks that every coefficient is below the modulus and every point on its curve; the two prepared
 * line tables (499 x 3 Fq2 each, Fq3 on MNT6-753) and the fixed-base tables of gamma_abc_g1[1..] are built on the device on first use. */
int gh_groth16_vk_create(int engine, const uint64_t* alpha_g1_beta_g2, const uint64_t* gamma_g2_xy, const uint64_t* delta_g2_xy,
                         const uint64_t* gamma_abc_g1_xy, size_t n_abc, gh_groth16_vk_t* out);
int gh_groth16_vk_free(gh_groth16_vk_t h);
/* n proofs (A, B, C) with n_inputs public inputs each (row i at inputs + i * n_inputs * 12); GH_E_BAD_ARG unless
 * n_inputs + 1 == n_abc (the reference: MalformedVerifyingKey).  out_status[i]: 1 = Ok(true), 0 = Ok(false), 2 = a proof point
 * is not on its curve (the row is not evaluated).  The verdict is
 *   final_exponentiation(miller(A, B) miller(g_ic, -gamma) miller(C, -delta)) == alpha_g1_beta_g2,
 *   g_ic = gamma_abc_g1[0] + sum_j inputs[i][j] gamma_abc_g1[j + 1]. */
int gh_groth16_verify(gh_groth16_vk_t h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                      const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs,
                      uint8_t* out_status);
/* Of the last gh_pairing_product or gh_groth16_verify: milliseconds of its phases (upload, g_ic, Miller loop, final
 * exponentiation, compare, download; a phase the call does not have reads 0), *total_ms the whole call.  Returns the number
 * of entries written (at most max_phases) or a negative status. */
int gh_pairing_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
