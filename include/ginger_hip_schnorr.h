/* ginger_hip_schnorr.h -- C ABI of the batched field-based Schnorr signature over MNT4-753 / MNT6-753 and of the batched
 * variable-base scalar multiplication it is built on:
 *
 *   primitives/src/signature/schnorr/field_based_schnorr.rs:57-67    keygen / get_public_key -> gh_schnorr_public_keys
 *   primitives/src/signature/schnorr/field_based_schnorr.rs:69-127   sign                    -> gh_schnorr_sign
 *   primitives/src/signature/schnorr/field_based_schnorr.rs:129-170  verify                  -> gh_schnorr_verify
 *   primitives/src/signature/schnorr/field_based_schnorr.rs:173-176  keyverify               -> gh_schnorr_keyverify
 *
 * The two instances of the reference (:195-196):
 *   SchnorrMNT4: data / hash field MNT4-753 Fr (GH_MNT4753_FR), group GH_MNT6753_G1, secrets mod MNT6-753 Fr, MNT4PoseidonHash
 *   SchnorrMNT6: data / hash field MNT6-753 Fr (GH_MNT6753_FR), group GH_MNT4753_G1, secrets mod MNT4-753 Fr, MNT6PoseidonHash
 * The group's base field is the data field, so messages, signatures (e || s) and key coordinates are elements of one field.
 *
 * Field elements are 12 little-endian u64 limbs of the Montgomery form x * 2^768, as in ginger_hip.h; sk and nonce are in the
 * Montgomery form of the group's scalar field.  A public key is affine x || y (24 words) plus an infinity byte, as gh_msm
 * takes its bases; the point at infinity hashes as GroupAffine::zero() = (0, 1).  Every input element must be below its
 * modulus (GH_E_BAD_ARG otherwise, as for a null pointer, a non-G1 curve or a hash over another field).  A message is any
 * number len >= 0 of elements, the same len for all n rows of one call.  Status codes, gh_init / gh_last_error and the
 * locking rules are those of ginger_hip.h; n == 0 is a successful no-op; without a usable gfx950 device the compute entry
 * points return GH_E_NO_DEVICE.
 */
#ifndef GINGER_HIP_SCHNORR_H
#define GINGER_HIP_SCHNORR_H

#include "ginger_hip.h"
#include "ginger_hip_poseidon.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_schnorr* gh_schnorr_t;

/* curve: GH_MNT6753_G1 (SchnorrMNT4) or GH_MNT4753_G1 (SchnorrMNT6); the hash's field must be the curve's base field and the
 * hash handle must outlive this one.  Host only: the generator's fixed-base table is built on first use.  window: the
 * fixed-base window; 0 = gh_fixed_base_window(n) of the call, the table rebuilt when a call's n asks for a larger window. */
int gh_schnorr_create(gh_curve_t curve, gh_poseidon_t hash, int window, gh_schnorr_t* out);
int gh_schnorr_free(gh_schnorr_t h);
/* out_pk = sk[i] G (affine, infinity for sk == 0) */
int gh_schnorr_public_keys(gh_schnorr_t h, const uint64_t* sk, size_t n, uint64_t* out_pk_xy, uint8_t* out_pk_inf);
/* out_status[i]: 1 signed, 0 nonce rejected (k == 0, e or s >= 2^752: the reference would draw again; out_sig row zeroed) */
int gh_schnorr_sign(gh_schnorr_t h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg,
                    size_t n, size_t len, const uint64_t* nonce, uint64_t* out_sig, uint8_t* out_status);
/* out_status[i]: 1 = Ok(true), 0 = Ok(false), 2 = Err (e or s >= 2^752) */
int gh_schnorr_verify(gh_schnorr_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                      const uint64_t* sig, uint8_t* out_status);
/* out_ok[i] = 1 if the key is on the curve (both G1s have cofactor 1: the subgroup test) or is the point at infinity */
int gh_schnorr_keyverify(gh_schnorr_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok);
/* out_xyz[i] = scalars[i] * (xy[i], inf[i]) on a G1 curve, projective in gh_proj_mul's layout (infinity as (0, 1, 0));
 * scalars are canonical 12-u64 integers below 2^753, inf may be NULL (no point at infinity); G2: GH_E_UNSUPPORTED */
int gh_batch_mul(gh_curve_t curve, const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_xyz);
/* Of the last gh_schnorr_sign, gh_schnorr_verify or gh_batch_mul: milliseconds of its phases (upload, fixed-base,
 * variable-base, normalise, hash, compare / finish with the download), *total_ms the whole call.  gh_batch_mul records only
 * its variable-base phase (the two kernels) and reports it as the total as well; the other phases read 0.  Returns the
 * number of entries written (at most max_phases) or a negative status. */
int gh_schnorr_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
