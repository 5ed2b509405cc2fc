/* ginger_hip_ecvrf.h -- C ABI of the batched field-based EC-VRF over MNT4-753 / MNT6-753, of the Bowe-Hopwood Pedersen hash
 * it uses as its group hash, and of the batched joint double-scalar multiplication its verification runs on:
 *
 *   primitives/src/crh/bowe_hopwood/mod.rs:83-151   BoweHopwoodPedersenCRH::evaluate  -> gh_bh_hash
 *   primitives/src/vrf/ecvrf/mod.rs:69-79           keygen / get_public_key           -> gh_ecvrf_public_keys
 *   primitives/src/vrf/ecvrf/mod.rs:81-158          prove                             -> gh_ecvrf_prove
 *   primitives/src/vrf/ecvrf/mod.rs:160-237         proof_to_hash                     -> gh_ecvrf_proof_to_hash
 *   primitives/src/vrf/ecvrf/mod.rs:239-243         keyverify                         -> gh_ecvrf_keyverify
 *
 * The two instances of the reference (:271-282):
 *   EcVrfMNT4: data / hash field MNT4-753 Fr (GH_MNT4753_FR), group GH_MNT6753_G1, secrets mod MNT6-753 Fr, MNT4PoseidonHash,
 *              Bowe-Hopwood over GH_MNT6753_G1
 *   EcVrfMNT6: data / hash field MNT6-753 Fr (GH_MNT6753_FR), group GH_MNT4753_G1, secrets mod MNT4-753 Fr, MNT6PoseidonHash,
 *              Bowe-Hopwood over GH_MNT4753_G1
 *
 * Layout and conventions are those of ginger_hip_schnorr.h: field elements are 12 little-endian u64 limbs of the Montgomery
 * form x * 2^768; sk and nonces are in the Montgomery form of the group's scalar field; a point is affine x || y (24 words)
 * plus an infinity byte, and the point at infinity hashes as GroupAffine::zero() = (0, 1).  A proof is gamma (a point) and
 * c || s (24 words, both in the data field).  Every input element must be below its modulus (GH_E_BAD_ARG otherwise, as for a
 * null pointer, a non-G1 curve or a message longer than the group hash takes).  n == 0 is a successful no-op; without a usable
 * gfx950 device the compute entry points return GH_E_NO_DEVICE.
 *
 * The message of a VRF is hashed to the curve as BH(to_bytes(m_0) || ... || to_bytes(m_(len-1))), each element as its
 * canonical integer in 96 little-endian bytes: len elements need 256 len <= num_windows * window_size chunks.
 */
#ifndef GINGER_HIP_ECVRF_H
#define GINGER_HIP_ECVRF_H

#include "ginger_hip.h"
#include "ginger_hip_poseidon.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_bh* gh_bh_t;
typedef struct gh_ecvrf* gh_ecvrf_t;

/* Bowe-Hopwood parameters over a G1 curve: generators[num_windows][window_size], segment-major rows of x || y (gen_xy) and
 * infinity bytes (gen_inf, NULL = none at infinity).  Coordinates must be below the modulus and every generator not at
 * infinity on the curve.  Host only: the device table of {1, 2, 3, 4} g is built on first use. */
int gh_bh_create(gh_curve_t curve, const uint64_t* gen_xy, const uint8_t* gen_inf, size_t num_windows, size_t window_size, gh_bh_t* out);
int gh_bh_free(gh_bh_t h);
/* out[i] = BH(input[i * nbytes .. (i + 1) * nbytes)), affine (out_xy: n x 24 words) and infinity bytes; the empty input hashes
 * to infinity; 8 nbytes > 3 num_windows window_size is GH_E_BAD_ARG */
int gh_bh_hash(gh_bh_t h, const uint8_t* input, size_t n, size_t nbytes, uint64_t* out_xy, uint8_t* out_inf);
/* out_xyz[i] = k1[i] * (xy1[i], inf1[i]) + k2[i] * (xy2[i], inf2[i]) on a G1 curve, projective in gh_proj_mul's layout
 * (infinity as (0, 1, 0)); scalars are canonical 12-u64 integers below 2^753, inf1 / inf2 may be NULL (no point at infinity);
 * G2: GH_E_UNSUPPORTED */
int gh_batch_double_mul(gh_curve_t curve, const uint64_t* xy1, const uint8_t* inf1, const uint64_t* k1,
                        const uint64_t* xy2, const uint8_t* inf2, const uint64_t* k2, size_t n, uint64_t* out_xyz);
/* curve: GH_MNT6753_G1 (EcVrfMNT4) or GH_MNT4753_G1 (EcVrfMNT6); the hash's field must be the curve's base field and the group
 * hash must be over the same curve; both handles must outlive this one.  window: the generator's fixed-base window, 0 =
 * gh_fixed_base_window(n) of the call, as for gh_schnorr_create. */
int gh_ecvrf_create(gh_curve_t curve, gh_poseidon_t hash, gh_bh_t group_hash, int window, gh_ecvrf_t* out);
int gh_ecvrf_free(gh_ecvrf_t h);
/* out_pk = sk[i] G (affine, infinity for sk == 0) */
int gh_ecvrf_public_keys(gh_ecvrf_t h, const uint64_t* sk, size_t n, uint64_t* out_pk_xy, uint8_t* out_pk_inf);
/* One attempt per row with the caller's nonce r.  out_status[i]: 1 proved, 0 nonce rejected (r == 0, c or s >= 2^752: the
 * reference would draw again; the c || s row is zeroed).  gamma = sk mh is written for every row. */
int gh_ecvrf_prove(gh_ecvrf_t h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n,
                   size_t len, const uint64_t* nonce, uint64_t* out_gamma_xy, uint8_t* out_gamma_inf, uint64_t* out_cs,
                   uint8_t* out_status);
/* out_status[i]: 1 = Ok(output) with the output in out_hash, 0 = Err(FailedVerification), 2 = Err (c or s >= 2^752),
 * 3 = Err (gamma not on the curve); out_hash rows are zero unless the status is 1 */
int gh_ecvrf_proof_to_hash(gh_ecvrf_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                           const uint64_t* gamma_xy, const uint8_t* gamma_inf, const uint64_t* cs, uint64_t* out_hash,
                           uint8_t* out_status);
/* out_ok[i] = 1 if the key is on the curve (both G1s have cofactor 1: the subgroup test) or is the point at infinity */
int gh_ecvrf_keyverify(gh_ecvrf_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok);
/* Of the last gh_ecvrf_prove, gh_ecvrf_proof_to_hash, gh_bh_hash or gh_batch_double_mul: milliseconds of its phases (upload,
 * group hash, fixed-base, variable-base, normalise, hash, finish with the download), *total_ms the whole call.  gh_bh_hash
 * records only its group-hash phase and gh_batch_double_mul only its variable-base phase (tables and the joint kernel), each
 * also as the total; the other phases read 0.  Returns the number of entries written (at most max_phases) or a negative
 * status. */
int gh_ecvrf_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
