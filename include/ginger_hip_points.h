/* ginger_hip_points.h -- C ABI of batched point validation and of the compressed wire form of a point, on the device, for
 * G1 and G2 of MNT4-753 and MNT6-753, and of the Groth16 verifiers that validate their proofs first:
 *
 *   algebra/src/curves/models/short_weierstrass_projective.rs:106-121, :149-151   group_membership_test -> gh_group_membership
 *   short_weierstrass_projective.rs:227-268, algebra/src/bits.rs                   FromCompressedBits::decompress -> gh_points_decompress
 *   short_weierstrass_projective.rs:205-225                                        ToCompressedBits::compress -> gh_points_compress
 *   decompress / group_membership_test of A, B, C, then verify_proof               -> gh_groth16_verify_compressed / _checked
 *
 * A point is affine x || y in the ABI's Montgomery form (12 LE u64 limbs of x * 2^768 per Fq coefficient, as in ginger_hip.h)
 * plus an infinity byte: deg * 24 words with deg = 1 (G1), 2 (MNT4-753 G2, c0 || c1) or 3 (MNT6-753 G2, c0 || c1 || c2).  A
 * compressed point is the x coordinate as deg * 12 u64 CANONICAL little-endian limbs per row -- the integer read_bits builds
 * from the bits before from_repr, which may be at or above the modulus -- plus one flags byte: bit 0 infinity, bit 1 parity.
 * Parity is is_odd of the canonical y; for Fq2 and Fq3 that of the highest non-zero coefficient (fp2.rs:101-103,
 * fp3.rs:135-139).
 *
 * Compressed data is untrusted: what is wrong with it is a per-row status, never GH_E_BAD_ARG.  Montgomery-form points are
 * typed data as everywhere else: a coefficient at or above the modulus is GH_E_BAD_ARG, as are a null pointer, an unknown
 * curve and a key of another kind.  Status codes, gh_init / gh_last_error and the locking rules are those of ginger_hip.h;
 * n == 0 is a successful no-op; without a usable gfx950 device the compute entry points return GH_E_NO_DEVICE.
 *
 * Square roots (csrc/sqrt29.h): whether a root exists is the reference's answer, including its quirk in Fq2 (fp2.rs:188-190):
 * an element with c1 = 0 is rooted in Fq only, so x with x^3 + a x + b = (c0, 0), c0 a non-residue of Fq, is NotOnCurve
 * although a root exists in Fq2.  Every loop on the device has a fixed trip count: no input makes a row run longer.
 *
 * Subgroup membership: G1 has cofactor 1, so the curve equation decides and NotPrimeOrder cannot occur there.  On G2 the
 * device computes r P over the twist with a fixed signed-digit chain for r and complete group steps: the verdict of the
 * reference's mul_bits(r).is_zero() for every point of the curve, points of order 2 (y = 0) included.
 */
#ifndef GINGER_HIP_POINTS_H
#define GINGER_HIP_POINTS_H

#include "ginger_hip_pairing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-row codes of gh_points_decompress (BitSerializationError) and of out_point_status below */
#define GH_POINT_OK 0
#define GH_POINT_INVALID_FIELD_ELEMENT 1 /* a coefficient of x is at or above the modulus */
#define GH_POINT_INVALID_FLAGS 2         /* infinity together with parity or with x != 0, or a flag bit above bit 1 */
#define GH_POINT_NOT_ON_CURVE 3          /* x^3 + a x + b has no root as the reference sees it; for a Montgomery-form point: off the curve */
#define GH_POINT_NOT_PRIME_ORDER 4       /* on the curve, r P != infinity */
#define GH_FLAG_INFINITY 1
#define GH_FLAG_PARITY 2
/* row status of the two verifiers below, next to 1 / 0 / 2 of gh_groth16_verify: a proof point failed validation */
#define GH_VERIFY_INVALID_POINT 3

/* out_ok[i] = 1 iff point i is the point at infinity, or is on its curve and r P = infinity (group_membership_test). */
int gh_group_membership(gh_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_ok);
/* FromCompressedBits::decompress per row, the checks in the reference's order.  GH_POINT_OK: out_xy / out_inf hold the point
 * with is_odd(y) == parity, infinity as GroupAffine::zero() = (0, 1) with its byte set; any other status: the row is zero. */
int gh_points_decompress(gh_curve_t curve, const uint64_t* x, const uint8_t* flags, size_t n, uint64_t* out_xy, uint8_t* out_inf,
                         uint8_t* out_status);
/* ToCompressedBits::compress per row: canonical x (zero for the point at infinity) and the two flags. */
int gh_points_compress(gh_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_x, uint8_t* out_flags);
/* gh_groth16_verify after group_membership_test of A, B and C.  out_status[i]: 1 = Ok(true), 0 = Ok(false),
 * GH_VERIFY_INVALID_POINT = a proof point is not a member of its group (the row is not evaluated; status 2 cannot occur).
 * out_point_status: null, or n x 3 bytes, the GH_POINT_* code of A, B, C of each row. */
int gh_groth16_verify_checked(gh_groth16_vk_t h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                              const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs,
                              uint8_t* out_status, uint8_t* out_point_status);
/* The same for proofs in the wire form: A, B, C each as canonical x plus a flags byte, decompressed on the device (with the
 * subgroup test) and verified there.  out_point_status: the decompression code of A, B, C. */
int gh_groth16_verify_compressed(gh_groth16_vk_t h, const uint64_t* a_x, const uint8_t* a_flags, const uint64_t* b_x, const uint8_t* b_flags,
                                 const uint64_t* c_x, const uint8_t* c_flags, const uint64_t* inputs, size_t n, size_t n_inputs,
                                 uint8_t* out_status, uint8_t* out_point_status);
/* Of the last call of this header: milliseconds of its phases (upload, validate, download; for the two verifiers validate
 * only, their other phases are in gh_pairing_last_timing), *total_ms their sum or the whole call.  Returns the number of
 * entries written (at most max_phases) or a negative status. */
int gh_points_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
