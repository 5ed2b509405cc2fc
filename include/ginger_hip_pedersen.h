/* ginger_hip_pedersen.h -- C ABI of the batched Pedersen hash and the Pedersen commitment over the MNT4-753 / MNT6-753 G1
 * groups:
 *
 *   primitives/src/crh/pedersen/mod.rs:65-116          PedersenCRH::evaluate      -> gh_pedersen_hash
 *   primitives/src/commitment/pedersen/mod.rs:76-122   PedersenCommitment::commit -> gh_pedersen_commit
 *
 * generators[num_windows][window_size] are taken as they are (nothing assumes that one is the double of the one before it)
 * and flattened window-major into g_0 .. g_(G-1), G = num_windows * window_size.  The bits of an input are those of
 * bytes_to_bits: the least significant bit of each byte first.
 *
 *   evaluate(input)  = sum over b < 8 nbytes of bit_b g_b                 (zero padding changes nothing; the empty input
 *                                                                         hashes to the point at infinity)
 *   commit(input, r) = evaluate(input) + sum over k < 753 of bit_k(r) h_k  (h_k the 753 randomness generators, bit_k bit k of
 *                                                                         the canonical integer of r)
 *
 * 8 nbytes > G is GH_E_BAD_ARG for both (the reference panics).  Layout and conventions are those of ginger_hip_schnorr.h
 * and ginger_hip_ecvrf.h: field elements are 12 little-endian u64 limbs of the Montgomery form x * 2^768; a generator row is
 * affine x || y (24 words) with an optional infinity byte (NULL = none at infinity); randomness is n rows of 12 limbs in the
 * Montgomery form of the group's scalar field, as sk is there, and a row at or above the modulus is GH_E_BAD_ARG.  Outputs
 * are affine x || y rows plus an infinity byte; a sum at infinity is reported as gh_bh_hash reports it.  The reference's
 * projective coordinates depend on its addition order: parity is defined after into_affine().
 *
 * G2 curves are GH_E_UNSUPPORTED, as for gh_batch_double_mul.  n == 0 is a successful no-op; without a usable gfx950 device
 * the compute entry points return GH_E_NO_DEVICE.
 */
#ifndef GINGER_HIP_PEDERSEN_H
#define GINGER_HIP_PEDERSEN_H

#include "ginger_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_pedersen* gh_pedersen_t;

/* gen_xy: G rows, window-major; rand_xy: the 753 randomness generators (n_rand must be 753, the MODULUS_BITS of both scalar
 * fields), or NULL with n_rand == 0 for a handle that only hashes.  Every coordinate must be below the modulus and every
 * generator not flagged at infinity on the curve.  table_bits t in {1, 2, 4, 8}, 0 = the default (8): the device table
 * holds the 2^t - 1 subset sums of every group of t consecutive generators, so that a row costs one mixed addition per t
 * input bits (t = 1 is the literal bit loop).  Host only: the tables are built on first use. */
int gh_pedersen_create(gh_curve_t curve, const uint64_t* gen_xy, const uint8_t* gen_inf, size_t num_windows, size_t window_size,
                       const uint64_t* rand_xy, const uint8_t* rand_inf, size_t n_rand, int table_bits, gh_pedersen_t* out);
int gh_pedersen_free(gh_pedersen_t h);
/* out[i] = evaluate(input[i * nbytes .. (i + 1) * nbytes)): out_xy n x 24 words, out_inf n bytes */
int gh_pedersen_hash(gh_pedersen_t h, const uint8_t* input, size_t n, size_t nbytes, uint64_t* out_xy, uint8_t* out_inf);
/* the same with input and outputs in device memory, on the library's stream; returns when the outputs are written */
int gh_pedersen_hash_dev(gh_pedersen_t h, const void* d_input, size_t n, size_t nbytes, void* d_out_xy, void* d_out_inf);
/* out[i] = commit(input row i, randomness row i); GH_E_BAD_ARG for a handle made without randomness generators */
int gh_pedersen_commit(gh_pedersen_t h, const uint8_t* input, size_t n, size_t nbytes, const uint64_t* randomness, uint64_t* out_xy,
                       uint8_t* out_inf);
/* the same in device memory.  The randomness rows cannot be checked on the host: the caller keeps them below the modulus. */
int gh_pedersen_commit_dev(gh_pedersen_t h, const void* d_input, size_t n, size_t nbytes, const void* d_randomness, void* d_out_xy,
                           void* d_out_inf);
/* Of the last hash or commit: milliseconds of its phases (upload, hash with the conversion of the randomness, normalise,
 * finish with the download), *total_ms the whole call.  Returns the number of entries written (at most max_phases) or a
 * negative status. */
int gh_pedersen_last_timing(float* phase_ms, int max_phases, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
