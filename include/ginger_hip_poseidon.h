/* ginger_hip_poseidon.h -- C ABI of the device Poseidon hash and Poseidon Merkle tree over the MNT4-753 / MNT6-753 scalar
 * fields (T = 3, rate 2, S-box x -> x^-1), the second performance-sensitive workload of ginger-lib:
 *
 *   primitives/src/crh/poseidon/mod.rs:580-616      PoseidonHash::evaluate             -> gh_poseidon_hash(_dev)
 *   primitives/src/crh/poseidon/mod.rs:623-670      PoseidonBatchHash::batch_evaluate_2_1 -> gh_poseidon_hash, len 2
 *   primitives/src/merkle_tree/field_based_mht/mod.rs:126-195  FieldBasedMerkleHashTree::new -> gh_poseidon_merkle_tree
 *   primitives/src/merkle_tree/field_based_mht/mod.rs:64-96    FieldBasedMerkleTreePath::verify -> gh_poseidon_merkle_verify
 *
 * The library embeds no parameter set: the caller passes its own (P::ROUND_CST, P::MDS_CST, P::C2, P::AFTER_ZERO_PERM of
 * a PoseidonParameters impl).  Field elements are 12 little-endian u64 limbs of the Montgomery form x * 2^768, as in
 * ginger_hip.h; constants must be below the field's modulus.  Status codes, gh_field_t, gh_init / gh_last_error and the
 * locking rules are those of ginger_hip.h.  Without a usable gfx950 device the compute entry points return
 * GH_E_NO_DEVICE; n == 0 is a successful no-op.
 *
 * Batched evaluation computes the mathematical function, also where the reference's batched form does not: when a
 * partial round's batch product is zero, PoseidonBatchHash leaves the batch's last state un-inverted (mod.rs:245-251);
 * here every output equals PoseidonHash::evaluate of its input.
 */
#ifndef GINGER_HIP_POSEIDON_H
#define GINGER_HIP_POSEIDON_H

#include "ginger_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_poseidon* gh_poseidon_t;

/* A parameter set: r_f full rounds before and after r_p partial ones (r_f >= 1), round_cst >= 3 (2 r_f + r_p) elements
 * (the rest is ignored), mds9 row-major, c2 the capacity constant, after_zero_perm3 the permutation of (0, 0, 0).
 * GH_E_BAD_ARG: a null pointer, r_f == 0, too few constants, a constant not below the modulus.  Needs no device. */
int gh_poseidon_create(gh_field_t field, uint32_t r_f, uint32_t r_p, const uint64_t* round_cst, size_t n_round_cst,
                       const uint64_t* mds9, const uint64_t* c2, const uint64_t* after_zero_perm3, gh_poseidon_t* out);
int gh_poseidon_free(gh_poseidon_t h);

/* n states of 3 elements, permuted in place */
int gh_poseidon_permute(gh_poseidon_t h, uint64_t* states, size_t n);
/* out[i] = evaluate(in[i len .. (i + 1) len)) for i < n (len 0: AFTER_ZERO_PERM[0], no permutation) */
int gh_poseidon_hash(gh_poseidon_t h, const uint64_t* in, size_t n, size_t len, uint64_t* out);
/* the same on device buffers (gh_dev_alloc) */
int gh_poseidon_hash_dev(gh_poseidon_t h, const void* d_in, size_t n, size_t len, void* d_out);

/* FieldBasedMerkleHashTree::new(leaves) with HEIGHT = height: L = next_pow2(n_leaves) (1 for no leaf), missing leaves are
 * evaluate([1]); out_tree (nullable) receives the 2L - 1 nodes in heap order (root at 0, leaves from L - 1), out_padding
 * (nullable) the height - tree_height padding hashes, out_root the root.  GH_E_BAD_ARG if log2(L) + 1 > height.
 * The levels are built on the device with the leaves uploaded once; levels of at most host_tail_nodes nodes
 * (gh_poseidon_set_tuning) and, when that threshold is not 0, the padding chain are finished on the host with the same
 * permutation code on at most 16 threads ($OMP_NUM_THREADS if smaller). */
int gh_poseidon_merkle_tree(gh_poseidon_t h, const uint64_t* leaves, size_t n_leaves, uint32_t height, uint64_t* out_tree,
                            uint64_t* out_padding, uint64_t* out_root);
/* n paths of height - 1 (sibling, direction) steps each: siblings n (height - 1) elements, directions n (height - 1) bytes
 * (non-zero: the running hash is the RIGHT input, i.e. the path node is a right child).  out_ok[i] = 1 if path i leads
 * from leaves[i] to root, else 0.  GH_E_BAD_ARG for height < 2 (the reference rejects an empty path). */
int gh_poseidon_merkle_verify(gh_poseidon_t h, const uint64_t* leaves, const uint64_t* siblings, const uint8_t* directions,
                              size_t n, uint32_t height, const uint64_t* root, uint8_t* out_ok);

/* states_per_lane: K of the kernels (1, 2, 4 or 8; 0 = choose from the batch size); host_tail_nodes: the node count at or
 * below which a tree level goes to the host (0 = never, SIZE_MAX = the default).  Process-wide. */
int gh_poseidon_set_tuning(int states_per_lane, size_t host_tail_nodes);
/* Of the last gh_poseidon_merkle_tree: the time of every internal level, bottom-up (the level above the leaves first, the
 * root's last), then one entry for the whole padding chain; *total_ms the whole call.  Returns the number of entries
 * written (at most max_levels) or a negative status. */
int gh_poseidon_last_timing(float* level_ms, int max_levels, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
