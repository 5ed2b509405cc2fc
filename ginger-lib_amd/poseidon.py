"""Poseidon hash and Poseidon Merkle tree on the device (include/ginger_hip_poseidon.h), with the reference's names:

    PoseidonParameters(field, r_f, r_p, round_cst, mds, c2, after_zero_perm)  /  PoseidonParameters.from_json(obj, tag)
    PoseidonHash(params).evaluate(x) / .evaluate_many(inputs)                 primitives/src/crh/poseidon/mod.rs:580-616
    PoseidonBatchHash(params).batch_evaluate_2_1(array)                      primitives/src/crh/poseidon/mod.rs:623-670
    FieldBasedMerkleHashTree(params, height, leaves).root() / leaves() / generate_proof(i, leaf)
    FieldBasedMerkleTreePath.verify(params, root, leaf), verify_paths(...)   primitives/src/merkle_tree/field_based_mht/mod.rs

Field elements are rows of 12 u64 limbs of the Montgomery form x * 2^768 (numpy uint64 arrays of shape (n, 12)), the
reference's in-memory form.  The parameter set is data the caller provides (for the reference's two sets: a JSON as
PoseidonParameters.from_json reads it); the library embeds none.
"""
import ctypes
import json

import numpy as np

from . import FIELDS, GingerHipError, _check, _ptr, _u64    # noqa: F401 (GingerHipError: re-exported)
from . import _handles
from ._handles import _rows, ci, sz, u32, vp

_ARGTYPES = {"gh_poseidon_create": [ci, u32, u32, vp, sz, vp, vp, vp, _handles.OUT_HANDLE], "gh_poseidon_free": [vp],
             "gh_poseidon_permute": [vp, vp, sz], "gh_poseidon_hash": [vp, vp, sz, sz, vp], "gh_poseidon_hash_dev": [vp, vp, sz, sz, vp],
             "gh_poseidon_merkle_tree": [vp, vp, sz, u32, vp, vp, vp], "gh_poseidon_merkle_verify": [vp, vp, vp, vp, sz, u32, vp, vp],
             "gh_poseidon_set_tuning": [ci, sz], "gh_poseidon_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_poseidon.h declares (kept apart from ABI_SYMBOLS / DIST_SYMBOLS)
POSEIDON_SYMBOLS = list(_ARGTYPES)
SIZE_MAX = (1 << 64) - 1
_lib = _handles.binder("Poseidon", _ARGTYPES)


def _hex_rows(vals):
    return np.array([[(int(h, 16) >> (64 * i)) & ((1 << 64) - 1) for i in range(12)] for h in vals], dtype=np.uint64).reshape(-1, 12)


def set_tuning(states_per_lane=0, host_tail_nodes=None):
    """K of the kernels (1, 2, 4, 8; 0 = automatic) and the node count at or below which tree levels go to the host
    (0 = never, None = the library default)."""
    _check(_lib().gh_poseidon_set_tuning(int(states_per_lane), SIZE_MAX if host_tail_nodes is None else int(host_tail_nodes)))


def last_timing(max_levels=64):
    """(per-level milliseconds of the last tree build, bottom-up, then the padding chain; total milliseconds)."""
    return _handles.last_timing(_lib().gh_poseidon_last_timing, max_levels)


class PoseidonParameters(_handles.Handle):
    """One parameter set (T = 3, rate 2); the handle holds its constants in the device's internal form."""
    _lib, _prefix = staticmethod(_lib), "gh_poseidon"

    def __init__(self, field, r_f, r_p, round_cst, mds, c2, after_zero_perm):
        self.field = field
        self.field_id = FIELDS[field] if isinstance(field, str) else int(field)
        self.r_f, self.r_p = int(r_f), int(r_p)
        self.round_cst = _rows(round_cst)
        self.mds = _rows(mds)
        self.c2 = _rows(c2)
        self.after_zero_perm = _rows(after_zero_perm)
        if self.mds.shape[0] != 9 or self.c2.shape[0] != 1 or self.after_zero_perm.shape[0] != 3:
            raise ValueError("mds needs 9 elements, c2 one, after_zero_perm three")
        self._create(self.field_id, self.r_f, self.r_p, _ptr(self.round_cst), self.round_cst.shape[0], _ptr(self.mds), _ptr(self.c2),
                     _ptr(self.after_zero_perm))

    @classmethod
    def from_json(cls, obj, tag):
        """obj: a path or a parsed dict of the shape {tag: {field, r_f, r_p, round_cst, mds, c2, after_zero_perm}} with the
        elements as hex integers of their 12-limb Montgomery words."""
        if isinstance(obj, str):
            with open(obj) as f:
                obj = json.load(f)
        d = obj[tag]
        return cls(d["field"], d["r_f"], d["r_p"], _hex_rows(d["round_cst"]), _hex_rows(d["mds"]), _hex_rows([d["c2"]]),
                   _hex_rows(d["after_zero_perm"]))

    def permute(self, states):
        """states: (n, 3, 12) or (3 n, 12) u64 -> permuted copy of the same shape"""
        st = np.array(states, dtype=np.uint64, copy=True, order="C")
        if st.size % 36:
            raise ValueError("states must be whole triples of elements")
        _check(_lib().gh_poseidon_permute(self.handle, _ptr(st), st.size // 36))
        return st


class PoseidonHash:
    def __init__(self, params):
        self.params = params

    def evaluate(self, inp):
        """one input of any length (rows of 12 limbs) -> digest (12 limbs)"""
        a = _rows(inp) if np.asarray(inp).size else np.zeros((0, 12), dtype=np.uint64)
        return self.evaluate_many(a.reshape(1, -1, 12))[0]

    def evaluate_many(self, inputs):
        """inputs: (n, len, 12) -> (n, 12): n independent evaluate() calls of len elements each"""
        a = np.ascontiguousarray(inputs, dtype=np.uint64)
        if a.ndim != 3 or a.shape[2] != 12:
            raise ValueError("inputs must have shape (n, len, 12)")
        n, ln = a.shape[0], a.shape[1]
        out = np.zeros((n, 12), dtype=np.uint64)
        _check(_lib().gh_poseidon_hash(self.params.handle, _ptr(a), n, ln, _ptr(out)))
        return out

    def evaluate_dev(self, d_in, n, length, d_out):
        """device buffers (DeviceBuffer.ptr or raw pointers) of n * length and n elements"""
        ptr = lambda b: b.ptr if hasattr(b, "ptr") else ctypes.c_void_p(b)
        _check(_lib().gh_poseidon_hash_dev(self.params.handle, ptr(d_in), n, length, ptr(d_out)))


class PoseidonBatchHash:
    def __init__(self, params):
        self.params = params

    def batch_evaluate_2_1(self, input_array):
        """In place, as the reference: the first half of input_array (2 n rows) receives the n digests of its pairs.
        Every digest is evaluate([a, b]) (the reference's zero-product quirk of mod.rs:245-251 is not reproduced)."""
        a = input_array
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags.c_contiguous and a.ndim == 2 and a.shape[1] == 12):
            raise ValueError("input_array must be a C-contiguous (2 n, 12) uint64 array")
        if a.shape[0] == 0 or a.shape[0] % 2:
            raise ValueError("the input must hold a non-zero, even number of elements")
        n = a.shape[0] // 2
        out = np.zeros((n, 12), dtype=np.uint64)
        _check(_lib().gh_poseidon_hash(self.params.handle, _ptr(a), n, 2, _ptr(out)))
        a[:n] = out
        return a


class FieldBasedMerkleTreePath:
    """height - 1 steps (sibling, direction); direction True: the running hash is the right input."""

    def __init__(self, siblings, directions):
        self.siblings = _rows(siblings)
        self.directions = np.asarray(directions, dtype=np.uint8)

    def verify(self, params, root, leaf):
        return bool(verify_paths(params, [leaf], [self], root)[0])


def verify_paths(params, leaves, paths, root):
    """batched FieldBasedMerkleTreePath::verify: -> bool array, one per (leaf, path)"""
    n = len(paths)
    if n == 0:
        return np.zeros(0, dtype=bool)
    steps = paths[0].siblings.shape[0]
    if any(p.siblings.shape[0] != steps or p.directions.shape[0] != steps for p in paths):
        raise ValueError("paths of different lengths")
    sib = np.ascontiguousarray(np.stack([p.siblings for p in paths]), dtype=np.uint64)
    dirs = np.ascontiguousarray(np.stack([p.directions for p in paths]), dtype=np.uint8)
    lv = np.ascontiguousarray(np.asarray(leaves, dtype=np.uint64).reshape(n, 12))
    rt = _u64(root).reshape(12)
    ok = np.zeros(n, dtype=np.uint8)
    _check(_lib().gh_poseidon_merkle_verify(params.handle, _ptr(lv), _ptr(sib), _ptr(dirs), n, steps + 1, _ptr(rt), _ptr(ok)))
    return ok.astype(bool)


class FieldBasedMerkleHashTree:
    """FieldBasedMerkleHashTree::new(leaves) of a config with HEIGHT = height, built on the device."""

    def __init__(self, params, height, leaves):
        self.params = params
        self.height = int(height)
        lv = np.ascontiguousarray(np.asarray(leaves, dtype=np.uint64).reshape(-1, 12))
        n = lv.shape[0]
        L = 1
        while L < n:
            L *= 2
        self.tree_height = L.bit_length()
        self.tree = np.zeros((2 * L - 1, 12), dtype=np.uint64)
        self.padding = np.zeros((max(self.height - self.tree_height, 0), 12), dtype=np.uint64)
        self._root = np.zeros(12, dtype=np.uint64)
        _check(_lib().gh_poseidon_merkle_tree(params.handle, _ptr(lv), n, self.height, _ptr(self.tree), _ptr(self.padding),
                                              _ptr(self._root)))

    def root(self):
        return self._root.copy()

    def leaves(self):
        return self.tree[(self.tree.shape[0] + 1) // 2 - 1:]

    def generate_proof(self, index, leaf):
        L = (self.tree.shape[0] + 1) // 2
        i = L - 1 + int(index)
        if i >= self.tree.shape[0] or not np.array_equal(self.tree[i], np.asarray(leaf, dtype=np.uint64).reshape(12)):
            raise ValueError("leaf does not match the tree at index %d" % index)
        sib, dirs = [], []
        while i > 0:
            right = i % 2 == 0
            sib.append(self.tree[i - 1] if right else self.tree[i + 1])
            dirs.append(right)
            i = (i - 1) // 2
        empty = self._empty()
        for _ in range(self.padding.shape[0]):
            sib.append(empty)
            dirs.append(False)
        if len(sib) != self.height - 1:
            raise ValueError("path length %d != height - 1" % len(sib))
        return FieldBasedMerkleTreePath(np.array(sib, dtype=np.uint64).reshape(-1, 12), dirs)

    def _empty(self):
        if not hasattr(self.params, "_empty"):
            # evaluate([1]) is the only node of the tree of no leaf
            self.params._empty = FieldBasedMerkleHashTree(self.params, 1, []).tree[0]
        return self.params._empty
