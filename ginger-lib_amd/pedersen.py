"""Batched Pedersen hash and Pedersen commitment on the device (include/ginger_hip_pedersen.h), with the reference's names
(primitives/src/crh/pedersen/mod.rs, primitives/src/commitment/pedersen/mod.rs):

    PedersenCRH(curve, gen_xy, gen_inf, num_windows, window_size, table_bits=0)     generators[num_windows][window_size]
        .evaluate(inputs) -> (xy, inf)                   inputs: uint8 (n, nbytes), one input per row
        .evaluate_dev(d_in, n, nbytes, d_xy, d_inf)      the same over device buffers
        .input_size_bits                                 INPUT_SIZE_BITS = num_windows * window_size
    PedersenCommitment(curve, gen_xy, gen_inf, num_windows, window_size, rand_xy, rand_inf, table_bits=0)
        .commit(inputs, randomness) -> (xy, inf)         randomness: (n, 12), Montgomery form of the group's scalar field
        .commit_dev(d_in, n, nbytes, d_rand, d_xy, d_inf)
        .evaluate / .evaluate_dev                        the hash under the same generators
    generator_powers(curve, base, num_powers)            base, 2 base, 4 base, ...: the reference's generator_powers
    create_generators(curve, bases, window_size)         one window of powers per base: the reference's create_generators

The generators are taken as they are, flattened window-major; bit b of an input (the least significant bit of each byte
first) selects generator b.  A point is (xy: (n, 24), inf: (n,) uint8), field elements are rows of 12 u64 limbs of the
Montgomery form x * 2^768.  table_bits t in {1, 2, 4, 8} (0 = the library's default): the device table holds the 2^t - 1
subset sums of every t consecutive generators, one mixed addition per t input bits.
"""
import ctypes

import numpy as np

from . import GingerHipError, _check, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles
from ._handles import _bytes, _cid, _rows, ci, sz, vp

_ARGTYPES = {"gh_pedersen_create": [ci, vp, vp, sz, sz, vp, vp, sz, ci, _handles.OUT_HANDLE], "gh_pedersen_free": [vp],
             "gh_pedersen_hash": [vp, vp, sz, sz, vp, vp], "gh_pedersen_hash_dev": [vp, vp, sz, sz, vp, vp],
             "gh_pedersen_commit": [vp, vp, sz, sz, vp, vp, vp], "gh_pedersen_commit_dev": [vp, vp, sz, sz, vp, vp, vp],
             "gh_pedersen_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_pedersen.h declares (kept apart from every other header's list)
PEDERSEN_SYMBOLS = list(_ARGTYPES)
PHASES = ["upload", "hash", "normalise", "finish"]
_lib = _handles.binder("Pedersen", _ARGTYPES)


def last_timing():
    """({phase: milliseconds} of the last evaluate / commit, total milliseconds)"""
    ms, tot = _handles.last_timing(_lib().gh_pedersen_last_timing, len(PHASES))
    return dict(zip(PHASES, ms)), tot


def _dptr(b):
    return b.ptr if hasattr(b, "ptr") else ctypes.c_void_p(b)


def _inputs(data):
    d = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
    if d.ndim != 2:
        raise ValueError("input must have shape (n, nbytes)")
    return d


class PedersenCRH(_handles.Handle):
    """generators[num_windows][window_size] as window-major rows: gen_xy (num_windows * window_size, 24), gen_inf (same
    count) or None"""

    _lib, _prefix = staticmethod(_lib), "gh_pedersen"

    def __init__(self, curve, gen_xy, gen_inf, num_windows, window_size, table_bits=0, _rand=None):
        self.curve = curve
        self.num_windows, self.window_size = int(num_windows), int(window_size)
        xy = _rows(gen_xy, 24)
        inf = None if gen_inf is None else _bytes(gen_inf)
        if xy.shape[0] != self.num_windows * self.window_size or (inf is not None and inf.shape[0] != xy.shape[0]):
            raise ValueError("num_windows * window_size generators")
        rxy, rinf = (None, None) if _rand is None else _rand
        self._create(_cid(curve), _ptr(xy), None if inf is None else _ptr(inf), self.num_windows, self.window_size,
                     None if rxy is None else _ptr(rxy), None if rinf is None else _ptr(rinf), 0 if rxy is None else rxy.shape[0],
                     int(table_bits))

    @property
    def input_size_bits(self):
        return self.num_windows * self.window_size

    def _out(self, n):
        return np.zeros((n, 24), dtype=np.uint64), np.zeros(n, dtype=np.uint8)

    def evaluate(self, inputs):
        """inputs: uint8 (n, nbytes) -> (xy (n, 24), inf (n,))"""
        d = _inputs(inputs)
        n, nbytes = d.shape
        xy, inf = self._out(n)
        _check(_lib().gh_pedersen_hash(self.handle, _ptr(d), n, nbytes, _ptr(xy), _ptr(inf)))
        return xy, inf

    def evaluate_dev(self, d_in, n, nbytes, d_xy, d_inf):
        """device buffers (DeviceBuffer or raw pointers): n * nbytes input bytes -> n x 24 words and n infinity bytes"""
        _check(_lib().gh_pedersen_hash_dev(self.handle, _dptr(d_in), n, nbytes, _dptr(d_xy), _dptr(d_inf)))


class PedersenCommitment(PedersenCRH):
    """the hash's generators and the 753 randomness generators rand_xy (753, 24), rand_inf (753,) or None"""

    def __init__(self, curve, gen_xy, gen_inf, num_windows, window_size, rand_xy, rand_inf, table_bits=0):
        rxy = _rows(rand_xy, 24)
        rinf = None if rand_inf is None else _bytes(rand_inf)
        if rinf is not None and rinf.shape[0] != rxy.shape[0]:
            raise ValueError("one infinity byte per randomness generator")
        super().__init__(curve, gen_xy, gen_inf, num_windows, window_size, table_bits, _rand=(rxy, rinf))

    def commit(self, inputs, randomness):
        """inputs: uint8 (n, nbytes), randomness: (n, 12) -> (xy (n, 24), inf (n,))"""
        d = _inputs(inputs)
        n, nbytes = d.shape
        r = _rows(randomness, 12)
        if r.shape[0] != n:
            raise ValueError("one randomness per row")
        xy, inf = self._out(n)
        _check(_lib().gh_pedersen_commit(self.handle, _ptr(d), n, nbytes, _ptr(r), _ptr(xy), _ptr(inf)))
        return xy, inf

    def commit_dev(self, d_in, n, nbytes, d_rand, d_xy, d_inf):
        """as evaluate_dev, with n x 12 words of randomness on the device (kept below the modulus by the caller)"""
        _check(_lib().gh_pedersen_commit_dev(self.handle, _dptr(d_in), n, nbytes, _dptr(d_rand), _dptr(d_xy), _dptr(d_inf)))


def generator_powers(curve, base, num_powers):
    """(xy (num_powers, 24), inf (num_powers,)) of base, 2 base, 4 base, ...: generator_powers of the reference with its RNG
    draw as the argument.  The doublings are one gh_batch_mul with the scalars 2^k."""
    from . import proj_to_affine, schnorr
    num_powers = int(num_powers)
    if num_powers > 753:
        raise ValueError("at most 753 powers (gh_batch_mul takes scalars below 2^753)")
    b = _rows(base, 24)
    if b.shape[0] != 1:
        raise ValueError("one base (24 limbs)")
    k = np.zeros((num_powers, 12), dtype=np.uint64)
    for j in range(num_powers):
        k[j, j // 64] = np.uint64(1 << (j % 64))
    xyz = schnorr.batch_mul(curve, np.repeat(b, num_powers, axis=0), k)
    xy = np.zeros((num_powers, 24), dtype=np.uint64)
    inf = np.zeros(num_powers, dtype=np.uint8)
    for j in range(num_powers):
        xy[j], inf[j] = proj_to_affine(curve, xyz[j])
    return xy, inf


def create_generators(curve, bases, window_size):
    """(gen_xy (len(bases) * window_size, 24), gen_inf): window i holds the window_size powers of bases[i], window-major"""
    parts = [generator_powers(curve, b, window_size) for b in _rows(bases, 24)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
