"""Batched field-based EC-VRF on the device (include/ginger_hip_ecvrf.h), with the reference's names
(primitives/src/vrf/ecvrf/mod.rs, primitives/src/crh/bowe_hopwood/mod.rs):

    BoweHopwoodPedersenCRH(curve, gen_xy, gen_inf, num_windows, window_size)   the group hash's parameters (segment-major)
        .evaluate(input) -> (xy, inf)                    input: uint8 (n, nbytes), one message per row
    FieldBasedEcVrf(params, bh, curve)                   params: a poseidon.PoseidonParameters over the curve's base field
        .get_public_key(sk) -> (pk_xy, pk_inf)           :77-79
        .prove(sk, pk, msg, nonces) -> (gamma, cs, status)   :81-158, one nonce per row; status 0 = the reference would draw again
        .proof_to_hash(pk, msg, gamma, cs) -> (out, status)  :160-237; 1 Ok, 0 FailedVerification, 2 c or s >= 2^752, 3 gamma off the curve
        .keyverify(pk) -> bool array
    batch_double_mul(curve, xy1, k1, xy2, k2, inf1=None, inf2=None) -> xyz    k1_i P1_i + k2_i P2_i, two bases per row

EcVrfMNT4 is FieldBasedEcVrf(PoseidonParameters over "mnt4753_fr", BoweHopwoodPedersenCRH over "mnt6753_g1", "mnt6753_g1"),
EcVrfMNT6 the same over "mnt6753_fr" with "mnt4753_g1".  Layouts are schnorr.py's: field elements are rows of 12 u64 limbs of
the Montgomery form x * 2^768; secrets and nonces are in the Montgomery form of the group's scalar field; a point is
(xy: (n, 24), inf: (n,) uint8); gamma is such a point and cs the rows c || s (24 limbs); messages have shape (n, len, 12).
"""
import numpy as np

from . import GingerHipError, _check, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles
from ._handles import _bytes, _cid, _msg, _pk, _rows, ci, sz, vp

_ARGTYPES = {"gh_bh_create": [ci, vp, vp, sz, sz, _handles.OUT_HANDLE], "gh_bh_free": [vp], "gh_bh_hash": [vp, vp, sz, sz, vp, vp],
             "gh_batch_double_mul": [ci, vp, vp, vp, vp, vp, vp, sz, vp], "gh_ecvrf_create": [ci, vp, vp, ci, _handles.OUT_HANDLE],
             "gh_ecvrf_free": [vp], "gh_ecvrf_public_keys": [vp, vp, sz, vp, vp],
             "gh_ecvrf_prove": [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, vp],
             "gh_ecvrf_proof_to_hash": [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, vp], "gh_ecvrf_keyverify": [vp, vp, vp, sz, vp],
             "gh_ecvrf_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_ecvrf.h declares (kept apart from the ABI / dist / Poseidon / Schnorr lists)
ECVRF_SYMBOLS = list(_ARGTYPES)
PHASES = ["upload", "group_hash", "fixed_base", "variable_base", "normalise", "hash", "finish"]
_lib = _handles.binder("EC-VRF", _ARGTYPES)


def last_timing():
    """({phase: milliseconds} of the last prove / proof_to_hash / evaluate / batch_double_mul, total milliseconds); evaluate
    records its group_hash phase only, batch_double_mul its variable_base phase only"""
    ms, tot = _handles.last_timing(_lib().gh_ecvrf_last_timing, len(PHASES))
    return dict(zip(PHASES, ms)), tot


def batch_double_mul(curve, xy1, k1, xy2, k2, inf1=None, inf2=None):
    """out[i] = k1[i] (xy1[i], inf1[i]) + k2[i] (xy2[i], inf2[i]) on a G1 curve: (n, 36) projective limbs, gh_proj_mul's
    layout.  Scalars are canonical 12-limb integers below 2^753."""
    xy1, xy2 = _rows(xy1, 24), _rows(xy2, 24)
    k1, k2 = _rows(k1, 12), _rows(k2, 12)
    n = xy1.shape[0]
    if xy2.shape[0] != n or k1.shape[0] != n or k2.shape[0] != n:
        raise ValueError("two bases and two scalars per row")
    infs = [None if f is None else _bytes(f, n) for f in (inf1, inf2)]
    out = np.zeros((n, 36), dtype=np.uint64)
    p = [None if f is None else _ptr(f) for f in infs]
    _check(_lib().gh_batch_double_mul(_cid(curve), _ptr(xy1), p[0], _ptr(k1), _ptr(xy2), p[1], _ptr(k2), n, _ptr(out)))
    return out


class BoweHopwoodPedersenCRH(_handles.Handle):
    """generators[num_windows][window_size] as segment-major rows: gen_xy (num_windows * window_size, 24), gen_inf (same
    count) or None"""

    _lib, _prefix = staticmethod(_lib), "gh_bh"

    def __init__(self, curve, gen_xy, gen_inf, num_windows, window_size):
        self.curve = curve
        self.num_windows, self.window_size = int(num_windows), int(window_size)
        xy = _rows(gen_xy, 24)
        inf = None if gen_inf is None else _bytes(gen_inf)
        if xy.shape[0] != self.num_windows * self.window_size or (inf is not None and inf.shape[0] != xy.shape[0]):
            raise ValueError("num_windows * window_size generators")
        self._create(_cid(curve), _ptr(xy), None if inf is None else _ptr(inf), self.num_windows, self.window_size)

    def evaluate(self, data):
        """data: uint8 (n, nbytes) -> (xy (n, 24), inf (n,))"""
        d = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
        if d.ndim != 2:
            raise ValueError("input must have shape (n, nbytes)")
        n, nbytes = d.shape
        xy = np.zeros((n, 24), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        _check(_lib().gh_bh_hash(self.handle, _ptr(d), n, nbytes, _ptr(xy), _ptr(inf)))
        return xy, inf


class FieldBasedEcVrf(_handles.KeyOps, _handles.Handle):
    _lib, _prefix = staticmethod(_lib), "gh_ecvrf"

    def __init__(self, params, bh, curve, window=0):
        self.params, self.bh = params, bh        # kept alive: the handle uses both
        self.curve = curve
        self._create(_cid(curve), params.handle, bh.handle, int(window))

    def prove(self, sk, pk, msg, nonces):
        """-> ((gamma_xy, gamma_inf), cs (n, 24), status (n,) uint8): 1 proved, 0 the nonce was rejected (its cs row is zero)"""
        sk = _rows(sk, 12)
        n = sk.shape[0]
        xy, inf = _pk(pk)
        m = _msg(msg, n)
        k = _rows(nonces, 12)
        if xy.shape[0] != n or k.shape[0] != n:
            raise ValueError("one key and one nonce per row")
        gxy = np.zeros((n, 24), dtype=np.uint64)
        ginf = np.zeros(n, dtype=np.uint8)
        cs = np.zeros((n, 24), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(_lib().gh_ecvrf_prove(self.handle, _ptr(sk), _ptr(xy), _ptr(inf), _ptr(m), n, m.shape[1], _ptr(k), _ptr(gxy), _ptr(ginf),
                                     _ptr(cs), _ptr(st)))
        return (gxy, ginf), cs, st

    def proof_to_hash(self, pk, msg, gamma, cs):
        """-> (output (n, 12), status (n,) uint8): 1 = Ok(output), 0 = FailedVerification, 2 = c or s >= 2^752, 3 = gamma not
        on the curve; output rows are zero unless the status is 1"""
        xy, inf = _pk(pk)
        n = xy.shape[0]
        m = _msg(msg, n)
        gxy, ginf = _pk(gamma)
        c = _rows(cs, 24)
        if gxy.shape[0] != n or c.shape[0] != n:
            raise ValueError("one proof per key")
        out = np.zeros((n, 12), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(_lib().gh_ecvrf_proof_to_hash(self.handle, _ptr(xy), _ptr(inf), _ptr(m), n, m.shape[1], _ptr(gxy), _ptr(ginf), _ptr(c),
                                             _ptr(out), _ptr(st)))
        return out, st
