"""Batched field-based Schnorr signatures on the device (include/ginger_hip_schnorr.h), with the reference's names
(primitives/src/signature/schnorr/field_based_schnorr.rs):

    FieldBasedSchnorrSignatureScheme(params, curve)      params: a poseidon.PoseidonParameters over the curve's base field
        .keygen_from(sk) -> (pk_xy, pk_inf)              keygen with the caller's secrets (sk G)
        .get_public_key(sk) -> (pk_xy, pk_inf)           :65-67
        .sign(sk, pk, msg, nonces) -> (sig, status)      :69-127, one nonce per row; status 0 = the reference would draw again
        .verify(pk, msg, sig) -> status                  :129-170; 1 Ok(true), 0 Ok(false), 2 Err
        .keyverify(pk) -> bool array                     :173-176
    batch_mul(curve, xy, scalars, inf=None) -> xyz       k_i P_i, one base per row

SchnorrMNT4 is FieldBasedSchnorrSignatureScheme(PoseidonParameters over "mnt4753_fr", "mnt6753_g1"), SchnorrMNT6 the same
over "mnt6753_fr" with "mnt4753_g1".  Field elements are rows of 12 u64 limbs of the Montgomery form x * 2^768 (numpy uint64);
secrets and nonces are in the Montgomery form of the group's scalar field; a public key is (xy: (n, 24), inf: (n,) uint8);
a signature row is e || s (24 limbs); messages have shape (n, len, 12) with one len per call.
"""
import numpy as np

from . import GingerHipError, _check, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles
from ._handles import _cid, _msg, _pk, _rows, ci, sz, vp

_ARGTYPES = {"gh_schnorr_create": [ci, vp, ci, _handles.OUT_HANDLE], "gh_schnorr_free": [vp],
             "gh_schnorr_public_keys": [vp, vp, sz, vp, vp], "gh_schnorr_sign": [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp],
             "gh_schnorr_verify": [vp, vp, vp, vp, sz, sz, vp, vp], "gh_schnorr_keyverify": [vp, vp, vp, sz, vp],
             "gh_batch_mul": [ci, vp, vp, vp, sz, vp], "gh_schnorr_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_schnorr.h declares (kept apart from ABI_SYMBOLS / DIST_SYMBOLS / POSEIDON_SYMBOLS)
SCHNORR_SYMBOLS = list(_ARGTYPES)
PHASES = ["upload", "fixed_base", "variable_base", "normalise", "hash", "finish"]
_lib = _handles.binder("Schnorr", _ARGTYPES)


def last_timing():
    """({phase: milliseconds} of the last sign / verify / batch_mul, total milliseconds); batch_mul records its variable_base
    phase only"""
    ms, tot = _handles.last_timing(_lib().gh_schnorr_last_timing, len(PHASES))
    return dict(zip(PHASES, ms)), tot


def batch_mul(curve, xy, scalars, inf=None):
    """out[i] = scalars[i] * (xy[i], inf[i]) on a G1 curve: (n, 36) projective limbs, gh_proj_mul's layout.  Scalars are
    canonical 12-limb integers below 2^753."""
    xy = _rows(xy, 24)
    k = _rows(scalars, 12)
    n = xy.shape[0]
    if k.shape[0] != n:
        raise ValueError("one scalar per base")
    infa = None if inf is None else _handles._bytes(inf, n)
    out = np.zeros((n, 36), dtype=np.uint64)
    _check(_lib().gh_batch_mul(_cid(curve), _ptr(xy), None if infa is None else _ptr(infa), _ptr(k), n, _ptr(out)))
    return out


class FieldBasedSchnorrSignatureScheme(_handles.KeyOps, _handles.Handle):
    _lib, _prefix = staticmethod(_lib), "gh_schnorr"

    def __init__(self, params, curve, window=0):
        self.params = params                     # kept alive: the handle uses its hash
        self.curve = curve
        self._create(_cid(curve), params.handle, int(window))

    def sign(self, sk, pk, msg, nonces):
        """-> (sig (n, 24), status (n,) uint8): 1 signed, 0 the nonce was rejected (its row is zero)"""
        sk = _rows(sk, 12)
        n = sk.shape[0]
        xy, inf = _pk(pk)
        m = _msg(msg, n)
        k = _rows(nonces, 12)
        if xy.shape[0] != n or k.shape[0] != n:
            raise ValueError("one key and one nonce per row")
        sig = np.zeros((n, 24), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        _check(_lib().gh_schnorr_sign(self.handle, _ptr(sk), _ptr(xy), _ptr(inf), _ptr(m), n, m.shape[1], _ptr(k), _ptr(sig), _ptr(st)))
        return sig, st

    def verify(self, pk, msg, sig):
        """-> status (n,) uint8: 1 = Ok(true), 0 = Ok(false), 2 = Err (e or s >= 2^752)"""
        xy, inf = _pk(pk)
        n = xy.shape[0]
        m = _msg(msg, n)
        s = _rows(sig, 24)
        if s.shape[0] != n:
            raise ValueError("one signature per key")
        st = np.zeros(n, dtype=np.uint8)
        _check(_lib().gh_schnorr_verify(self.handle, _ptr(xy), _ptr(inf), _ptr(m), n, m.shape[1], _ptr(s), _ptr(st)))
        return st

    def batch_mul(self, xy, scalars, inf=None):
        return batch_mul(self.curve, xy, scalars, inf)
