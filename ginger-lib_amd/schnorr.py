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
import ctypes

import numpy as np

from . import CURVES, GingerHipError, _check, _ptr, _u64, load_library

# every symbol include/ginger_hip_schnorr.h declares (kept apart from ABI_SYMBOLS / DIST_SYMBOLS / POSEIDON_SYMBOLS)
SCHNORR_SYMBOLS = ["gh_schnorr_create", "gh_schnorr_free", "gh_schnorr_public_keys", "gh_schnorr_sign", "gh_schnorr_verify",
                   "gh_schnorr_keyverify", "gh_batch_mul", "gh_schnorr_last_timing"]
PHASES = ["upload", "fixed_base", "variable_base", "normalise", "hash", "finish"]
_bound = None


def _lib():
    global _bound
    lib = load_library()
    if _bound is lib:
        return lib
    missing = [s for s in SCHNORR_SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise GingerHipError("libginger_hip.so lacks Schnorr symbols: %s" % missing)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.gh_schnorr_create.argtypes = [ci, vp, ci, ctypes.POINTER(vp)]
    lib.gh_schnorr_free.argtypes = [vp]
    lib.gh_schnorr_public_keys.argtypes = [vp, vp, sz, vp, vp]
    lib.gh_schnorr_sign.argtypes = [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp]
    lib.gh_schnorr_verify.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp]
    lib.gh_schnorr_keyverify.argtypes = [vp, vp, vp, sz, vp]
    lib.gh_batch_mul.argtypes = [ci, vp, vp, vp, sz, vp]
    lib.gh_schnorr_last_timing.argtypes = [ctypes.POINTER(ctypes.c_float), ci, ctypes.POINTER(ctypes.c_float)]
    _bound = lib
    return lib


def _rows(a, words):
    a = _u64(a, words)
    return np.ascontiguousarray(a.reshape(-1, words))


def _msg(msg, n):
    m = np.ascontiguousarray(msg, dtype=np.uint64)
    if m.size == 0:
        return np.zeros((n, 0, 12), dtype=np.uint64)
    if m.ndim != 3 or m.shape[0] != n or m.shape[2] != 12:
        raise ValueError("messages must have shape (n, len, 12)")
    return m


def _pk(pk):
    xy, inf = pk
    xy = _rows(xy, 24)
    inf = np.ascontiguousarray(np.asarray(inf, dtype=np.uint8).reshape(-1))
    if inf.shape[0] != xy.shape[0]:
        raise ValueError("one infinity byte per public key")
    return xy, inf


def last_timing():
    """({phase: milliseconds} of the last sign / verify / batch_mul, total milliseconds); batch_mul records its variable_base
    phase only"""
    buf = (ctypes.c_float * len(PHASES))()
    tot = ctypes.c_float()
    n = _lib().gh_schnorr_last_timing(buf, len(PHASES), ctypes.byref(tot))
    if n < 0:
        _check(n)
    return {PHASES[i]: buf[i] for i in range(n)}, tot.value


def batch_mul(curve, xy, scalars, inf=None):
    """out[i] = scalars[i] * (xy[i], inf[i]) on a G1 curve: (n, 36) projective limbs, gh_proj_mul's layout.  Scalars are
    canonical 12-limb integers below 2^753."""
    cid = CURVES[curve] if isinstance(curve, str) else int(curve)
    xy = _rows(xy, 24)
    k = _rows(scalars, 12)
    n = xy.shape[0]
    if k.shape[0] != n:
        raise ValueError("one scalar per base")
    infa = None if inf is None else np.ascontiguousarray(np.asarray(inf, dtype=np.uint8).reshape(n))
    out = np.zeros((n, 36), dtype=np.uint64)
    _check(_lib().gh_batch_mul(cid, _ptr(xy), None if infa is None else _ptr(infa), _ptr(k), n, _ptr(out)))
    return out


class FieldBasedSchnorrSignatureScheme:
    def __init__(self, params, curve, window=0):
        self.params = params                     # kept alive: the handle uses its hash
        self.curve = curve
        cid = CURVES[curve] if isinstance(curve, str) else int(curve)
        h = ctypes.c_void_p()
        _check(_lib().gh_schnorr_create(cid, params.handle, int(window), ctypes.byref(h)))
        self.handle = h

    def keygen_from(self, sk):
        """(pk, sk) of keygen for the given secrets: pk = sk G"""
        return self.get_public_key(sk), sk

    def get_public_key(self, sk):
        sk = _rows(sk, 12)
        n = sk.shape[0]
        xy = np.zeros((n, 24), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        _check(_lib().gh_schnorr_public_keys(self.handle, _ptr(sk), n, _ptr(xy), _ptr(inf)))
        return xy, inf

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

    def keyverify(self, pk):
        xy, inf = _pk(pk)
        ok = np.zeros(xy.shape[0], dtype=np.uint8)
        _check(_lib().gh_schnorr_keyverify(self.handle, _ptr(xy), _ptr(inf), xy.shape[0], _ptr(ok)))
        return ok.astype(bool)

    def batch_mul(self, xy, scalars, inf=None):
        return batch_mul(self.curve, xy, scalars, inf)

    def close(self):
        if getattr(self, "handle", None):
            _lib().gh_schnorr_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
