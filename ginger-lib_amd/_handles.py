"""What the handle wrappers of poseidon.py, schnorr.py and ecvrf.py share: binding a header's symbols once per loaded library,
reading a *_last_timing, the row layouts of their arguments, and the life cycle of a handle."""
import ctypes

import numpy as np

from . import CURVES, GingerHipError, _check, _ptr, _u64, load_library

vp, sz, ci, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
OUT_HANDLE = ctypes.POINTER(vp)
TIMING = [ctypes.POINTER(ctypes.c_float), ci, ctypes.POINTER(ctypes.c_float)]   # every gh_*_last_timing


def binder(what, argtypes):
    """-> _lib(): the loaded library with the argument types of `argtypes` ({symbol: [types]}) set, once per load; a symbol
    the library lacks is an error that names `what`"""
    bound = []

    def _lib():
        lib = load_library()
        if bound and bound[0] is lib:
            return lib
        missing = [s for s in argtypes if not hasattr(lib, s)]
        if missing:
            raise GingerHipError("libginger_hip.so lacks %s symbols: %s" % (what, missing))
        for name, types in argtypes.items():
            getattr(lib, name).argtypes = types
        bound[:] = [lib]
        return lib
    return _lib


def last_timing(fn, count):
    """(the first `count` phase times of a gh_*_last_timing in milliseconds, total milliseconds)"""
    buf = (ctypes.c_float * count)()
    tot = ctypes.c_float()
    n = fn(buf, count, ctypes.byref(tot))
    if n < 0:
        _check(n)
    return [buf[i] for i in range(n)], tot.value


def _cid(curve):
    return CURVES[curve] if isinstance(curve, str) else int(curve)


def _rows(a, words=12):
    a = _u64(a, words)
    return np.ascontiguousarray(a.reshape(-1, words))


def _bytes(a, n=-1):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint8).reshape(n))


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
    inf = _bytes(inf)
    if inf.shape[0] != xy.shape[0]:
        raise ValueError("one infinity byte per public key")
    return xy, inf


class Handle:
    """Owns self.handle.  A subclass sets _lib (its module's binder, as a staticmethod) and _prefix: its entry points are
    <_prefix>_<name>, <_prefix>_free among them."""
    handle = None

    def _fn(self, name):
        return getattr(self._lib(), "%s_%s" % (self._prefix, name))

    def _create(self, *args):
        h = vp()
        _check(self._fn("create")(*args, ctypes.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            self._fn("free")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeyOps:
    """The key functions a signature scheme and the VRF share, for a Handle over a group with <_prefix>_public_keys and
    <_prefix>_keyverify"""

    def keygen_from(self, sk):
        """(pk, sk) of keygen for the given secrets: pk = sk G"""
        return self.get_public_key(sk), sk

    def get_public_key(self, sk):
        sk = _rows(sk, 12)
        n = sk.shape[0]
        xy = np.zeros((n, 24), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        _check(self._fn("public_keys")(self.handle, _ptr(sk), n, _ptr(xy), _ptr(inf)))
        return xy, inf

    def keyverify(self, pk):
        xy, inf = _pk(pk)
        ok = np.zeros(xy.shape[0], dtype=np.uint8)
        _check(self._fn("keyverify")(self.handle, _ptr(xy), _ptr(inf), xy.shape[0], _ptr(ok)))
        return ok.astype(bool)
