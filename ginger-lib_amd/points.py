"""Batched point validation and the compressed wire form of a point on the device (include/ginger_hip_points.h), with the
reference's names (algebra/src/curves/models/short_weierstrass_projective.rs:106-121, :205-268):

    group_membership_test(curve, points) -> (n,) bool    on the curve and r P = infinity (or the point at infinity)
    compress(curve, points) -> (n, deg * 753 + 2) uint8  ToCompressedBits::compress as the reference's Vec<bool>
    decompress(curve, bitvecs) -> (points, status)       FromCompressedBits::decompress per row
    compress_limbs / decompress_limbs                    the same on the C ABI's form of a compressed point
    pairing.PreparedVerifyingKey.verify_checked / .verify_compressed      Groth16 verification of validated proofs

A batch of points is (xy: (n, 24 deg), inf: (n,) uint8): rows of 12 u64 limbs of the Montgomery form x * 2^768 per Fq
coefficient, x || y, deg = 1 (G1), 2 (MNT4-753 G2) or 3 (MNT6-753 G2).  A compressed point in the ABI's form is
(x: (n, 12 deg) canonical little-endian limbs, flags: (n,) uint8, bit 0 infinity, bit 1 parity).  A bit vector holds, per
coefficient, 753 bits, most significant first, c0 || c1 || c2, then the infinity bit, then the parity bit.  Status per row
(BitSerializationError): 0 Ok, 1 InvalidFieldElement, 2 InvalidFlags, 3 NotOnCurve, 4 NotPrimeOrder; a failed row is zero."""
import numpy as np

from . import CURVE_DEG, GingerHipError, _check, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles
from ._handles import _bytes, _cid, _rows, ci, sz, vp

_ARGTYPES = {"gh_group_membership": [ci, vp, vp, sz, vp],
             "gh_points_decompress": [ci, vp, vp, sz, vp, vp, vp],
             "gh_points_compress": [ci, vp, vp, sz, vp, vp],
             "gh_groth16_verify_checked": [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, vp, vp],
             "gh_groth16_verify_compressed": [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, vp, vp],
             "gh_points_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_points.h declares
POINTS_SYMBOLS = list(_ARGTYPES)
PHASES = ["upload", "validate", "download"]
OK, INVALID_FIELD_ELEMENT, INVALID_FLAGS, NOT_ON_CURVE, NOT_PRIME_ORDER = range(5)
FLAG_INFINITY, FLAG_PARITY = 1, 2
VERIFY_INVALID_POINT = 3
MODULUS_BITS = 753
_lib = _handles.binder("points", _ARGTYPES)
_DEG = {cid: CURVE_DEG[name] for name, cid in _handles.CURVES.items()}


def last_timing():
    """({phase: milliseconds} of the last call of this module, total milliseconds); after verify_checked / verify_compressed
    the validate phase alone (their other phases: pairing.last_timing)"""
    ms, tot = _handles.last_timing(_lib().gh_points_last_timing, len(PHASES))
    return dict(zip(PHASES, ms)), tot


def _deg(curve):
    cid = _cid(curve)
    if cid not in _DEG:
        raise ValueError("unknown curve")
    return cid, _DEG[cid]


def _points(pts, words):
    xy, inf = pts
    xy = _rows(xy, words)
    inf = _bytes(inf)
    if inf.shape[0] != xy.shape[0]:
        raise ValueError("one infinity byte per point")
    return xy, inf


def group_membership_test(curve, points):
    cid, deg = _deg(curve)
    xy, inf = _points(points, 24 * deg)
    ok = np.zeros(xy.shape[0], dtype=np.uint8)
    _check(_lib().gh_group_membership(cid, _ptr(xy), _ptr(inf), xy.shape[0], _ptr(ok)))
    return ok.astype(bool)


def compress_limbs(curve, points):
    """-> (x: (n, 12 deg) canonical limbs, zero for the point at infinity; flags: (n,) uint8)"""
    cid, deg = _deg(curve)
    xy, inf = _points(points, 24 * deg)
    n = xy.shape[0]
    x = np.zeros((n, 12 * deg), dtype=np.uint64)
    flags = np.zeros(n, dtype=np.uint8)
    _check(_lib().gh_points_compress(cid, _ptr(xy), _ptr(inf), n, _ptr(x), _ptr(flags)))
    return x, flags


def decompress_limbs(curve, x, flags):
    """-> ((xy, inf), status); infinity comes out as (0, 1) with its byte set"""
    cid, deg = _deg(curve)
    x = _rows(x, 12 * deg)
    flags = _bytes(flags)
    n = x.shape[0]
    if flags.shape[0] != n:
        raise ValueError("one flags byte per point")
    xy = np.zeros((n, 24 * deg), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    _check(_lib().gh_points_decompress(cid, _ptr(x), _ptr(flags), n, _ptr(xy), _ptr(inf), _ptr(st)))
    return (xy, inf), st


def limbs_to_bits(x, flags):
    """the ABI's compressed form -> the reference's Vec<bool> rows, (n, deg * 753 + 2) uint8; coefficients must be below 2^753"""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    n, deg = x.shape[0], x.shape[1] // 12
    out = np.zeros((n, deg * MODULUS_BITS + 2), dtype=np.uint8)
    for i in range(n):
        for c in range(deg):
            v = sum(int(w) << (64 * j) for j, w in enumerate(x[i, 12 * c:12 * c + 12]))
            if v >> MODULUS_BITS:
                raise ValueError("a coefficient does not fit 753 bits")
            out[i, MODULUS_BITS * c:MODULUS_BITS * (c + 1)] = [(v >> b) & 1 for b in range(MODULUS_BITS - 1, -1, -1)]
        out[i, -2], out[i, -1] = flags[i] & 1, (flags[i] >> 1) & 1
    return out


def bits_to_limbs(deg, bitvecs):
    """Vec<bool> rows -> the ABI's compressed form.  Leading zero bits are tolerated as read_bits does (fields/mod.rs:290-316):
    over a prime field (deg 1) the coordinate may have any length; a value that does not fit 768 bits reads as all ones (above
    every modulus, InvalidFieldElement).  Over an extension the reference slices fixed 753-bit coefficients."""
    rows = [np.asarray(b, dtype=np.uint8).reshape(-1) for b in bitvecs]
    x = np.zeros((len(rows), 12 * deg), dtype=np.uint64)
    flags = np.zeros(len(rows), dtype=np.uint8)
    for i, b in enumerate(rows):
        body = b[:-2]
        if len(b) < 2 or (deg > 1 and len(body) != deg * MODULUS_BITS):
            raise ValueError("a compressed point is its coordinate bits, the infinity bit and the parity bit")
        flags[i] = int(b[-2] != 0) | int(b[-1] != 0) << 1
        parts = [body] if deg == 1 else [body[MODULUS_BITS * c:MODULUS_BITS * (c + 1)] for c in range(deg)]
        for c, part in enumerate(parts):
            v = int("".join("1" if t else "0" for t in part) or "0", 2)
            if v >> 768:
                v = (1 << 768) - 1
            x[i, 12 * c:12 * c + 12] = [(v >> (64 * j)) & 0xffffffffffffffff for j in range(12)]
    return x, flags


def compress(curve, points):
    """ToCompressedBits::compress per point, as rows of bits"""
    return limbs_to_bits(*compress_limbs(curve, points))


def decompress(curve, bitvecs):
    """FromCompressedBits::decompress per row of bits -> ((xy, inf), status)"""
    _, deg = _deg(curve)
    return decompress_limbs(curve, *bits_to_limbs(deg, bitvecs))


def _verify_validated(pvk, compressed, a, b, c, inputs):
    """the body of pairing.PreparedVerifyingKey.verify_checked (a, b, c: batches of points) and .verify_compressed (a, b, c:
    (x limbs, flags) each) -> (status (n,), point status (n, 3): the code of A, B, C)"""
    from .pairing import _WIDTHS
    g2 = _WIDTHS[pvk.engine].g2_words
    wa, wb = (12, g2 // 2) if compressed else (24, g2)
    axy, ainf = _points(a, wa)
    bxy, binf = _points(b, wb)
    cxy, cinf = _points(c, wa)
    n = axy.shape[0]
    x = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(n, -1) if n else np.zeros((0, 12 * pvk.num_inputs), dtype=np.uint64)
    if bxy.shape[0] != n or cxy.shape[0] != n or x.shape[1] % 12:
        raise ValueError("one A, B, C and one row of inputs per proof")
    st = np.zeros(n, dtype=np.uint8)
    pst = np.zeros((n, 3), dtype=np.uint8)
    fn = _lib().gh_groth16_verify_compressed if compressed else _lib().gh_groth16_verify_checked
    _check(fn(pvk.handle, _ptr(axy), _ptr(ainf), _ptr(bxy), _ptr(binf), _ptr(cxy), _ptr(cinf), _ptr(x) if x.size else None, n,
              x.shape[1] // 12, _ptr(st), _ptr(pst)))
    return st, pst
