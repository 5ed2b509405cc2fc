"""Batched MNT4-753 and MNT6-753 ate pairings and Groth16 verification on the device (include/ginger_hip_pairing.h), with the
reference's names (algebra PairingEngine, proof-systems/src/groth16/verifier.rs):

    pairing_product(g1, g2, k=1) -> (n, 48)              final_exponentiation(prod_j miller_loop(P_ij, Q_ij)): pairing for
                                                         k = 1, product_of_pairings for k = 2, 3
    PreparedVerifyingKey(alpha_g1_beta_g2, gamma_g2, delta_g2, gamma_abc_g1)        prepare_verifying_key, from limb arrays
    PreparedVerifyingKey.from_parameters(blob)           the same from a Parameters::write stream
        .verify(a, b, c, inputs) -> status               verify_proof per row: 1 Ok(true), 0 Ok(false), 2 a point off its curve
    verify_proofs(pvk, proofs, inputs) -> status         the same for Proof::write byte strings and integer inputs
    parameters_with_pairing(blob) -> blob                a Parameters stream with the real e(alpha_g1, beta_g2) in its first
                                                         384 bytes (groth16.generate_parameters writes filler there)

Field elements are rows of 12 u64 limbs of the Montgomery form x * 2^768 (numpy uint64).  A batch of G1 points is
(xy: (m, 24), inf: (m,) uint8), of G2 points (xy: (m, 48), inf) with a coordinate as c0 || c1; an Fq4 value is a row of 48
limbs in the order c0.c0, c0.c1, c1.c0, c1.c1 (Fp4::write).  Public inputs are Montgomery rows of MNT4-753 Fr.  Subgroup
membership of the points is the caller's business (the reference checks it where a point is read): verify does not test it,
.verify_checked and .verify_compressed (include/ginger_hip_points.h, module points) do, on the device.

The engine is "mnt4753" unless a call says engine="mnt6753" (pairing="mnt6753" where a Parameters stream is read).  Over
MNT6-753 a G2 coordinate is c0 || c1 || c2, so a G2 batch is (m, 72), an Fq6 value a row of 72 limbs in the order c0.c0,
c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (Fp6::write, 576 bytes), a G2 record 577 bytes, and public inputs are rows of MNT6-753 Fr."""
import numpy as np

from . import GingerHipError, _check, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles, groth16, limbs
from ._handles import _bytes, _rows, ci, sz, vp

_ARGTYPES = {"gh_pairing_product": [ci, vp, vp, vp, vp, sz, sz, vp],
             "gh_groth16_vk_create": [ci, vp, vp, vp, vp, sz, _handles.OUT_HANDLE], "gh_groth16_vk_free": [vp],
             "gh_groth16_verify": [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, vp], "gh_pairing_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_pairing.h declares
PAIRING_SYMBOLS = list(_ARGTYPES)
PHASES = ["upload", "g_ic", "miller", "final_exp", "compare", "download"]
ENGINES = {"mnt4753": 0, "mnt6753": 2}
_lib = _handles.binder("pairing", _ARGTYPES)

_G1_REC = 193


class _Widths:
    """what an engine's layouts are made of: deg Fq coefficients per G2 coordinate and per half of a GT element"""

    def __init__(self, engine):
        self.deg = limbs.G2_DEG[engine]
        self.fq = limbs.base_modulus(engine)
        self.fr = limbs.MODULUS[engine]
        self.g2_words = self.gt_words = 24 * self.deg
        self.g2_rec = 192 * self.deg + 1
        self.gt_bytes = 192 * self.deg


_WIDTHS = {e: _Widths(e) for e in ENGINES}


def last_timing():
    """({phase: milliseconds} of the last pairing_product / verify, total milliseconds)"""
    ms, tot = _handles.last_timing(_lib().gh_pairing_last_timing, len(PHASES))
    return dict(zip(PHASES, ms)), tot


def _points(pts, words):
    xy, inf = pts
    xy = _rows(xy, words)
    inf = _bytes(inf)
    if inf.shape[0] != xy.shape[0]:
        raise ValueError("one infinity byte per point")
    return xy, inf


def pairing_product(g1, g2, k=1, engine="mnt4753"):
    """out[i] = final_exponentiation(prod_{j<k} miller_loop(P_ij, Q_ij)) as (n, 48) limbs ((n, 72) over MNT6-753); pair j of
    row i is point i * k + j"""
    w = _WIDTHS[engine]
    xy1, inf1 = _points(g1, 24)
    xy2, inf2 = _points(g2, w.g2_words)
    m = xy1.shape[0]
    if xy2.shape[0] != m or k < 1 or m % k:
        raise ValueError("one G2 point per G1 point, k of each per row")
    n = m // k
    out = np.zeros((n, w.gt_words), dtype=np.uint64)
    _check(_lib().gh_pairing_product(ENGINES[engine], _ptr(xy1), _ptr(inf1), _ptr(xy2), _ptr(inf2), n, k, _ptr(out)))
    return out


def gt_to_bytes(gt, engine="mnt4753"):
    """one Fq4 row (48 Montgomery limbs) -> its Fp4::write bytes: 4 x 96 canonical little-endian; over MNT6-753 one Fq6 row
    (72 limbs) -> the 6 x 96 bytes of Fp6::write"""
    w = _WIDTHS[engine]
    ints = limbs.ints_from_mont_rows(np.asarray(gt, dtype=np.uint64).reshape(2 * w.deg, 12), w.fq)
    return b"".join(int(v).to_bytes(96, "little") for v in ints)


def _wire_rows(data, rec, coeffs, engine="mnt4753"):
    """GroupAffine::write records -> (Montgomery rows (n, 12 coeffs), infinity bytes); coefficients must be below the modulus"""
    fq = _WIDTHS[engine].fq
    n = len(data) // rec
    if n * rec != len(data):
        raise ValueError("truncated point record")
    vals, inf = [], np.zeros(n, dtype=np.uint8)
    for i in range(n):
        r = data[i * rec:(i + 1) * rec]
        inf[i] = 1 if r[rec - 1] else 0
        for c in range(coeffs):
            v = int.from_bytes(r[96 * c:96 * c + 96], "little")
            if v >= fq:
                raise ValueError("a coordinate is not below the modulus")
            vals.append(v)
    return limbs.mont_rows(vals, fq).reshape(n, 12 * coeffs), inf


class _ProofKey(_handles.Handle):
    """what the Groth16 key and the GM17 key (gm17_verify.py) share; a subclass names its entry point in _verify"""

    def verify(self, a, b, c, inputs):
        """a, c: G1 batches, b: a G2 batch, inputs: (n, num_inputs, 12) Montgomery rows of Fr -> status (n,) uint8"""
        axy, ainf = _points(a, 24)
        bxy, binf = _points(b, _WIDTHS[self.engine].g2_words)
        cxy, cinf = _points(c, 24)
        n = axy.shape[0]
        x = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(n, -1) if n else np.zeros((0, 12 * self.num_inputs), dtype=np.uint64)
        if bxy.shape[0] != n or cxy.shape[0] != n or x.shape[1] % 12:
            raise ValueError("one A, B, C and one row of inputs per proof")
        st = np.zeros(n, dtype=np.uint8)
        _check(getattr(self._lib(), self._verify)(self.handle, _ptr(axy), _ptr(ainf), _ptr(bxy), _ptr(binf), _ptr(cxy), _ptr(cinf),
                                                  _ptr(x) if x.size else None, n, x.shape[1] // 12, _ptr(st)))
        return st


class PreparedVerifyingKey(_ProofKey):
    """prepare_verifying_key (verifier.rs:9-16): keeps alpha_g1_beta_g2, -gamma_g2, -delta_g2 (as line tables, built on the
    device on first use) and gamma_abc_g1 (as fixed-base tables)"""
    _lib, _prefix, _verify = staticmethod(_lib), "gh_groth16_vk", "gh_groth16_verify"

    def __init__(self, alpha_g1_beta_g2, gamma_g2, delta_g2, gamma_abc_g1, engine="mnt4753"):
        w = _WIDTHS[engine]
        gt = _rows(alpha_g1_beta_g2, w.gt_words)
        g, d = _rows(gamma_g2, w.g2_words), _rows(delta_g2, w.g2_words)
        abc = _rows(gamma_abc_g1, 24)
        if gt.shape[0] != 1 or g.shape[0] != 1 or d.shape[0] != 1:
            raise ValueError("one alpha_g1_beta_g2, one gamma_g2, one delta_g2")
        self.engine = engine
        self.num_inputs = abc.shape[0] - 1
        self.alpha_g1_beta_g2 = gt[0].copy()
        self._create(ENGINES[engine], _ptr(gt), _ptr(g), _ptr(d), _ptr(abc), abc.shape[0])

    @classmethod
    def from_parameters(cls, blob, pairing="mnt4753"):
        """from a Parameters::write stream (or groth16.parse_parameters' dict of it); points at infinity are refused"""
        w = _WIDTHS[pairing]
        pk = blob if isinstance(blob, dict) else groth16.parse_parameters(pairing, blob)
        gt = [int.from_bytes(pk["vk_alpha_g1_beta_g2"][96 * c:96 * c + 96], "little") for c in range(2 * w.deg)]
        if any(v >= w.fq for v in gt):
            raise ValueError("alpha_g1_beta_g2 is not an element of the target field (the filler of groth16.generate_parameters? "
                             "see parameters_with_pairing)")
        gt = limbs.mont_rows(gt, w.fq)
        g, gi = _wire_rows(pk["vk_gamma_g2"], w.g2_rec, 2 * w.deg, pairing)
        d, di = _wire_rows(pk["vk_delta_g2"], w.g2_rec, 2 * w.deg, pairing)
        abc, ai = _wire_rows(pk["vk_gamma_abc_g1"], _G1_REC, 2, pairing)
        if gi.any() or di.any() or ai.any():
            raise ValueError("a point of the verifying key is the point at infinity")
        return cls(gt.reshape(1, w.gt_words), g, d, abc, engine=pairing)

    def verify_checked(self, a, b, c, inputs):
        """verify after group_membership_test of A, B, C on the device -> (status (n,), point status (n, 3)); status 3: a
        proof point is not a member of its group (its code, points.NOT_ON_CURVE or NOT_PRIME_ORDER, under A, B or C)"""
        from . import points
        return points._verify_validated(self, False, a, b, c, inputs)

    def verify_compressed(self, a, b, c, inputs):
        """the same for proofs in the wire form: a, b, c are (canonical x limbs, flags) as points.compress_limbs gives them,
        decompressed and verified on the device; point status: the decompression code of A, B, C"""
        from . import points
        return points._verify_validated(self, True, a, b, c, inputs)


def verify_proofs(pvk, proofs, inputs):
    """proofs: Proof::write byte strings (A || B || C records, mod.rs:35-42); inputs: one list of integers per proof.
    -> status (n,) uint8: 1 Ok(true), 0 Ok(false), 2 a proof point is not on its curve"""
    w = _WIDTHS[pvk.engine]
    n = len(proofs)
    if len(inputs) != n:
        raise ValueError("one list of inputs per proof")
    rec = _G1_REC + w.g2_rec + _G1_REC
    if any(len(p) != rec for p in proofs):
        raise ValueError("a proof is not %d bytes" % rec)
    a = _wire_rows(b"".join(p[:_G1_REC] for p in proofs), _G1_REC, 2, pvk.engine)
    b = _wire_rows(b"".join(p[_G1_REC:_G1_REC + w.g2_rec] for p in proofs), w.g2_rec, 2 * w.deg, pvk.engine)
    c = _wire_rows(b"".join(p[_G1_REC + w.g2_rec:] for p in proofs), _G1_REC, 2, pvk.engine)
    if any(len(row) != pvk.num_inputs for row in inputs):
        raise ValueError("the number of public inputs does not match the verifying key")
    flat = [int(v) for row in inputs for v in row]
    if any(v < 0 or v >= w.fr for v in flat):
        raise ValueError("a public input is not below the modulus")
    x = limbs.mont_rows(flat, w.fr).reshape(n, pvk.num_inputs * 12)
    return pvk.verify(a, b, c, x)


def parameters_with_pairing(blob, pairing="mnt4753"):
    """the Parameters::write stream `blob` with vk.alpha_g1_beta_g2 = e(alpha_g1, beta_g2) computed on the device in place of
    its first 384 bytes (576 over MNT6-753; generator.rs:313)"""
    w = _WIDTHS[pairing]
    pk = groth16.parse_parameters(pairing, blob)
    gt = pairing_product(_wire_rows(pk["alpha_g1"], _G1_REC, 2, pairing), _wire_rows(pk["beta_g2"], w.g2_rec, 2 * w.deg, pairing),
                         engine=pairing)
    return gt_to_bytes(gt[0], pairing) + bytes(blob[w.gt_bytes:])
