"""Batched GM17 proof verification on the device (include/ginger_hip_gm17.h) over the MNT4-753 and MNT6-753 pairings of
pairing.py, with the reference's names (proof-systems/src/gm17/verifier.rs):

    PreparedVerifyingKey(g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, h_g2, query)      prepare_verifying_key, from limb arrays
    PreparedVerifyingKey.from_key(vk)                    the same from the dict gm17.verifying_key returns
        .verify(a, b, c, inputs) -> status               verify_proof per row: 1 Ok(true) (both pairing equations hold),
                                                         0 Ok(false), 2 a proof point off its curve
    verify_proofs(pvk, proofs, inputs) -> status         the same for the A || B || C records of gm17.proof_bytes and integer inputs

Layouts are pairing.py's: rows of 12 u64 Montgomery limbs, a G1 batch (xy: (m, 24), inf: (m,) uint8), a G2 batch (m, 48) over
MNT4-753 and (m, 72) over MNT6-753, public inputs as Montgomery rows of the engine's Fr.  The engine is "mnt4753" unless a key
says engine="mnt6753".  No key point may be at infinity.  Subgroup membership of the points is the caller's business."""
import numpy as np

from . import GingerHipError, _check, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles, limbs
from ._handles import _rows, ci, sz, vp
from .pairing import ENGINES, _G1_REC, _WIDTHS, _points, _wire_rows

_ARGTYPES = {"gh_gm17_vk_create": [ci, vp, vp, vp, vp, vp, vp, sz, _handles.OUT_HANDLE], "gh_gm17_vk_free": [vp],
             "gh_gm17_verify": [vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, vp], "gh_gm17_last_timing": _handles.TIMING}
# every symbol include/ginger_hip_gm17.h declares
GM17_SYMBOLS = list(_ARGTYPES)
PHASES = ["upload", "g_psi", "sums", "test1_miller", "test1_final_exp", "test2_miller", "test2_final_exp", "compare", "download"]
_lib = _handles.binder("GM17", _ARGTYPES)


def last_timing():
    """({phase: milliseconds} of the last verify, total milliseconds)"""
    ms, tot = _handles.last_timing(_lib().gh_gm17_last_timing, len(PHASES))
    return dict(zip(PHASES, ms)), tot


class PreparedVerifyingKey(_handles.Handle):
    """prepare_verifying_key (verifier.rs:9-22): keeps g_alpha, h_beta, g_gamma, h_gamma and h (the last two as line tables) and
    query (as fixed-base tables); e(-g_alpha, h_beta), the tables and the device copies are made on first use"""
    _lib, _prefix = staticmethod(_lib), "gh_gm17_vk"

    def __init__(self, g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, h_g2, query, engine="mnt4753"):
        w = _WIDTHS[engine]
        ga, gg = _rows(g_alpha_g1, 24), _rows(g_gamma_g1, 24)
        hb, hg, h = (_rows(v, w.g2_words) for v in (h_beta_g2, h_gamma_g2, h_g2))
        q = _rows(query, 24)
        if any(v.shape[0] != 1 for v in (ga, gg, hb, hg, h)) or q.shape[0] < 1:
            raise ValueError("one g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2 and h_g2, and at least one point of query")
        self.engine = engine
        self.num_inputs = q.shape[0] - 1
        self._create(ENGINES[engine], _ptr(ga), _ptr(hb), _ptr(gg), _ptr(hg), _ptr(h), _ptr(q), q.shape[0])

    @classmethod
    def from_key(cls, vk):
        """from the dict of gm17.verifying_key: its points as limb rows and its "pairing" """
        return cls(vk["g_alpha_g1"], vk["h_beta_g2"], vk["g_gamma_g1"], vk["h_gamma_g2"], vk["h_g2"], vk["query"], engine=vk["pairing"])

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
        _check(_lib().gh_gm17_verify(self.handle, _ptr(axy), _ptr(ainf), _ptr(bxy), _ptr(binf), _ptr(cxy), _ptr(cinf),
                                     _ptr(x) if x.size else None, n, x.shape[1] // 12, _ptr(st)))
        return st


def verify_proofs(pvk, proofs, inputs):
    """proofs: A || B || C as GroupAffine::write records (gm17.proof_bytes); inputs: one list of integers per proof.
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
