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
from . import GingerHipError, _ptr    # noqa: F401 (GingerHipError: re-exported)
from . import _handles, pairing
from ._handles import _rows, ci, sz, vp
from .pairing import ENGINES, _WIDTHS

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


class PreparedVerifyingKey(pairing._ProofKey):
    """prepare_verifying_key (verifier.rs:9-22): keeps g_alpha, h_beta, g_gamma, h_gamma and h (the last two as line tables) and
    query (as fixed-base tables); e(-g_alpha, h_beta), the tables and the device copies are made on first use"""
    _lib, _prefix, _verify = staticmethod(_lib), "gh_gm17_vk", "gh_gm17_verify"

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


def verify_proofs(pvk, proofs, inputs):
    """proofs: A || B || C as GroupAffine::write records (gm17.proof_bytes); inputs: one list of integers per proof.
    -> status (n,) uint8: 1 Ok(true), 0 Ok(false), 2 a proof point is not on its curve"""
    return pairing.verify_proofs(pvk, proofs, inputs)
