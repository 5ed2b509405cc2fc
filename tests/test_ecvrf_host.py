"""Bowe-Hopwood and the field-based EC-VRF without a GPU: the Python restatement tests/ecvrf_ref.py against the definitions,
and the argument checks / exports of include/ginger_hip_ecvrf.h and of its Rust extern block."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ecvrf_ref
import pyref
from schnorr_ref import BOUND, mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = list(ecvrf_ref.SCHEMES)
GH_E_BAD_ARG, GH_E_UNSUPPORTED, GH_E_NO_DEVICE = -1, -2, -3
MNT4_G1, MNT4_G2, MNT6_G1 = 0, 1, 2


@pytest.fixture(scope="module")
def refs():
    out = {}
    for s, (_, curve) in ecvrf_ref.SCHEMES.items():
        C = pyref.CURVES[curve]
        out[s] = ecvrf_ref.EcVrf(s, ecvrf_ref.make_bh(C, ecvrf_ref.rng(len(s)), 4, 128))
    return out


# ---- Bowe-Hopwood
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bh_closed_form_with_recipe_generators(refs, scheme):
    """BH(x) = sum over segments of (sum_k d_k 16^k) base_seg, with textbook scalar multiplication"""
    V = refs[scheme]
    C, bh = V.C, V.bh
    rng = ecvrf_ref.rng(2)
    for nbytes in (1, 5, 48, 96, 97, 192):
        data = bytes(rng.randrange(256) for _ in range(nbytes))
        digits = bh.chunks(data)
        want = None
        for seg in range(bh.num_windows):
            k = sum(d * 16 ** j for j, d in enumerate(digits[seg * bh.window_size:(seg + 1) * bh.window_size]))
            want = C.add(want, C.mul(k % V.r, bh.gens[seg][0]))
        assert bh.evaluate(data) == want, nbytes


def test_bh_chunk_encodings_and_padding(refs):
    V = refs["EcVrfMNT4"]
    C, bh = V.C, V.bh
    g0 = bh.gens[0][0]
    # the eight encodings of chunk 0: bits (c0, c1, c2) = byte bits 0, 1, 2
    for code in range(8):
        c0, c1, c2 = code & 1, (code >> 1) & 1, (code >> 2) & 1
        d = (1 - 2 * c2) * (1 + c0 + 2 * c1)
        assert bh.chunks(bytes([code])) == [d, 1, 1]
        first = C.mul(abs(d), g0) if d > 0 else C.neg(C.mul(abs(d), g0))
        want = C.add(C.add(first, bh.gens[0][1]), bh.gens[0][2])     # chunks 1 (bits 3-5) and 2 (bits 6, 7, one pad bit) are 0
        assert bh.evaluate(bytes([code])) == want, code
    assert bh.evaluate(b"") is None
    assert len(bh.chunks(b"\x00")) == 3 and len(bh.chunks(b"\x00\x00")) == 6 and len(bh.chunks(b"\x00" * 3)) == 8
    assert bh.chunks(b"\x80") == [1, 1, 3]                            # bit 7 is c1 of chunk 2, padded with one zero
    with pytest.raises(ValueError):
        bh.evaluate(b"\x00" * (bh.capacity_bits() // 8 + 1))


def test_bh_uses_only_the_chunks_present(refs):
    V = refs["EcVrfMNT6"]
    bh = V.bh
    short = ecvrf_ref.BoweHopwood(V.C, [list(bh.gens[0][:3])])        # 9 bits
    assert short.evaluate(b"\x01") == bh.evaluate(b"\x01")


# ---- EC-VRF
@pytest.mark.parametrize("scheme", SCHEMES)
def test_restatement_prove_and_proof_to_hash(refs, scheme):
    V = refs[scheme]
    rng = ecvrf_ref.rng(1 + len(scheme))
    for L in (0, 1, 2):
        msg = [rng.randrange(V.p) for _ in range(L)]
        pk, sk = V.keygen(rng)
        assert V.keyverify(pk) and pk == V.pk(sk)
        proof = V.prove(sk, pk, msg, rng)
        code, out = V.proof_to_hash(pk, msg, proof)
        assert code == ecvrf_ref.OK
        assert out == V.H.evaluate(list(msg) + list(ecvrf_ref.coords(proof[0])))
        assert (proof[0] is None) == (L == 0)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_restatement_tampering(refs, scheme):
    V = refs[scheme]
    rng = ecvrf_ref.rng(7 + len(scheme))
    msg = [rng.randrange(V.p)]
    pk, sk = V.keygen(rng)
    gamma, c, s = V.prove(sk, pk, msg, rng)
    F, R, G_ = ecvrf_ref.FAILED, ecvrf_ref.RANGE, ecvrf_ref.GAMMA
    assert V.proof_to_hash(pk, [rng.randrange(V.p)], (gamma, c, s))[0] == F
    assert V.proof_to_hash(V.keygen(rng)[0], msg, (gamma, c, s))[0] == F
    assert V.proof_to_hash(pk, msg, (gamma, (c + 1) % BOUND, s))[0] == F
    assert V.proof_to_hash(pk, msg, (gamma, c, (s + 1) % BOUND))[0] == F
    assert V.proof_to_hash(pk, msg, (V.C.add(gamma, V.G), c, s))[0] == F
    assert V.proof_to_hash(pk, msg, (gamma, BOUND, s))[0] == R
    assert V.proof_to_hash(pk, msg, (gamma, c, V.p - 1))[0] == R
    off = (gamma[0], ((gamma[1][0] + 1) % V.p,))
    assert V.proof_to_hash(pk, msg, (off, c, s))[0] == G_
    assert V.proof_to_hash(pk, msg, (off, BOUND, s))[0] == R           # the range check comes first
    assert V.prove_with(sk, pk, msg, 0) is None


# ---- the C ABI without a device
def test_ecvrf_symbols_exported_and_kept_apart(gl):
    from ginger_lib_amd import ecvrf, poseidon, schnorr
    lib = gl.load_library()
    for s in ecvrf.ECVRF_SYMBOLS:
        assert hasattr(lib, s), s
    assert not set(ecvrf.ECVRF_SYMBOLS) & set(gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS + schnorr.SCHNORR_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_ecvrf.h")).read()
    assert sorted(re.findall(r"^int (gh_\w+)\(", hdr, re.M)) == sorted(ecvrf.ECVRF_SYMBOLS)


def _params(tag):
    import poseidon_ref
    from ginger_lib_amd import poseidon
    return poseidon.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, tag)


def _gens(V, count):
    xy = np.zeros((count, 24), dtype=np.uint64)
    for i, P in enumerate(V.bh.flat()[:count]):
        xy[i] = V.fe(P[0][0]) + V.fe(P[1][0])
    return xy


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_create_checks_arguments(gl, refs):
    from ginger_lib_amd import ecvrf
    lib = ecvrf._lib()
    V4, V6 = refs["EcVrfMNT4"], refs["EcVrfMNT6"]                   # groups MNT6-753 G1 and MNT4-753 G1
    g6, g4 = _gens(V4, 512), _gens(V6, 512)
    b = ctypes.c_void_p()
    assert lib.gh_bh_create(MNT6_G1, _p(g6), None, 4, 128, ctypes.byref(b)) == 0 and b.value
    bh6 = b.value
    assert lib.gh_bh_create(MNT4_G1, _p(g4), None, 2, 256, ctypes.byref(b)) == 0 and b.value
    bh4 = b.value
    assert lib.gh_bh_create(MNT4_G1, _p(g6), None, 4, 128, ctypes.byref(b)) == GH_E_BAD_ARG      # not on that curve
    assert lib.gh_bh_create(MNT4_G2, _p(g4), None, 4, 128, ctypes.byref(b)) == GH_E_BAD_ARG
    assert lib.gh_bh_create(MNT6_G1, _p(g6), None, 0, 128, ctypes.byref(b)) == GH_E_BAD_ARG
    assert lib.gh_bh_create(MNT6_G1, None, None, 4, 128, ctypes.byref(b)) == GH_E_BAD_ARG
    bad = g6.copy()
    bad[7, :12] = pyref.int_to_limbs(V4.p)                                                      # a coordinate equal to p
    assert lib.gh_bh_create(MNT6_G1, _p(bad), None, 4, 128, ctypes.byref(b)) == GH_E_BAD_ARG
    inf = np.zeros(512, dtype=np.uint8)
    inf[7] = 1                                                                                  # ... still checked at infinity
    assert lib.gh_bh_create(MNT6_G1, _p(bad), _p(inf), 4, 128, ctypes.byref(b)) == GH_E_BAD_ARG
    off = g6.copy()
    off[3, 12:] = off[3, :12]
    assert lib.gh_bh_create(MNT6_G1, _p(off), None, 4, 128, ctypes.byref(b)) == GH_E_BAD_ARG
    inf[7] = 0
    inf[3] = 1
    assert lib.gh_bh_create(MNT6_G1, _p(off), _p(inf), 4, 128, ctypes.byref(b)) == 0           # off the curve but at infinity
    assert lib.gh_bh_free(b) == 0
    p4, p6 = _params("mnt4753"), _params("mnt6753")                 # hash fields MNT4-753 Fr (= p6) and MNT6-753 Fr (= p4)
    h = ctypes.c_void_p()
    assert lib.gh_ecvrf_create(MNT6_G1, p4.handle, bh6, 0, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_ecvrf_free(h) == 0
    assert lib.gh_ecvrf_create(MNT4_G1, p6.handle, bh4, 0, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_ecvrf_free(h) == 0
    assert lib.gh_ecvrf_create(MNT4_G2, p6.handle, bh4, 0, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_create(MNT6_G1, p6.handle, bh6, 0, ctypes.byref(h)) == GH_E_BAD_ARG     # hash over the wrong field
    assert "field" in lib.gh_last_error().decode()
    assert lib.gh_ecvrf_create(MNT6_G1, p4.handle, bh4, 0, ctypes.byref(h)) == GH_E_BAD_ARG     # BH over the other curve
    assert "curve" in lib.gh_last_error().decode()
    assert lib.gh_ecvrf_create(MNT6_G1, p4.handle, None, 0, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_create(MNT6_G1, p4.handle, p4.handle, 0, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_create(MNT6_G1, p4.handle, bh6, 23, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_create(MNT6_G1, p4.handle, bh6, 0, None) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_free(None) == 0 and lib.gh_bh_free(None) == 0
    assert lib.gh_bh_free(bh6) == 0 and lib.gh_bh_free(bh4) == 0
    with pytest.raises(ecvrf.GingerHipError):
        ecvrf.BoweHopwoodPedersenCRH("mnt4753_g1", g6, None, 4, 128)


def test_compute_entry_points_without_gpu(gl, refs):
    """n == 0 is a no-op everywhere, non-canonical input and an over-long message are GH_E_BAD_ARG before any device work, and
    on a machine without a device every compute entry point fails with GH_E_NO_DEVICE."""
    from ginger_lib_amd import ecvrf
    lib = ecvrf._lib()
    V = refs["EcVrfMNT4"]
    B = ecvrf.BoweHopwoodPedersenCRH("mnt6753_g1", _gens(V, 512), None, 4, 128)
    D = ecvrf.FieldBasedEcVrf(_params("mnt4753"), B, "mnt6753_g1")
    h, bh = D.handle, B.handle
    x = np.zeros((8, 36), dtype=np.uint64)
    y = np.zeros(1024, dtype=np.uint8)
    p, pb = _p(x), _p(y)
    assert lib.gh_ecvrf_public_keys(h, p, 0, p, pb) == 0
    assert lib.gh_ecvrf_prove(h, p, p, pb, p, 0, 2, p, p, pb, p, pb) == 0
    assert lib.gh_ecvrf_proof_to_hash(h, p, pb, p, 0, 1, p, pb, p, p, pb) == 0
    assert lib.gh_ecvrf_keyverify(h, p, pb, 0, pb) == 0
    assert lib.gh_bh_hash(bh, pb, 0, 5, p, pb) == 0
    assert lib.gh_batch_double_mul(MNT4_G1, p, pb, p, p, pb, p, 0, p) == 0
    assert lib.gh_batch_double_mul(MNT4_G2, p, pb, p, p, pb, p, 1, p) == GH_E_UNSUPPORTED
    assert lib.gh_ecvrf_proof_to_hash(h, None, pb, p, 1, 1, p, pb, p, p, pb) == GH_E_BAD_ARG
    # capacity: 768 len <= 3 * 512 chunks -> len <= 2; 8 nbytes <= 1536 -> nbytes <= 192
    big = np.zeros((1, 3, 12), dtype=np.uint64)
    assert lib.gh_ecvrf_proof_to_hash(h, p, pb, _p(big), 1, 3, p, pb, p, p, pb) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_prove(h, p, p, pb, _p(big), 1, 3, p, p, pb, p, pb) == GH_E_BAD_ARG
    assert "longer" in lib.gh_last_error().decode()
    assert lib.gh_bh_hash(bh, pb, 1, 193, p, pb) == GH_E_BAD_ARG
    # non-canonical input: a coordinate / message element / c / s equal to the modulus, a key equal to the group order
    bad = np.zeros((2, 36), dtype=np.uint64)
    bad[0, :12] = pyref.int_to_limbs(V.p)
    pbad = _p(bad)
    assert lib.gh_ecvrf_proof_to_hash(h, pbad, pb, p, 1, 1, p, pb, p, p, pb) == GH_E_BAD_ARG          # pk
    assert lib.gh_ecvrf_proof_to_hash(h, p, pb, pbad, 1, 1, p, pb, p, p, pb) == GH_E_BAD_ARG          # message
    assert lib.gh_ecvrf_proof_to_hash(h, p, pb, p, 1, 1, pbad, pb, p, p, pb) == GH_E_BAD_ARG          # gamma
    assert lib.gh_ecvrf_proof_to_hash(h, p, pb, p, 1, 1, p, pb, pbad, p, pb) == GH_E_BAD_ARG          # c
    bad_s = np.zeros((1, 24), dtype=np.uint64)
    bad_s[0, 12:] = pyref.int_to_limbs(V.p)
    assert lib.gh_ecvrf_proof_to_hash(h, p, pb, p, 1, 1, p, pb, _p(bad_s), p, pb) == GH_E_BAD_ARG     # s
    assert lib.gh_ecvrf_keyverify(h, pbad, pb, 1, pb) == GH_E_BAD_ARG
    sk_bad = np.zeros((1, 12), dtype=np.uint64)
    sk_bad[0] = pyref.int_to_limbs(V.r)                                                                # EcVrfMNT4's secrets are mod p4
    assert lib.gh_ecvrf_public_keys(h, _p(sk_bad), 1, p, pb) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_prove(h, _p(sk_bad), p, pb, p, 1, 1, p, p, pb, p, pb) == GH_E_BAD_ARG
    assert lib.gh_ecvrf_prove(h, p, p, pb, p, 1, 1, _p(sk_bad), p, pb, p, pb) == GH_E_BAD_ARG          # nonce
    k_bad = np.zeros((1, 12), dtype=np.uint64)
    k_bad[0, 11] = 1 << 49
    assert lib.gh_batch_double_mul(MNT6_G1, p, pb, p, p, pb, _p(k_bad), 1, p) == GH_E_BAD_ARG
    assert lib.gh_batch_double_mul(MNT6_G1, pbad, pb, p, p, pb, p, 1, p) == GH_E_BAD_ARG
    # whether a device is usable is the library's own verdict (gh_init), not the framework's
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:
        e = GH_E_NO_DEVICE
        assert lib.gh_ecvrf_public_keys(h, p, 1, p, pb) == e
        assert lib.gh_ecvrf_prove(h, p, p, pb, p, 1, 1, p, p, pb, p, pb) == e
        assert lib.gh_ecvrf_proof_to_hash(h, p, pb, p, 1, 1, p, pb, p, p, pb) == e
        assert lib.gh_ecvrf_keyverify(h, p, pb, 1, pb) == e
        assert lib.gh_bh_hash(bh, pb, 1, 5, p, pb) == e
        assert lib.gh_batch_double_mul(MNT4_G1, p, pb, p, p, pb, p, 1, p) == e
        with pytest.raises(ecvrf.GingerHipError):
            D.keyverify((x[:1, :24], y[:1]))
    D.close()
    B.close()


def test_package_ecvrf_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "ecvrf.py")).read()
    for needle in ("tests/", "import pyref", "poseidon_ref", "schnorr_ref", "ecvrf_ref", "oracle"):
        assert needle not in txt, needle


# ---- the Rust side (delivered as files: no Rust toolchain checks them here)
RUST_SRC = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")


def test_rust_ecvrf_extern_block_is_generated_from_the_header():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    rs = open(os.path.join(RUST_SRC, "ecvrf.rs")).read()
    block = rs[rs.index("// ---- GENERATED by"):rs.index("// ---- GENERATED: end")]
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (gh_\w+)\((.*?)\)", block)}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ginger_hip_ecvrf.h")).read(), flags=re.S)
    c = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(gh_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)}
    assert sorted(rust) == sorted(c) and len(c) == 11
    for name, params in c.items():
        assert params.count(",") == rust[name].count(","), name
    assert "*mut GhBh" in block and "*mut GhEcvrf" in block and "*mut GhPoseidon" in block
    lib = open(os.path.join(RUST_SRC, "lib.rs")).read()
    assert "pub mod ecvrf;" in lib[lib.index("// ---- GENERATED: end"):]
    assert "gh_ecvrf" not in lib and "gh_bh_" not in lib and "gh_batch_double_mul" not in lib
