"""Field-based Schnorr without a GPU: the Python restatement against the reference's own two checks, the recoding of the
variable-base kernel (ginger-lib_amd/csrc/schnorr_recode.h compiled by g++, tests/host_shim/schnorr_shim.cpp), and the
argument checks / exports of include/ginger_hip_schnorr.h and of its Rust extern block."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import pyref
import schnorr_ref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = list(schnorr_ref.SCHEMES)
GH_E_BAD_ARG, GH_E_UNSUPPORTED, GH_E_NO_DEVICE = -1, -2, -3
MNT4_G1, MNT4_G2, MNT6_G1 = 0, 1, 2


@pytest.fixture(scope="module")
def refs():
    return {s: schnorr_ref.Schnorr(s) for s in SCHEMES}


# ---- the restatement: the reference's tests sign_and_verify / failed_verification (field_based_schnorr.rs:198-228)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_restatement_sign_and_verify(refs, scheme):
    S = refs[scheme]
    rng = schnorr_ref.rng(1 + len(scheme))
    for msg in ([rng.randrange(S.p)], [], [rng.randrange(S.p), rng.randrange(S.p)]):
        pk, sk = S.keygen(rng)
        assert S.keyverify(pk)
        assert pk == S.pk(sk)
        sig = S.sign(sk, pk, msg, rng)
        assert S.verify(pk, msg, sig) is True


@pytest.mark.parametrize("scheme", SCHEMES)
def test_restatement_failed_verification(refs, scheme):
    S = refs[scheme]
    rng = schnorr_ref.rng(7 + len(scheme))
    msg, bad = [rng.randrange(S.p)], [rng.randrange(S.p)]
    pk, sk = S.keygen(rng)
    sig = S.sign(sk, pk, msg, rng)
    assert S.verify(pk, bad, sig) is False
    bad_sig = S.sign(sk, pk, bad, rng)
    assert S.verify(pk, msg, bad_sig) is False
    new_pk, _ = S.keygen(rng)
    assert S.verify(new_pk, msg, sig) is False
    assert S.verify(pk, msg, (schnorr_ref.BOUND, sig[1])) is None
    assert S.verify(pk, msg, (sig[0], S.p - 1)) is None


@pytest.mark.parametrize("scheme", SCHEMES)
def test_restatement_scalar_multiplication(refs, scheme):
    S = refs[scheme]
    rng = schnorr_ref.rng(3)
    C = S.C
    for k in (0, 1, 2, 3, S.r - 1, S.r, S.r + 1, rng.randrange(S.r)):
        assert schnorr_ref.mul(C, k, S.G) == C.mul(k, S.G), k
    assert schnorr_ref.mul(C, S.r, S.G) is None
    assert schnorr_ref.mul(C, (1 << 753) - 1, S.G) == schnorr_ref.mul(C, ((1 << 753) - 1) % S.r, S.G)


# ---- the recoding the kernel runs
@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("schnorr")
    lib.t_vb_recode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("w", [4, 5, 6])
def test_recoding_reconstructs_the_scalar(shim, w):
    rng = random.Random(w)
    ks = [0, 1, 2, 3, 4, 5, 6, 7, (1 << 753) - 1, (1 << 753) - 2, (1 << 752), (1 << 752) - 1, pyref.P4.p - 1, pyref.P6.p - 1]
    ks += [rng.getrandbits(753) for _ in range(40)] + [rng.getrandbits(rng.randrange(1, 753)) for _ in range(20)]
    m = -(-753 // w)
    for k in ks:
        words = np.array([(k >> (32 * i)) & 0xFFFFFFFF for i in range(24)], dtype=np.uint32)
        d = np.zeros(200, dtype=np.int32)
        assert shim.t_vb_recode(w, words.ctypes.data, d.ctypes.data) == m
        digits = [int(x) for x in d[:m]]
        assert all(x % 2 and abs(x) < (1 << w) for x in digits), k      # odd, non-zero, in the table
        assert digits[-1] > 0
        assert sum(x << (w * j) for j, x in enumerate(digits)) == k | 1, k


# ---- the C ABI without a device
def test_schnorr_symbols_exported_and_kept_apart(gl):
    from ginger_lib_amd import poseidon, schnorr
    lib = gl.load_library()
    for s in schnorr.SCHNORR_SYMBOLS:
        assert hasattr(lib, s), s
    assert not set(schnorr.SCHNORR_SYMBOLS) & set(gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_schnorr.h")).read()
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(schnorr.SCHNORR_SYMBOLS)


def _params(tag):
    import poseidon_ref
    from ginger_lib_amd import poseidon
    return poseidon.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, tag)


def test_create_checks_arguments(gl):
    from ginger_lib_amd import schnorr
    lib = schnorr._lib()
    p4, p6 = _params("mnt4753"), _params("mnt6753")       # hash fields MNT4-753 Fr (= p6) and MNT6-753 Fr (= p4)
    h = ctypes.c_void_p()
    assert lib.gh_schnorr_create(MNT6_G1, p4.handle, 0, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_schnorr_free(h) == 0
    assert lib.gh_schnorr_create(MNT4_G1, p6.handle, 0, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_schnorr_free(h) == 0
    assert lib.gh_schnorr_create(MNT4_G2, p6.handle, 0, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_schnorr_create(3, p4.handle, 0, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_schnorr_create(MNT6_G1, None, 0, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_schnorr_create(MNT6_G1, p6.handle, 0, ctypes.byref(h)) == GH_E_BAD_ARG      # hash over the wrong field
    assert "field" in lib.gh_last_error().decode()
    assert lib.gh_schnorr_create(MNT4_G1, p4.handle, 0, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_schnorr_create(MNT6_G1, p4.handle, 0, None) == GH_E_BAD_ARG
    assert lib.gh_schnorr_free(None) == 0
    with pytest.raises(schnorr.GingerHipError):
        schnorr.FieldBasedSchnorrSignatureScheme(p6, "mnt6753_g1")


def test_compute_entry_points_without_gpu(gl):
    """n == 0 is a no-op everywhere, non-canonical input is GH_E_BAD_ARG before any device work, and on a machine without a
    device every compute entry point fails with GH_E_NO_DEVICE."""
    from ginger_lib_amd import schnorr
    lib = schnorr._lib()
    prm = _params("mnt4753")
    S = schnorr.FieldBasedSchnorrSignatureScheme(prm, "mnt6753_g1")
    h = S.handle
    x = np.zeros((8, 36), dtype=np.uint64)
    b = np.zeros(64, dtype=np.uint8)
    p, pb = x.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    assert lib.gh_schnorr_public_keys(h, p, 0, p, pb) == 0
    assert lib.gh_schnorr_sign(h, p, p, pb, p, 0, 3, p, p, pb) == 0
    assert lib.gh_schnorr_verify(h, p, pb, p, 0, 1, p, pb) == 0
    assert lib.gh_schnorr_keyverify(h, p, pb, 0, pb) == 0
    assert lib.gh_batch_mul(MNT4_G1, p, pb, p, 0, p) == 0
    assert lib.gh_batch_mul(MNT4_G2, p, pb, p, 1, p) == GH_E_UNSUPPORTED
    assert lib.gh_schnorr_verify(h, None, pb, p, 1, 1, p, pb) == GH_E_BAD_ARG
    # non-canonical input: a coordinate equal to the modulus, a scalar of 2^753
    bad = np.zeros((2, 36), dtype=np.uint64)
    bad[0, :12] = pyref.int_to_limbs(pyref.P6.p)
    pbad = bad.ctypes.data_as(ctypes.c_void_p)
    assert lib.gh_schnorr_verify(h, pbad, pb, p, 1, 1, p, pb) == GH_E_BAD_ARG
    assert lib.gh_schnorr_verify(h, p, pb, pbad, 1, 1, p, pb) == GH_E_BAD_ARG            # message
    assert lib.gh_schnorr_verify(h, p, pb, p, 1, 1, pbad, pb) == GH_E_BAD_ARG            # signature
    assert lib.gh_schnorr_keyverify(h, pbad, pb, 1, pb) == GH_E_BAD_ARG
    sk_bad = np.zeros((1, 12), dtype=np.uint64)
    sk_bad[0] = pyref.int_to_limbs(pyref.P4.p)                                            # SchnorrMNT4's secrets are mod p4
    assert lib.gh_schnorr_public_keys(h, sk_bad.ctypes.data_as(ctypes.c_void_p), 1, p, pb) == GH_E_BAD_ARG
    assert lib.gh_schnorr_sign(h, sk_bad.ctypes.data_as(ctypes.c_void_p), p, pb, p, 1, 1, p, p, pb) == GH_E_BAD_ARG
    k_bad = np.zeros((1, 12), dtype=np.uint64)
    k_bad[0, 11] = 1 << 49
    assert lib.gh_batch_mul(MNT6_G1, p, pb, k_bad.ctypes.data_as(ctypes.c_void_p), 1, p) == GH_E_BAD_ARG
    # whether a device is usable is the library's own verdict (gh_init), not the framework's
    expect = GH_E_NO_DEVICE if lib.gh_init(None, 0) == GH_E_NO_DEVICE else 0
    if expect == GH_E_NO_DEVICE:
        assert lib.gh_schnorr_public_keys(h, p, 1, p, pb) == expect
        assert lib.gh_schnorr_sign(h, p, p, pb, p, 1, 1, p, p, pb) == expect
        assert lib.gh_schnorr_verify(h, p, pb, p, 1, 1, p, pb) == expect
        assert lib.gh_schnorr_keyverify(h, p, pb, 1, pb) == expect
        assert lib.gh_batch_mul(MNT4_G1, p, pb, p, 1, p) == expect
        with pytest.raises(schnorr.GingerHipError):
            S.keyverify((x[:1, :24], b[:1]))
    S.close()


def test_package_schnorr_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "schnorr.py")).read()
    for needle in ("tests/", "import pyref", "poseidon_ref", "schnorr_ref", "oracle"):
        assert needle not in txt, needle


# ---- the Rust side (delivered as files: no Rust toolchain checks them here)
RUST_SRC = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")


def test_rust_schnorr_extern_block_is_generated_from_the_header():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    rs = open(os.path.join(RUST_SRC, "schnorr.rs")).read()
    block = rs[rs.index("// ---- GENERATED by"):rs.index("// ---- GENERATED: end")]
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (gh_\w+)\((.*?)\)", block)}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ginger_hip_schnorr.h")).read(), flags=re.S)
    c = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(gh_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)}
    assert sorted(rust) == sorted(c) and len(c) == 8
    for name, params in c.items():
        assert params.count(",") == rust[name].count(","), name
    assert "*mut GhSchnorr" in block and "*mut GhPoseidon" in block
    lib = open(os.path.join(RUST_SRC, "lib.rs")).read()
    assert "pub mod schnorr;" in lib[lib.index("// ---- GENERATED: end"):]
    assert "gh_schnorr" not in lib and "gh_batch_mul" not in lib     # the crate's main extern block stays the two headers
