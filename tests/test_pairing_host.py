"""The MNT4-753 pairing without a GPU: the Python restatement against the reference's known answer, the GH_HD code of
ginger-lib_amd/csrc/pairing29.h compiled by g++ (tests/host_shim/pairing_shim.cpp) against both, the generated constants
re-derived from p and r, and the argument checks / exports of include/ginger_hip_pairing.h and of its Rust extern block.
Every comparison is exact integer equality."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import pairing_ref as pr
import pyref
from pairing_ref import fq4_of, fq4_row, g1_row, g2_row, limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "build", "libpairing_shim.so")
F = pyref.P4
C1, C2 = pr.C1, pr.C2
GH_E_BAD_ARG, GH_E_NO_DEVICE = -1, -3
V = ctypes.c_void_p


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(ROOT, "tests", "host_shim", "pairing_shim.cpp")
    deps = [src] + [os.path.join(ROOT, "ginger-lib_amd", "csrc", f)
                    for f in ("fp29.h", "ec29.h", "pairing29.h", "pairing_constants_gen.h", "constants_gen.h")]
    os.makedirs(os.path.dirname(SHIM), exist_ok=True)
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SHIM, src])
    lib = ctypes.CDLL(SHIM)
    lib.t_pairing_product.argtypes = [V, V, V, V, ctypes.c_int, V]
    lib.t_pairing_prepared.argtypes = [V, V, V]
    lib.t_fq4_op.argtypes = [ctypes.c_int, V, V, V]
    return lib


def shim_product(shim, pairs):
    k = len(pairs)
    a = np.ascontiguousarray(np.concatenate([g1_row(P) for P, _ in pairs]))
    b = np.ascontiguousarray(np.concatenate([g2_row(Q) for _, Q in pairs]))
    ai = np.array([P is None for P, _ in pairs], dtype=np.uint8)
    bi = np.array([Q is None for _, Q in pairs], dtype=np.uint8)
    out = np.zeros(48, dtype=np.uint64)
    assert shim.t_pairing_product(a.ctypes.data, ai.ctypes.data, b.ctypes.data, bi.ctypes.data, k, out.ctypes.data) == 0
    return fq4_of(out)


def shim_op(shim, op, a, b=None):
    x, y = fq4_row(a), fq4_row(b if b is not None else pr.ONE)
    out = np.zeros(48, dtype=np.uint64)
    assert shim.t_fq4_op(op, x.ctypes.data, y.ctypes.data, out.ctypes.data) == 0
    return fq4_of(out)


# ---- 1. the restatement against the reference's known answer (curves/mnt4753/tests.rs:266-467)
def test_restatement_equals_the_known_answer():
    P, Q, want = pr.kat()
    assert C1.on_curve(P) and C2.on_curve(Q)
    got = pr.pairing(P, Q)
    assert got == want
    assert got != pr.ONE and pr.fpow(got, pr.r) == pr.ONE


# ---- 2. the device's arithmetic on the host against the known answer: all four Fq words
def test_shim_pairing_equals_the_known_answer(shim):
    P, Q, want = pr.kat()
    got = shim_product(shim, [(P, Q)])
    assert pr.tower(got) == pr.tower(want)
    a, b, out = g1_row(P), g2_row(Q), np.zeros(48, dtype=np.uint64)
    assert shim.t_pairing_prepared(a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0      # the prepared-Q steps
    assert fq4_of(out) == want


# ---- 3. the shim against the restatement
def test_shim_agrees_with_the_restatement(shim):
    rng = random.Random(753)
    for _ in range(3):
        P, Q = C1.mul(rng.randrange(1, pr.r), C1.G), C2.mul(rng.randrange(1, pr.r), C2.G)
        assert shim_product(shim, [(P, Q)]) == pr.pairing(P, Q)
    P, Q = C1.mul(5, C1.G), C2.mul(7, C2.G)
    pairs = [(P, Q), (C1.neg(P), Q)]
    assert pr.product(pairs) == pr.ONE
    assert shim_product(shim, pairs) == pr.ONE                       # e(P, Q) e(-P, Q) = 1 under one final exponentiation
    assert shim_product(shim, [(None, Q)]) == pr.ONE == pr.product([(None, Q)])
    assert shim_product(shim, [(P, None)]) == pr.ONE == pr.product([(P, None)])
    three = [(P, Q), (None, Q), (C1.G, C2.G)]
    assert shim_product(shim, three) == pr.product(three)


# ---- 4. the tower
def test_shim_fq4_arithmetic(shim):
    rng = random.Random(4)
    rnd = lambda: [rng.randrange(pr.p) for _ in range(4)]
    for _ in range(3):
        a, b = rnd(), rnd()
        assert shim_op(shim, 0, a, b) == pr.mul(a, b)
        assert shim_op(shim, 1, a) == pr.mul(a, a)
        assert shim_op(shim, 2, a) == pr.inv(a) and pr.mul(a, pr.inv(a)) == pr.ONE
        for k in (1, 2, 3):
            assert shim_op(shim, 2 + k, a) == pr.frobenius(a, k), k
        assert shim_op(shim, 9, a) == pr.from_tower([v if i < 2 else (-v) % pr.p for i, v in enumerate(pr.tower(a))])
        sparse = pr.from_tower([b[0], 0, b[2], b[3]])
        assert shim_op(shim, 8, a, sparse) == pr.mul(a, sparse)
        u = pr.mul(pr.frobenius(a, 2), pr.inv(a))                    # after the easy part: norm one over Fq2
        assert shim_op(shim, 6, u) == pr.mul(u, u)
        assert shim_op(shim, 7, u) == pr.fpow(u, pr.T - 1)
        assert shim_op(shim, 10, a) == pr.final_exponentiation(a)
    assert shim_op(shim, 2, [0, 0, 0, 0]) == [0, 0, 0, 0]            # the inverse of zero is zero
    assert shim_op(shim, 10, [0, 0, 0, 0]) == [0, 0, 0, 0]
    assert shim_op(shim, 0, pr.ONE, pr.ONE) == pr.ONE


# ---- 5. the constants
def test_constants_rederived_from_p_and_r():
    J = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_constants.json")))
    p, r = pr.p, pr.r
    T = r - p
    assert int(J["ate_loop_count"], 16) == T and T.bit_length() == 377 and J["ate_is_loop_count_neg"] is True
    naf = J["ate_naf"]
    assert len(naf) == 376 and sum(1 for d in naf if d) == 123 and set(naf) <= {-1, 0, 1}
    assert all(not (x and y) for x, y in zip(naf, naf[1:] + [1]))                         # non-adjacent, the leading 1 included
    assert sum(d << i for i, d in enumerate(naf)) + (1 << len(naf)) == T
    assert (p * p + 1) % r == 0
    m1, w0 = int(J["final_exponent_last_chunk_1"], 16), int(J["final_exponent_last_chunk_abs_of_w0"], 16)
    assert J["final_exponent_last_chunk_w0_is_neg"] is True and (p * p + 1) // r == m1 * p - w0 and (m1, w0) == (1, T - 1)
    assert (p ** 4 - 1) // r == (p * p - 1) * (m1 * p - w0)
    w0n = J["w0_naf"]
    assert set(w0n) <= {-1, 0, 1} and w0n[-1] == 1 and sum(d << i for i, d in enumerate(w0n)) == w0
    assert all(not (x and y) for x, y in zip(w0n, w0n[1:]))
    assert J["nonresidue"] == 13 and pow(13, (p - 1) // 2, p) == p - 1                   # 13 is a non-residue
    assert [int(v, 16) for v in J["frobenius_fq2_c1"]] == [pow(13, (p ** i - 1) // 2, p) for i in range(2)] == [1, p - 1]
    assert [int(v, 16) for v in J["frobenius_fq4_c1"]] == [pow(13, (p ** i - 1) // 4, p) for i in range(4)]
    assert [int(v, 16) for v in J["twist"]] == [0, 1]
    assert [int(v, 16) for v in J["twist_coeff_a"]] == [C1.a[0] * 13 % p, 0] == list(C2.a)
    hdr = open(os.path.join(ROOT, "ginger-lib_amd", "csrc", "pairing_constants_gen.h")).read()
    digits = lambda name: [int(t) for t in re.search(r"#define %s \{(.*?)\}" % name, hdr).group(1).split(",")]
    assert digits("GH_MNT4_ATE_NAF") == naf[::-1] and digits("GH_MNT4_W0_NAF") == w0n[::-1]
    assert "#define GH_MNT4_ATE_DIGITS 376" in hdr and "#define GH_MNT4_ATE_NONZERO 123" in hdr
    for i, v in enumerate(J["frobenius_fq4_c1"]):
        words = [int(t.rstrip("u"), 16) for t in re.search(r"#define GH_MNT4_FROB4_C1_%d_I29 \{(.*?)\}" % i, hdr).group(1).split(",")]
        assert sum(w << (29 * k) for k, w in enumerate(words)) == int(v, 16) * pow(2, 754, p) % p


# ---- 6. the C ABI without a device
def test_pairing_symbols_exported_and_kept_apart(gl):
    from ginger_lib_amd import ecvrf, pairing, poseidon, schnorr
    lib = gl.load_library()
    for s in pairing.PAIRING_SYMBOLS:
        assert hasattr(lib, s), s
    others = gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS + schnorr.SCHNORR_SYMBOLS + ecvrf.ECVRF_SYMBOLS
    assert not set(pairing.PAIRING_SYMBOLS) & set(others)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_pairing.h")).read()
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(pairing.PAIRING_SYMBOLS) and len(declared) == 5


def _vk_arrays():
    gt = fq4_row(pr.ONE).reshape(1, 48)
    gamma, delta = g2_row(C2.mul(3, C2.G)).reshape(1, 48), g2_row(C2.mul(5, C2.G)).reshape(1, 48)
    abc = np.stack([g1_row(C1.mul(k, C1.G)) for k in (2, 7)])
    return gt, gamma, delta, abc


def test_vk_create_checks_arguments(gl):
    from ginger_lib_amd import pairing
    lib = pairing._lib()
    gt, gamma, delta, abc = _vk_arrays()
    ptr = lambda a: a.ctypes.data_as(V)
    h = V()
    assert lib.gh_groth16_vk_create(0, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_groth16_vk_free(h) == 0
    assert lib.gh_groth16_vk_free(None) == 0
    for args in ((None, ptr(gamma), ptr(delta), ptr(abc)), (ptr(gt), None, ptr(delta), ptr(abc)), (ptr(gt), ptr(gamma), None, ptr(abc)),
                 (ptr(gt), ptr(gamma), ptr(delta), None)):
        assert lib.gh_groth16_vk_create(0, *args, 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_groth16_vk_create(0, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, None) == GH_E_BAD_ARG
    assert lib.gh_groth16_vk_create(1, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == GH_E_BAD_ARG     # no such engine
    assert lib.gh_groth16_vk_create(0, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 0, ctypes.byref(h)) == GH_E_BAD_ARG     # n_abc = 0
    big = np.array(pyref.int_to_limbs(pr.p), dtype=np.uint64)                                                             # a coefficient = p
    for which in range(4):
        arrs = [a.copy() for a in (gt, gamma, delta, abc)]
        arrs[which].reshape(-1)[:12] = big
        assert lib.gh_groth16_vk_create(0, *[ptr(a) for a in arrs], 2, ctypes.byref(h)) == GH_E_BAD_ARG, which
        assert "modulus" in lib.gh_last_error().decode()
    off = gamma.copy()
    off[0, :12] = limbs(1234)                                                                                             # gamma off the curve
    assert lib.gh_groth16_vk_create(0, ptr(gt), ptr(off), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert "curve" in lib.gh_last_error().decode()
    off1 = abc.copy()
    off1[1, 12:24] = limbs(99)
    assert lib.gh_groth16_vk_create(0, ptr(gt), ptr(gamma), ptr(delta), ptr(off1), 2, ctypes.byref(h)) == GH_E_BAD_ARG
    with pytest.raises(pairing.GingerHipError):
        pairing.PreparedVerifyingKey(gt, off, delta, abc)


def test_compute_entry_points_without_gpu(gl):
    """n == 0 is a no-op, bad arguments are GH_E_BAD_ARG before any device work, and without a device the compute entry points
    return GH_E_NO_DEVICE; creating a key needs no device."""
    from ginger_lib_amd import pairing
    lib = pairing._lib()
    pvk = pairing.PreparedVerifyingKey(*_vk_arrays())
    assert pvk.num_inputs == 1
    h = pvk.handle
    x = np.zeros((4, 48), dtype=np.uint64)
    b = np.zeros(16, dtype=np.uint8)
    p, pb = x.ctypes.data_as(V), b.ctypes.data_as(V)
    assert lib.gh_pairing_product(0, p, pb, p, pb, 0, 1, p) == 0
    assert lib.gh_pairing_product(0, None, None, None, None, 0, 3, None) == 0
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 0, 1, pb) == 0
    assert lib.gh_pairing_product(7, p, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    for k in (0, 4):
        assert lib.gh_pairing_product(0, p, pb, p, pb, 1, k, p) == GH_E_BAD_ARG
    assert lib.gh_pairing_product(0, None, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 0, pb) == GH_E_BAD_ARG          # n_inputs + 1 != n_abc
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 2, pb) == GH_E_BAD_ARG
    assert "MalformedVerifyingKey" in lib.gh_last_error().decode()
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, None, 1, 1, pb) == GH_E_BAD_ARG
    assert lib.gh_groth16_verify(None, p, pb, p, pb, p, pb, p, 1, 1, pb) < 0
    bad = np.zeros((2, 48), dtype=np.uint64)
    bad[0, :12] = pyref.int_to_limbs(pr.p)
    pbad = bad.ctypes.data_as(V)
    assert lib.gh_pairing_product(0, pbad, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    assert lib.gh_pairing_product(0, p, pb, pbad, pb, 1, 1, p) == GH_E_BAD_ARG
    for pos in range(3):
        args = [p, pb, p, pb, p, pb]
        args[2 * pos] = pbad
        assert lib.gh_groth16_verify(h, *args, p, 1, 1, pb) == GH_E_BAD_ARG, pos
    rbad = np.zeros((1, 12), dtype=np.uint64)
    rbad[0] = pyref.int_to_limbs(pr.r)                                                          # a public input = r
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, rbad.ctypes.data_as(V), 1, 1, pb) == GH_E_BAD_ARG
    buf = (ctypes.c_float * 6)()
    tot = ctypes.c_float()
    assert lib.gh_pairing_last_timing(buf, 6, ctypes.byref(tot)) == 6
    assert lib.gh_pairing_last_timing(None, 3, None) == GH_E_BAD_ARG
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:                                                  # the library's own verdict
        assert lib.gh_pairing_product(0, p, pb, p, pb, 1, 1, p) == GH_E_NO_DEVICE
        assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 1, pb) == GH_E_NO_DEVICE
        with pytest.raises(pairing.GingerHipError):
            pairing.pairing_product((x[:1, :24], b[:1]), (x[:1], b[:1]))
    pvk.close()


def test_package_pairing_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "pairing.py")).read()
    for needle in ("tests/", "import pyref", "pairing_ref", "groth16_ref", "oracle"):
        assert needle not in txt, needle


def test_wire_helpers_round_trip():
    """Proof::write records -> limb rows, and an Fq4 row -> the bytes of Fp4::write"""
    from ginger_lib_amd import pairing
    P, Q, want = pr.kat()
    rec = P[0][0].to_bytes(96, "little") + P[1][0].to_bytes(96, "little") + b"\x00"
    xy, inf = pairing._wire_rows(rec + bytes(192) + b"\x01", 193, 2)
    assert list(xy[0]) == list(g1_row(P)) and list(inf) == [0, 1]
    assert pairing.gt_to_bytes(fq4_row(want)) == b"".join(v.to_bytes(96, "little") for v in pr.tower(want))
    with pytest.raises(ValueError):
        pairing._wire_rows(pr.p.to_bytes(96, "little") + bytes(97), 193, 2)


# ---- the Rust side (delivered as files: no Rust toolchain checks them here)
def test_rust_pairing_extern_block_is_generated_from_the_header():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    src = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")
    rs = open(os.path.join(src, "pairing.rs")).read()
    block = rs[rs.index("// ---- GENERATED by"):rs.index("// ---- GENERATED: end")]
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (gh_\w+)\((.*?)\)", block)}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ginger_hip_pairing.h")).read(), flags=re.S)
    c = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(gh_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)}
    assert sorted(rust) == sorted(c) and len(c) == 5
    for name, params in c.items():
        assert params.count(",") == rust[name].count(","), name
    assert "*mut GhGroth16Vk" in block
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "pub mod pairing;" in lib[lib.index("// ---- GENERATED: end"):]
    assert "gh_pairing" not in lib and "gh_groth16" not in lib       # the crate's main extern block stays the two headers
