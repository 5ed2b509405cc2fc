"""The MNT6-753 pairing without a GPU: the Python restatement (tests/pairing6_ref.py) against the reference's known answer, the
GH_HD code of ginger-lib_amd/csrc/pairing29_mnt6.h compiled by g++ (tests/host_shim/pairing6_shim.cpp) against both, the
generated constants re-derived from p and r, and the argument checks of engine 2 of include/ginger_hip_pairing.h.
Every comparison is exact integer equality."""
import ctypes
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import pairing6_ref as pr
import pyref
from pairing6_ref import fq6_of, fq6_row, g1_row, g2_row, limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "build", "libpairing6_shim.so")
C1, C2 = pr.C1, pr.C2
GH_E_BAD_ARG, GH_E_NO_DEVICE = -1, -3
MNT6 = 2
V = ctypes.c_void_p


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(ROOT, "tests", "host_shim", "pairing6_shim.cpp")
    deps = [src] + [os.path.join(ROOT, "ginger-lib_amd", "csrc", f)
                    for f in ("fp29.h", "ec29.h", "pairing29.h", "pairing29_mnt6.h", "pairing_constants_gen.h", "constants_gen.h")]
    os.makedirs(os.path.dirname(SHIM), exist_ok=True)
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SHIM, src])
    lib = ctypes.CDLL(SHIM)
    lib.t_pairing6_product.argtypes = [V, V, V, V, ctypes.c_int, V]
    lib.t_pairing6_prepared.argtypes = [V, V, V]
    lib.t_fq6_op.argtypes = [ctypes.c_int, V, V, V]
    return lib


def shim_product(shim, pairs):
    k = len(pairs)
    a = np.ascontiguousarray(np.concatenate([g1_row(P) for P, _ in pairs]))
    b = np.ascontiguousarray(np.concatenate([g2_row(Q) for _, Q in pairs]))
    ai = np.array([P is None for P, _ in pairs], dtype=np.uint8)
    bi = np.array([Q is None for _, Q in pairs], dtype=np.uint8)
    out = np.zeros(72, dtype=np.uint64)
    assert shim.t_pairing6_product(a.ctypes.data, ai.ctypes.data, b.ctypes.data, bi.ctypes.data, k, out.ctypes.data) == 0
    return fq6_of(out)


def shim_op(shim, op, a, b=None):
    x, y = fq6_row(a), fq6_row(b if b is not None else pr.ONE)
    out = np.zeros(72, dtype=np.uint64)
    assert shim.t_fq6_op(op, x.ctypes.data, y.ctypes.data, out.ctypes.data) == 0
    return fq6_of(out)


# ---- 1. the restatement against the reference's known answer (curves/mnt6753/tests.rs:319-590)
def test_restatement_equals_the_known_answer():
    P, Q, want = pr.kat()
    assert C1.on_curve(P) and C2.on_curve(Q)
    got = pr.pairing(P, Q)
    assert got == want
    assert got != pr.ONE and pr.fpow(got, pr.r) == pr.ONE


# ---- 2. the device's arithmetic on the host against the known answer: all six Fq words
def test_shim_pairing_equals_the_known_answer(shim):
    P, Q, want = pr.kat()
    got = shim_product(shim, [(P, Q)])
    assert pr.tower(got) == pr.tower(want)
    a, b, out = g1_row(P), g2_row(Q), np.zeros(72, dtype=np.uint64)
    assert shim.t_pairing6_prepared(a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0     # the prepared-Q steps
    assert fq6_of(out) == want


# ---- 3. the shim against the restatement
def test_shim_agrees_with_the_restatement(shim):
    rng = random.Random(6753)
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
def test_shim_fq6_arithmetic(shim):
    rng = random.Random(6)
    rnd = lambda: [rng.randrange(pr.p) for _ in range(6)]
    for _ in range(3):
        a, b = rnd(), rnd()
        assert shim_op(shim, 0, a, b) == pr.mul(a, b)
        assert shim_op(shim, 1, a) == pr.mul(a, a)
        assert shim_op(shim, 2, a) == pr.inv(a) and pr.mul(a, pr.inv(a)) == pr.ONE
        for k in (1, 2, 3, 4, 5):
            assert shim_op(shim, 2 + k, a) == pr.frobenius(a, k), k
        assert shim_op(shim, 11, a) == pr.from_tower([v if i < 3 else (-v) % pr.p for i, v in enumerate(pr.tower(a))])
        sparse = pr.from_tower([0, 0, b[0], b[1], b[2], b[3]])       # [c0: (0, 0, a), c1: full]
        assert shim_op(shim, 10, a, sparse) == pr.mul(a, sparse)
        u = pr.fpow(a, (pr.p ** 3 - 1) * (pr.p + 1))                 # after the easy part: norm one over Fq3
        assert pr.mul(u, pr.frobenius(u, 3)) == pr.ONE
        assert shim_op(shim, 8, u) == pr.mul(u, u)
        assert shim_op(shim, 9, u) == pr.fpow(u, pr.T)
        assert shim_op(shim, 12, a) == pr.final_exponentiation(a)
    assert shim_op(shim, 2, pr.ZERO) == pr.ZERO                      # the inverse of zero is zero
    assert shim_op(shim, 12, pr.ZERO) == pr.ZERO
    assert shim_op(shim, 0, pr.ONE, pr.ONE) == pr.ONE


# ---- 5. the constants
def test_constants_rederived_from_p_and_r():
    J = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing6_constants.json")))
    J4 = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_constants.json")))
    p, r = pr.p, pr.r
    assert p == pyref.P6.p and r == pyref.P4.p
    T = p - r
    assert int(J["ate_loop_count"], 16) == T and T > 0 and T.bit_length() == 377 and J["ate_is_loop_count_neg"] is False
    assert T == int(J4["ate_loop_count"], 16)                                            # the same integer as MNT4's |T|
    naf = J["ate_naf"]
    assert naf == J4["ate_naf"]
    assert len(naf) == 376 and sum(1 for d in naf if d) == 123 and set(naf) <= {-1, 0, 1}
    assert all(not (x and y) for x, y in zip(naf, naf[1:] + [1]))                         # non-adjacent, the leading 1 included
    assert sum(d << i for i, d in enumerate(naf)) + (1 << len(naf)) == T
    assert (p * p - p + 1) % r == 0
    m1, w0 = int(J["final_exponent_last_chunk_1"], 16), int(J["final_exponent_last_chunk_abs_of_w0"], 16)
    assert J["final_exponent_last_chunk_w0_is_neg"] is False and (p * p - p + 1) // r == m1 * p + w0 and (m1, w0) == (1, T)
    assert (p ** 6 - 1) // r == (p ** 3 - 1) * (p + 1) * (p + T)
    w0n = J["w0_naf"]
    assert w0n == naf + [1] and sum(d << i for i, d in enumerate(w0n)) == w0
    assert J["nonresidue"] == 11 and pow(11, (p - 1) // 2, p) == p - 1 and pow(11, (p - 1) // 3, p) != 1   # neither a square nor a cube
    c1 = [pow(11, (p ** i - 1) // 3, p) for i in range(3)]
    assert [int(v, 16) for v in J["frobenius_fq3_c1"]] == c1 and c1[0] == 1
    assert [int(v, 16) for v in J["frobenius_fq3_c2"]] == [v * v % p for v in c1]
    assert [int(v, 16) for v in J["frobenius_fq6_c1"]] == [pow(11, (p ** i - 1) // 6, p) for i in range(6)]
    assert [int(v, 16) for v in J["twist"]] == [0, 1, 0]
    assert [int(v, 16) for v in J["twist_coeff_a"]] == [0, 0, C1.a[0]] == list(C2.a) and C1.a[0] == 11
    hdr = open(os.path.join(ROOT, "ginger-lib_amd", "csrc", "pairing_constants_gen.h")).read()
    digits = lambda name: [int(t) for t in re.search(r"#define %s \{(.*?)\}" % name, hdr).group(1).split(",")]
    assert digits("GH_MNT6_ATE_NAF") == naf[::-1] and digits("GH_MNT6_W0_NAF") == w0n[::-1]
    assert "#define GH_MNT6_ATE_DIGITS 376" in hdr and "#define GH_MNT6_ATE_NONZERO 123" in hdr and "#define GH_MNT6_W0_DIGITS 377" in hdr
    for key, name in (("frobenius_fq3_c1", "GH_MNT6_FROB3_C1"), ("frobenius_fq3_c2", "GH_MNT6_FROB3_C2"), ("frobenius_fq6_c1", "GH_MNT6_FROB6_C1")):
        for i, v in enumerate(J[key]):
            words = [int(t.rstrip("u"), 16) for t in re.search(r"#define %s_%d_I29 \{(.*?)\}" % (name, i), hdr).group(1).split(",")]
            assert sum(w << (29 * k) for k, w in enumerate(words)) == int(v, 16) * pow(2, 754, p) % p, (name, i)
    assert "#define GH_PAIRING_MNT6753 2" in open(os.path.join(ROOT, "include", "ginger_hip_pairing.h")).read()


# ---- 6. the C ABI without a device
def _vk_arrays():
    gt = fq6_row(pr.ONE).reshape(1, 72)
    gamma, delta = g2_row(C2.mul(3, C2.G)).reshape(1, 72), g2_row(C2.mul(5, C2.G)).reshape(1, 72)
    abc = np.stack([g1_row(C1.mul(k, C1.G)) for k in (2, 7)])
    return gt, gamma, delta, abc


def test_engines_table(gl):
    from ginger_lib_amd import pairing
    assert pairing.ENGINES == {"mnt4753": 0, "mnt6753": MNT6}


def test_vk_create_checks_arguments(gl):
    from ginger_lib_amd import pairing
    lib = pairing._lib()
    gt, gamma, delta, abc = _vk_arrays()
    ptr = lambda a: a.ctypes.data_as(V)
    h = V()
    assert lib.gh_groth16_vk_create(MNT6, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_groth16_vk_free(h) == 0
    for args in ((None, ptr(gamma), ptr(delta), ptr(abc)), (ptr(gt), None, ptr(delta), ptr(abc)), (ptr(gt), ptr(gamma), None, ptr(abc)),
                 (ptr(gt), ptr(gamma), ptr(delta), None)):
        assert lib.gh_groth16_vk_create(MNT6, *args, 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_groth16_vk_create(MNT6, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, None) == GH_E_BAD_ARG
    for engine in (1, 7):                                                                                                 # no such engine
        assert lib.gh_groth16_vk_create(engine, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == GH_E_BAD_ARG
        assert "engine" in lib.gh_last_error().decode()
    assert lib.gh_groth16_vk_create(MNT6, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 0, ctypes.byref(h)) == GH_E_BAD_ARG  # n_abc = 0
    big = np.array(pyref.int_to_limbs(pr.p), dtype=np.uint64)                                                             # a coefficient = p
    for which in range(4):
        for at in ((0, 60) if which < 3 else (0, 36)):                                                                    # the first and the last coefficient
            arrs = [a.copy() for a in (gt, gamma, delta, abc)]
            arrs[which].reshape(-1)[at:at + 12] = big
            assert lib.gh_groth16_vk_create(MNT6, *[ptr(a) for a in arrs], 2, ctypes.byref(h)) == GH_E_BAD_ARG, (which, at)
            assert "modulus" in lib.gh_last_error().decode()
    off = gamma.copy()
    off[0, :12] = limbs(1234)                                                                                             # gamma off the curve
    assert lib.gh_groth16_vk_create(MNT6, ptr(gt), ptr(off), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert "curve" in lib.gh_last_error().decode()
    off1 = abc.copy()
    off1[1, 12:24] = limbs(99)                                                                                            # an abc point off the curve
    assert lib.gh_groth16_vk_create(MNT6, ptr(gt), ptr(gamma), ptr(delta), ptr(off1), 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert "curve" in lib.gh_last_error().decode()
    with pytest.raises(pairing.GingerHipError):
        pairing.PreparedVerifyingKey(gt, off, delta, abc, engine="mnt6753")
    with pytest.raises(ValueError):                                                                                       # MNT4-sized rows
        pairing.PreparedVerifyingKey(gt[:, :48], gamma, delta, abc, engine="mnt6753")


def test_compute_entry_points_without_gpu(gl):
    """n == 0 is a no-op, bad arguments are GH_E_BAD_ARG before any device work, and without a device the compute entry points
    return GH_E_NO_DEVICE; creating a key needs no device."""
    from ginger_lib_amd import pairing
    lib = pairing._lib()
    pvk = pairing.PreparedVerifyingKey(*_vk_arrays(), engine="mnt6753")
    assert pvk.num_inputs == 1 and pvk.engine == "mnt6753"
    h = pvk.handle
    x = np.zeros((4, 72), dtype=np.uint64)
    b = np.zeros(16, dtype=np.uint8)
    p, pb = x.ctypes.data_as(V), b.ctypes.data_as(V)
    assert lib.gh_pairing_product(MNT6, p, pb, p, pb, 0, 1, p) == 0
    assert lib.gh_pairing_product(MNT6, None, None, None, None, 0, 3, None) == 0
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 0, 1, pb) == 0
    for engine in (1, 7):
        assert lib.gh_pairing_product(engine, p, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    for k in (0, 4):
        assert lib.gh_pairing_product(MNT6, p, pb, p, pb, 1, k, p) == GH_E_BAD_ARG
    assert lib.gh_pairing_product(MNT6, None, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 0, pb) == GH_E_BAD_ARG          # n_inputs + 1 != n_abc
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 2, pb) == GH_E_BAD_ARG
    assert "MalformedVerifyingKey" in lib.gh_last_error().decode()
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, None, 1, 1, pb) == GH_E_BAD_ARG
    bad = np.zeros((2, 72), dtype=np.uint64)
    bad[0, 60:72] = pyref.int_to_limbs(pr.p)                                                    # the sixth coefficient of a G2 point = p
    pbad = bad.ctypes.data_as(V)
    assert lib.gh_pairing_product(MNT6, p, pb, pbad, pb, 1, 1, p) == GH_E_BAD_ARG
    assert lib.gh_groth16_verify(h, p, pb, pbad, pb, p, pb, p, 1, 1, pb) == GH_E_BAD_ARG
    bad1 = np.zeros((2, 72), dtype=np.uint64)
    bad1[0, 12:24] = pyref.int_to_limbs(pr.p)                                                   # y of a G1 point = p
    pbad1 = bad1.ctypes.data_as(V)
    assert lib.gh_pairing_product(MNT6, pbad1, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    for pos in (0, 2):
        args = [p, pb, p, pb, p, pb]
        args[2 * pos] = pbad1
        assert lib.gh_groth16_verify(h, *args, p, 1, 1, pb) == GH_E_BAD_ARG, pos
    rbad = np.zeros((1, 12), dtype=np.uint64)
    rbad[0] = pyref.int_to_limbs(pr.r)                                                          # a public input = r
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, rbad.ctypes.data_as(V), 1, 1, pb) == GH_E_BAD_ARG
    assert "public input" in lib.gh_last_error().decode()
    rok = np.zeros((1, 12), dtype=np.uint64)
    rok[0] = pyref.int_to_limbs(pr.r - 1)                                                       # below r (r < p: MNT4's engine refuses it)
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:                                                  # the library's own verdict
        assert lib.gh_pairing_product(MNT6, p, pb, p, pb, 1, 1, p) == GH_E_NO_DEVICE
        assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 1, pb) == GH_E_NO_DEVICE
        assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, rok.ctypes.data_as(V), 1, 1, pb) == GH_E_NO_DEVICE
        with pytest.raises(pairing.GingerHipError):
            pairing.pairing_product((x[:1, :24], b[:1]), (x[:1], b[:1]), engine="mnt6753")
    pvk.close()


def test_wire_helpers_round_trip():
    """Proof::write records -> limb rows over MNT6-753 Fq, and an Fq6 row -> the bytes of Fp6::write"""
    from ginger_lib_amd import pairing
    P, Q, want = pr.kat()
    rec = b"".join(v.to_bytes(96, "little") for v in Q[0] + Q[1]) + b"\x00"
    assert len(rec) == 577
    xy, inf = pairing._wire_rows(rec + bytes(576) + b"\x01", 577, 6, "mnt6753")
    assert list(xy[0]) == list(g2_row(Q)) and list(inf) == [0, 1]
    assert pairing.gt_to_bytes(fq6_row(want), "mnt6753") == b"".join(v.to_bytes(96, "little") for v in pr.tower(want))
    with pytest.raises(ValueError):
        pairing._wire_rows(pr.p.to_bytes(96, "little") + bytes(97), 193, 2, "mnt6753")
    assert pr.r < pr.p                                                                          # r is a valid MNT6 coordinate, not an MNT4 one
    pairing._wire_rows(pr.r.to_bytes(96, "little") + bytes(97), 193, 2, "mnt6753")
    with pytest.raises(ValueError):
        pairing._wire_rows(pr.r.to_bytes(96, "little") + bytes(97), 193, 2)
