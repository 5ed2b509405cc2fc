"""The MNT4-753 and MNT6-753 pairings without a GPU, every engine test once per engine object of tests/pairing_ref.py: the Python
restatement against the reference's known answer, the GH_HD code of ginger-lib_amd/csrc/pairing29.h and pairing29_mnt6.h compiled
by g++ (tests/host_shim/pairing_shim.cpp) against both, the generated constants re-derived from p and r, and the argument checks
/ exports of include/ginger_hip_pairing.h and of its Rust extern block.  Every comparison is exact integer equality.

An engine test is written once, as check_<name>(..., pr), and run by two tests at the end of the file: test_<name> over MNT4-753
and test_<name>_mnt6 over MNT6-753 (the tower test: test_shim_fq4_arithmetic / test_shim_fq6_arithmetic)."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import pairing_ref
import pyref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_BAD_ARG, GH_E_NO_DEVICE = -1, -3
V = ctypes.c_void_p
# the shim's tower operations (tests/host_shim/pairing_shim.cpp)
OP_MUL, OP_SQR, OP_INV, OP_CYC_SQR, OP_CYC_EXP, OP_SPARSE, OP_UNITARY_INV, OP_FINAL_EXP, OP_FROBENIUS = range(9)


M4, M6 = pairing_ref.engine("mnt4753"), pairing_ref.engine("mnt6753")


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("pairing")
    I = ctypes.c_int
    lib.t_pairing_product.argtypes = [I, V, V, V, V, I, V]
    lib.t_pairing_prepared.argtypes = [I, V, V, V]
    lib.t_gt_op.argtypes = [I, I, V, V, V]
    return lib


def shim_product(shim, pr, pairs):
    k = len(pairs)
    a = np.ascontiguousarray(np.concatenate([pr.g1_row(P) for P, _ in pairs]))
    b = np.ascontiguousarray(np.concatenate([pr.g2_row(Q) for _, Q in pairs]))
    ai = np.array([P is None for P, _ in pairs], dtype=np.uint8)
    bi = np.array([Q is None for _, Q in pairs], dtype=np.uint8)
    out = np.zeros(pr.gt_words, dtype=np.uint64)
    assert shim.t_pairing_product(pr.id, a.ctypes.data, ai.ctypes.data, b.ctypes.data, bi.ctypes.data, k, out.ctypes.data) == 0
    return pr.gt_of(out)


def shim_op(shim, pr, op, a, b=None):
    x, y = pr.gt_row(a), pr.gt_row(b if b is not None else pr.ONE)
    out = np.zeros(pr.gt_words, dtype=np.uint64)
    assert shim.t_gt_op(pr.id, op, x.ctypes.data, y.ctypes.data, out.ctypes.data) == 0
    return pr.gt_of(out)


# ---- 1. the restatement against the reference's known answer (curves/mnt4753/tests.rs:266-467, curves/mnt6753/tests.rs:319-590)
def check_restatement_equals_the_known_answer(pr):
    P, Q, want = pr.kat()
    assert pr.C1.on_curve(P) and pr.C2.on_curve(Q)
    got = pr.pairing(P, Q)
    assert got == want
    assert got != pr.ONE and pr.fpow(got, pr.r) == pr.ONE


# ---- 2. the device's arithmetic on the host against the known answer: all k Fq words
def check_shim_pairing_equals_the_known_answer(shim, pr):
    P, Q, want = pr.kat()
    got = shim_product(shim, pr, [(P, Q)])
    assert pr.tower(got) == pr.tower(want)
    a, b, out = pr.g1_row(P), pr.g2_row(Q), np.zeros(pr.gt_words, dtype=np.uint64)
    assert shim.t_pairing_prepared(pr.id, a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0      # the prepared-Q steps
    assert pr.gt_of(out) == want
    for engine in (1, 7):                                            # no such engine
        assert shim.t_pairing_prepared(engine, a.ctypes.data, b.ctypes.data, out.ctypes.data) != 0


# ---- 3. the shim against the restatement
def check_shim_agrees_with_the_restatement(shim, pr):
    C1, C2 = pr.C1, pr.C2
    rng = random.Random({"mnt4753": 753, "mnt6753": 6753}[pr.name])
    for _ in range(3):
        P, Q = C1.mul(rng.randrange(1, pr.r), C1.G), C2.mul(rng.randrange(1, pr.r), C2.G)
        assert shim_product(shim, pr, [(P, Q)]) == pr.pairing(P, Q)
    P, Q = C1.mul(5, C1.G), C2.mul(7, C2.G)
    pairs = [(P, Q), (C1.neg(P), Q)]
    assert pr.product(pairs) == pr.ONE
    assert shim_product(shim, pr, pairs) == pr.ONE                   # e(P, Q) e(-P, Q) = 1 under one final exponentiation
    assert shim_product(shim, pr, [(None, Q)]) == pr.ONE == pr.product([(None, Q)])
    assert shim_product(shim, pr, [(P, None)]) == pr.ONE == pr.product([(P, None)])
    three = [(P, Q), (None, Q), (C1.G, C2.G)]
    assert shim_product(shim, pr, three) == pr.product(three)


# ---- 4. the tower
def check_shim_tower_arithmetic(shim, pr):
    k, d = pr.k, pr.k // 2
    rng = random.Random(k)
    rnd = lambda: [rng.randrange(pr.p) for _ in range(k)]
    for _ in range(3):
        a, b = rnd(), rnd()
        assert shim_op(shim, pr, OP_MUL, a, b) == pr.mul(a, b)
        assert shim_op(shim, pr, OP_SQR, a) == pr.mul(a, a)
        assert shim_op(shim, pr, OP_INV, a) == pr.inv(a) and pr.mul(a, pr.inv(a)) == pr.ONE
        for j in range(1, k):
            assert shim_op(shim, pr, OP_FROBENIUS + j, a) == pr.frobenius(a, j), j
        assert shim_op(shim, pr, OP_UNITARY_INV, a) == pr.from_tower([v if i < d else (-v) % pr.p for i, v in enumerate(pr.tower(a))])
        if k == 4:
            sparse = pr.from_tower([b[0], 0, b[2], b[3]])            # mul_by_023
            u = pr.mul(pr.frobenius(a, 2), pr.inv(a))                # after the easy part: norm one over Fq2
            w0 = pr.T - 1
        else:
            sparse = pr.from_tower([0, 0, b[0], b[1], b[2], b[3]])   # mul_by_2345: [c0: (0, 0, a), c1: full]
            u = pr.fpow(a, (pr.p ** 3 - 1) * (pr.p + 1))             # after the easy part: norm one over Fq3
            assert pr.mul(u, pr.frobenius(u, 3)) == pr.ONE
            w0 = pr.T
        assert shim_op(shim, pr, OP_SPARSE, a, sparse) == pr.mul(a, sparse)
        assert shim_op(shim, pr, OP_CYC_SQR, u) == pr.mul(u, u)
        assert shim_op(shim, pr, OP_CYC_EXP, u) == pr.fpow(u, w0)
        assert shim_op(shim, pr, OP_FINAL_EXP, a) == pr.final_exponentiation(a)
    assert shim_op(shim, pr, OP_INV, pr.ZERO) == pr.ZERO             # the inverse of zero is zero
    assert shim_op(shim, pr, OP_FINAL_EXP, pr.ZERO) == pr.ZERO
    assert shim_op(shim, pr, OP_MUL, pr.ONE, pr.ONE) == pr.ONE
    x = pr.gt_row(pr.ONE)
    for op in (-1, OP_FROBENIUS, OP_FROBENIUS + k):                  # Frobenius powers 1 .. k - 1 only
        assert shim.t_gt_op(pr.id, op, x.ctypes.data, x.ctypes.data, x.ctypes.data) != 0
    assert shim.t_gt_op(1, OP_MUL, x.ctypes.data, x.ctypes.data, x.ctypes.data) != 0        # no such engine


# ---- 5. the constants
def check_constants_rederived_from_p_and_r(pr):
    golden = lambda name: json.load(open(os.path.join(ROOT, "tests", "golden", name)))
    J4 = golden("pairing_constants.json")
    J = J4 if pr.k == 4 else golden("pairing6_constants.json")
    p, r, T, NR, C1, C2 = pr.p, pr.r, pr.T, pr.NR, pr.C1, pr.C2
    ints = lambda key: [int(v, 16) for v in J[key]]
    naf, w0n = J["ate_naf"], J["w0_naf"]
    m1, w0 = int(J["final_exponent_last_chunk_1"], 16), int(J["final_exponent_last_chunk_abs_of_w0"], 16)
    assert int(J["ate_loop_count"], 16) == T and T > 0 and T.bit_length() == 377
    assert len(naf) == 376 and sum(1 for d in naf if d) == 123 and set(naf) <= {-1, 0, 1}
    assert all(not (x and y) for x, y in zip(naf, naf[1:] + [1]))                         # non-adjacent, the leading 1 included
    assert sum(d << i for i, d in enumerate(naf)) + (1 << len(naf)) == T
    assert sum(d << i for i, d in enumerate(w0n)) == w0
    assert J["nonresidue"] == NR and pow(NR, (p - 1) // 2, p) == p - 1                    # NR is a non-residue
    if pr.k == 4:
        assert T == r - p and J["ate_is_loop_count_neg"] is True
        assert (p * p + 1) % r == 0
        assert J["final_exponent_last_chunk_w0_is_neg"] is True and (p * p + 1) // r == m1 * p - w0 and (m1, w0) == (1, T - 1)
        assert (p ** 4 - 1) // r == (p * p - 1) * (m1 * p - w0)
        assert set(w0n) <= {-1, 0, 1} and w0n[-1] == 1
        assert all(not (x and y) for x, y in zip(w0n, w0n[1:]))
        assert ints("frobenius_fq2_c1") == [pow(13, (p ** i - 1) // 2, p) for i in range(2)] == [1, p - 1]
        assert ints("frobenius_fq4_c1") == [pow(13, (p ** i - 1) // 4, p) for i in range(4)]
        assert ints("twist") == [0, 1]
        assert ints("twist_coeff_a") == [C1.a[0] * 13 % p, 0] == list(C2.a)
        tables = (("frobenius_fq4_c1", "GH_MNT4_FROB4_C1"),)
    else:
        assert p == pyref.P6.p and r == pyref.P4.p
        assert T == p - r and J["ate_is_loop_count_neg"] is False
        assert T == int(J4["ate_loop_count"], 16)                                         # the same integer as MNT4's |T|
        assert naf == J4["ate_naf"]
        assert (p * p - p + 1) % r == 0
        assert J["final_exponent_last_chunk_w0_is_neg"] is False and (p * p - p + 1) // r == m1 * p + w0 and (m1, w0) == (1, T)
        assert (p ** 6 - 1) // r == (p ** 3 - 1) * (p + 1) * (p + T)
        assert w0n == naf + [1]
        assert pow(11, (p - 1) // 3, p) != 1                                              # nor a cube
        c1 = [pow(11, (p ** i - 1) // 3, p) for i in range(3)]
        assert ints("frobenius_fq3_c1") == c1 and c1[0] == 1
        assert ints("frobenius_fq3_c2") == [v * v % p for v in c1]
        assert ints("frobenius_fq6_c1") == [pow(11, (p ** i - 1) // 6, p) for i in range(6)]
        assert ints("twist") == [0, 1, 0]
        assert ints("twist_coeff_a") == [0, 0, C1.a[0]] == list(C2.a) and C1.a[0] == 11
        tables = (("frobenius_fq3_c1", "GH_MNT6_FROB3_C1"), ("frobenius_fq3_c2", "GH_MNT6_FROB3_C2"), ("frobenius_fq6_c1", "GH_MNT6_FROB6_C1"))
    hdr = open(os.path.join(ROOT, "ginger-lib_amd", "csrc", "pairing_constants_gen.h")).read()
    tag = "GH_MNT%d" % pr.k
    digits = lambda name: [int(t) for t in re.search(r"#define %s \{(.*?)\}" % name, hdr).group(1).split(",")]
    assert digits(tag + "_ATE_NAF") == naf[::-1] and digits(tag + "_W0_NAF") == w0n[::-1]
    assert "#define %s_ATE_DIGITS 376" % tag in hdr and "#define %s_ATE_NONZERO 123" % tag in hdr
    for key, name in tables:
        for i, v in enumerate(J[key]):
            words = [int(t.rstrip("u"), 16) for t in re.search(r"#define %s_%d_I29 \{(.*?)\}" % (name, i), hdr).group(1).split(",")]
            assert sum(w << (29 * j) for j, w in enumerate(words)) == int(v, 16) * pow(2, 754, p) % p, (name, i)
    if pr.k == 6:
        assert "#define GH_MNT6_W0_DIGITS 377" in hdr
        assert "#define GH_PAIRING_MNT6753 2" in open(os.path.join(ROOT, "include", "ginger_hip_pairing.h")).read()


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


def test_engines_table(gl):
    from ginger_lib_amd import pairing
    assert pairing.ENGINES == {"mnt4753": 0, "mnt6753": 2}
    assert pairing.ENGINES == {name: pairing_ref.engine(name).id for name in pairing_ref.ENGINES}


def test_last_timing_checks_arguments(gl):
    from ginger_lib_amd import pairing
    lib = pairing._lib()
    buf = (ctypes.c_float * 6)()
    tot = ctypes.c_float()
    assert lib.gh_pairing_last_timing(buf, 6, ctypes.byref(tot)) == 6
    assert lib.gh_pairing_last_timing(None, 3, None) == GH_E_BAD_ARG


def test_vk_free_of_null(gl):
    from ginger_lib_amd import pairing
    assert pairing._lib().gh_groth16_vk_free(None) == 0


def _vk_arrays(pr):
    C1, C2 = pr.C1, pr.C2
    gt = pr.gt_row(pr.ONE).reshape(1, -1)
    gamma, delta = pr.g2_row(C2.mul(3, C2.G)).reshape(1, -1), pr.g2_row(C2.mul(5, C2.G)).reshape(1, -1)
    abc = np.stack([pr.g1_row(C1.mul(k, C1.G)) for k in (2, 7)])
    return gt, gamma, delta, abc


def check_vk_create_checks_arguments(gl, pr):
    from ginger_lib_amd import pairing
    lib = pairing._lib()
    gt, gamma, delta, abc = _vk_arrays(pr)
    ptr = lambda a: a.ctypes.data_as(V)
    h = V()
    assert lib.gh_groth16_vk_create(pr.id, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_groth16_vk_free(h) == 0
    for args in ((None, ptr(gamma), ptr(delta), ptr(abc)), (ptr(gt), None, ptr(delta), ptr(abc)), (ptr(gt), ptr(gamma), None, ptr(abc)),
                 (ptr(gt), ptr(gamma), ptr(delta), None)):
        assert lib.gh_groth16_vk_create(pr.id, *args, 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_groth16_vk_create(pr.id, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, None) == GH_E_BAD_ARG
    for engine in (1, 7):                                                                                                 # no such engine
        assert lib.gh_groth16_vk_create(engine, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == GH_E_BAD_ARG
        assert "engine" in lib.gh_last_error().decode()
    assert lib.gh_groth16_vk_create(pr.id, ptr(gt), ptr(gamma), ptr(delta), ptr(abc), 0, ctypes.byref(h)) == GH_E_BAD_ARG # n_abc = 0
    big = np.array(pyref.int_to_limbs(pr.p), dtype=np.uint64)                                                             # a coefficient = p
    for which in range(4):
        for at in ((0, 12 * (pr.k - 1)) if which < 3 else (0, 36)):                                                       # the first and the last coefficient
            arrs = [a.copy() for a in (gt, gamma, delta, abc)]
            arrs[which].reshape(-1)[at:at + 12] = big
            assert lib.gh_groth16_vk_create(pr.id, *[ptr(a) for a in arrs], 2, ctypes.byref(h)) == GH_E_BAD_ARG, (which, at)
            assert "modulus" in lib.gh_last_error().decode()
    off = gamma.copy()
    off[0, :12] = pr.limbs(1234)                                                                                          # gamma off the curve
    assert lib.gh_groth16_vk_create(pr.id, ptr(gt), ptr(off), ptr(delta), ptr(abc), 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert "curve" in lib.gh_last_error().decode()
    off1 = abc.copy()
    off1[1, 12:24] = pr.limbs(99)                                                                                         # an abc point off the curve
    assert lib.gh_groth16_vk_create(pr.id, ptr(gt), ptr(gamma), ptr(delta), ptr(off1), 2, ctypes.byref(h)) == GH_E_BAD_ARG
    assert "curve" in lib.gh_last_error().decode()
    with pytest.raises(pairing.GingerHipError):
        pairing.PreparedVerifyingKey(gt, off, delta, abc, engine=pr.name)
    other = pairing_ref.engine([name for name in pairing_ref.ENGINES if name != pr.name][0])
    with pytest.raises(ValueError):                                                                                       # rows of the other engine's width
        pairing.PreparedVerifyingKey(other.gt_row(other.ONE).reshape(1, -1), gamma, delta, abc, engine=pr.name)


def check_compute_entry_points_without_gpu(gl, pr):
    """n == 0 is a no-op, bad arguments are GH_E_BAD_ARG before any device work, and without a device the compute entry points
    return GH_E_NO_DEVICE; creating a key needs no device."""
    from ginger_lib_amd import pairing
    lib = pairing._lib()
    E, w = pr.id, pr.gt_words
    pvk = pairing.PreparedVerifyingKey(*_vk_arrays(pr), engine=pr.name)
    assert pvk.num_inputs == 1 and pvk.engine == pr.name
    h = pvk.handle
    x = np.zeros((4, w), dtype=np.uint64)
    b = np.zeros(16, dtype=np.uint8)
    p, pb = x.ctypes.data_as(V), b.ctypes.data_as(V)
    assert lib.gh_pairing_product(E, p, pb, p, pb, 0, 1, p) == 0
    assert lib.gh_pairing_product(E, None, None, None, None, 0, 3, None) == 0
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 0, 1, pb) == 0
    for engine in (1, 7):
        assert lib.gh_pairing_product(engine, p, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    for k in (0, 4):
        assert lib.gh_pairing_product(E, p, pb, p, pb, 1, k, p) == GH_E_BAD_ARG
    assert lib.gh_pairing_product(E, None, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 0, pb) == GH_E_BAD_ARG          # n_inputs + 1 != n_abc
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 2, pb) == GH_E_BAD_ARG
    assert "MalformedVerifyingKey" in lib.gh_last_error().decode()
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, None, 1, 1, pb) == GH_E_BAD_ARG
    assert lib.gh_groth16_verify(None, p, pb, p, pb, p, pb, p, 1, 1, pb) < 0

    def with_p_at(at):
        bad = np.zeros((2, w), dtype=np.uint64)
        bad[0, at:at + 12] = pyref.int_to_limbs(pr.p)
        return bad
    # a coordinate = p: the first coefficient of any point, y of a G1 point, the last coefficient of a G2 point
    for bad, g1, g2, positions in ((with_p_at(0), True, True, (0, 1, 2)), (with_p_at(12), True, False, (0, 2)), (with_p_at(w - 12), False, True, (1,))):
        pbad = bad.ctypes.data_as(V)
        if g1:
            assert lib.gh_pairing_product(E, pbad, pb, p, pb, 1, 1, p) == GH_E_BAD_ARG
        if g2:
            assert lib.gh_pairing_product(E, p, pb, pbad, pb, 1, 1, p) == GH_E_BAD_ARG
        for pos in positions:
            args = [p, pb, p, pb, p, pb]
            args[2 * pos] = pbad
            assert lib.gh_groth16_verify(h, *args, p, 1, 1, pb) == GH_E_BAD_ARG, pos
            assert "modulus" in lib.gh_last_error().decode()
    rbad = np.zeros((1, 12), dtype=np.uint64)
    rbad[0] = pyref.int_to_limbs(pr.r)                                                          # a public input = r
    assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, rbad.ctypes.data_as(V), 1, 1, pb) == GH_E_BAD_ARG
    assert "public input" in lib.gh_last_error().decode()
    rok = np.zeros((1, 12), dtype=np.uint64)
    rok[0] = pyref.int_to_limbs(pr.r - 1)                                                       # below r (MNT6: r < p, MNT4's engine refuses it)
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:                                                  # the library's own verdict
        assert lib.gh_pairing_product(E, p, pb, p, pb, 1, 1, p) == GH_E_NO_DEVICE
        assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, p, 1, 1, pb) == GH_E_NO_DEVICE
        if pr.name == "mnt6753":
            assert lib.gh_groth16_verify(h, p, pb, p, pb, p, pb, rok.ctypes.data_as(V), 1, 1, pb) == GH_E_NO_DEVICE
        with pytest.raises(pairing.GingerHipError):
            pairing.pairing_product((x[:1, :24], b[:1]), (x[:1], b[:1]), engine=pr.name)
    pvk.close()


def test_package_pairing_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "pairing.py")).read()
    for needle in ("tests/", "import pyref", "pairing_ref", "groth16_ref", "oracle"):
        assert needle not in txt, needle


def check_wire_helpers_round_trip(pr):
    """Proof::write records of G1 (193 bytes) and G2 (385 / 577 bytes) -> limb rows over the engine's Fq, and an Fq^k row -> the
    bytes of Fp4::write / Fp6::write"""
    from ginger_lib_amd import pairing
    P, Q, want = pr.kat()
    rec = P[0][0].to_bytes(96, "little") + P[1][0].to_bytes(96, "little") + b"\x00"
    xy, inf = pairing._wire_rows(rec + bytes(192) + b"\x01", 193, 2, pr.name)
    assert list(xy[0]) == list(pr.g1_row(P)) and list(inf) == [0, 1]
    rec = b"".join(v.to_bytes(96, "little") for v in Q[0] + Q[1]) + b"\x00"
    assert len(rec) == {"mnt4753": 385, "mnt6753": 577}[pr.name]
    xy, inf = pairing._wire_rows(rec + bytes(len(rec) - 1) + b"\x01", len(rec), pr.k, pr.name)
    assert list(xy[0]) == list(pr.g2_row(Q)) and list(inf) == [0, 1]
    assert pairing.gt_to_bytes(pr.gt_row(want), pr.name) == b"".join(v.to_bytes(96, "little") for v in pr.tower(want))
    with pytest.raises(ValueError):
        pairing._wire_rows(pr.p.to_bytes(96, "little") + bytes(97), 193, 2, pr.name)
    if pr.name == "mnt6753":
        assert pr.r < pr.p                                                                      # r is a valid MNT6 coordinate, not an MNT4 one
        pairing._wire_rows(pr.r.to_bytes(96, "little") + bytes(97), 193, 2, "mnt6753")
        with pytest.raises(ValueError):
            pairing._wire_rows(pr.r.to_bytes(96, "little") + bytes(97), 193, 2)


# ---- every engine test above, once per engine
def test_restatement_equals_the_known_answer():
    check_restatement_equals_the_known_answer(M4)


def test_restatement_equals_the_known_answer_mnt6():
    check_restatement_equals_the_known_answer(M6)


def test_shim_pairing_equals_the_known_answer(shim):
    check_shim_pairing_equals_the_known_answer(shim, M4)


def test_shim_pairing_equals_the_known_answer_mnt6(shim):
    check_shim_pairing_equals_the_known_answer(shim, M6)


def test_shim_agrees_with_the_restatement(shim):
    check_shim_agrees_with_the_restatement(shim, M4)


def test_shim_agrees_with_the_restatement_mnt6(shim):
    check_shim_agrees_with_the_restatement(shim, M6)


def test_shim_fq4_arithmetic(shim):
    check_shim_tower_arithmetic(shim, M4)


def test_shim_fq6_arithmetic(shim):
    check_shim_tower_arithmetic(shim, M6)


def test_constants_rederived_from_p_and_r():
    check_constants_rederived_from_p_and_r(M4)


def test_constants_rederived_from_p_and_r_mnt6():
    check_constants_rederived_from_p_and_r(M6)


def test_vk_create_checks_arguments(gl):
    check_vk_create_checks_arguments(gl, M4)


def test_vk_create_checks_arguments_mnt6(gl):
    check_vk_create_checks_arguments(gl, M6)


def test_compute_entry_points_without_gpu(gl):
    check_compute_entry_points_without_gpu(gl, M4)


def test_compute_entry_points_without_gpu_mnt6(gl):
    check_compute_entry_points_without_gpu(gl, M6)


def test_wire_helpers_round_trip():
    check_wire_helpers_round_trip(M4)


def test_wire_helpers_round_trip_mnt6():
    check_wire_helpers_round_trip(M6)


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
