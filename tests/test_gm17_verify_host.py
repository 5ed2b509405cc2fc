"""GM17 verification without a GPU: the literal restatement of verifier.rs (tests/gm17_verify_ref.py) against the closed form
of a key known in the exponent, the GH_HD group additions of ginger-lib_amd/csrc/gm17_sum.h compiled by g++
(tests/host_shim/gm17_shim.cpp) against pyref's curve add and, composed with the shim's Miller loop and final exponentiation,
against the closed form, and the argument checks of include/ginger_hip_gm17.h.  Every comparison is exact."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import gm17_verify_ref as R
import pairing_ref
import pyref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_BAD_ARG, GH_E_NO_DEVICE = -1, -3
V = ctypes.c_void_p


@pytest.fixture(scope="module", params=pairing_ref.ENGINES)
def pr(request):
    return pairing_ref.engine(request.param)


@pytest.fixture(scope="module")
def edge(pr):
    key = R.ExpKey(pr, 1701)
    rows, expected, tests = R.edge_rows(key)
    return {"key": key, "rows": rows, "expected": expected, "tests": tests}


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("gm17")
    I = ctypes.c_int
    lib.t_gm17_sum_g1.argtypes = lib.t_gm17_sum_g2.argtypes = [I, V, I, V, I, V, V]
    lib.t_gm17_row.argtypes = [I, V, V, V, V, V, V, I, V, I, V, I, V, I, ctypes.POINTER(I)]
    return lib


# ---- 1. the restatement against the closed form
def test_restatement_equals_the_closed_form(pr, edge):
    key = edge["key"]
    got = [2 if not R.on_curves(pr, row[:3]) else int(R.gm17_verify(pr, key.vk, row[:3], row[3])) for row in edge["rows"]]
    assert got == edge["expected"]
    assert R.gm17_verify(pr, key.vk, edge["rows"][0][:3], edge["rows"][0][3][:1]) is None          # MalformedVerifyingKey


# ---- 2. the device's group additions on the host
def _shim_sum(shim, pr, g2, P, Q):
    eng = pr.id
    row = pr.g2_row if g2 else pr.g1_row
    p, q = np.ascontiguousarray(row(P)), np.ascontiguousarray(row(Q))
    out, inf = np.zeros_like(p), np.zeros(1, dtype=np.uint8)
    fn = shim.t_gm17_sum_g2 if g2 else shim.t_gm17_sum_g1
    assert fn(eng, p.ctypes.data, int(P is None), q.ctypes.data, int(Q is None), out.ctypes.data, inf.ctypes.data) == 0
    return [int(v) for v in out], int(inf[0])


@pytest.mark.parametrize("g2", [False, True])
def test_shim_sums_equal_the_curve_add(shim, pr, g2):
    C = pr.C2 if g2 else pr.C1
    row = pr.g2_row if g2 else pr.g1_row
    rng = random.Random(1702 + g2)
    pt = lambda: C.mul(rng.randrange(1, 1 << 64), C.G)
    P, Q = pt(), pt()
    cases = [(P, Q), (P, P), (P, C.neg(P)), (None, Q), (P, None), (None, None)] + [(pt(), pt()) for _ in range(20)]
    for k, (X, Y) in enumerate(cases):
        want = C.add(X, Y)
        assert (k in (2, 5)) == (want is None)
        assert C.on_curve(want)
        xy, inf = _shim_sum(shim, pr, g2, X, Y)
        assert inf == int(want is None), k
        assert xy == [int(v) for v in row(want)], k                  # a sum at infinity carries zero coordinates, as row(None)
    assert C.add(P, P) == C.mul(2, P)


def test_shim_verdict_equals_the_closed_form(shim, pr, edge):
    """one row's verdict composed on the host: the shim's sums, Miller loop and final exponentiation"""
    key = edge["key"]
    vk, C1 = key.vk, pr.C1
    eng = pr.id
    keep = [np.ascontiguousarray(a) for a in (pr.g1_row(vk["g_alpha_g1"]), pr.g2_row(vk["h_beta_g2"]), pr.g1_row(vk["g_gamma_g1"]),
                                              pr.g2_row(vk["h_gamma_g2"]), pr.g2_row(vk["h_g2"]))]
    got, bits = [], []
    for A, B, C, s in edge["rows"]:
        if not R.on_curves(pr, (A, B, C)):
            got.append(2)
            bits.append(None)
            continue
        psi = vk["query"][0]
        for x, q in zip(s, vk["query"][1:]):
            psi = C1.add(psi, C1.mul(x % pr.r, q))
        arrs = [np.ascontiguousarray(a) for a in (pr.g1_row(A), pr.g2_row(B), pr.g1_row(C), pr.g1_row(psi))]
        t = ctypes.c_int(-1)
        st = shim.t_gm17_row(eng, *[a.ctypes.data for a in keep], arrs[0].ctypes.data, int(A is None), arrs[1].ctypes.data, int(B is None),
                             arrs[2].ctypes.data, int(C is None), arrs[3].ctypes.data, int(psi is None), ctypes.byref(t))
        got.append(st)
        bits.append((bool(t.value & 1), bool(t.value & 2)))
    assert got == edge["expected"]
    assert bits == edge["tests"]                                     # which of the two tests fails, row by row


def test_sanitized_standalone_check(tmp_path):
    """the same additions on their degenerate cases as a program of its own under the host sanitizers (gm17_sum_check.cpp)"""
    out = shim_build.sanitized_check("gm17_sum_check.cpp", str(tmp_path / "gm17_sum_check"))
    assert out.returncode == 0 and (out.stdout + out.stderr).strip().endswith("ok"), (out.stdout + out.stderr)[-2000:]


# ---- 3. the C ABI without a device
def _vk_arrays(pr):
    C1, C2 = pr.C1, pr.C2
    g1 = lambda k: pr.g1_row(C1.mul(k, C1.G)).reshape(1, 24)
    g2 = lambda k: pr.g2_row(C2.mul(k, C2.G)).reshape(1, -1)
    return [g1(2), g2(3), g1(5), g2(5), g2(1), np.concatenate([g1(7), g1(11)])]


def test_gm17_symbols_exported_and_kept_apart(gl):
    from ginger_lib_amd import ecvrf, gm17_verify, pairing, poseidon, schnorr
    lib = gl.load_library()
    assert len(gm17_verify.GM17_SYMBOLS) == 4
    for s in gm17_verify.GM17_SYMBOLS:
        assert hasattr(lib, s), s
    others = (gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS + schnorr.SCHNORR_SYMBOLS + ecvrf.ECVRF_SYMBOLS +
              pairing.PAIRING_SYMBOLS)
    assert not set(gm17_verify.GM17_SYMBOLS) & set(others)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_gm17.h")).read()
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(gm17_verify.GM17_SYMBOLS)
    assert len(gm17_verify.PHASES) == 9 and len(pairing.PAIRING_SYMBOLS) == 5


def test_rust_gm17_extern_block_is_generated_from_the_header():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    src = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")
    rs = open(os.path.join(src, "gm17.rs")).read()
    block = rs[rs.index("// ---- GENERATED by"):rs.index("// ---- GENERATED: end")]
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (gh_\w+)\((.*?)\)", block)}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ginger_hip_gm17.h")).read(), flags=re.S)
    c = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(gh_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)}
    assert sorted(rust) == sorted(c) and len(c) == 4
    for name, params in c.items():
        assert params.count(",") == rust[name].count(","), name
    assert "*mut GhGm17Vk" in block
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "pub mod gm17;" in lib[lib.index("// ---- GENERATED: end"):]
    assert "gh_gm17" not in lib


def test_vk_create_checks_arguments(gl, pr):
    from ginger_lib_amd import gm17_verify
    lib = gm17_verify._lib()
    eng = pr.id
    arrs = _vk_arrays(pr)
    ptr = lambda a: a.ctypes.data_as(V)
    h = V()
    assert lib.gh_gm17_vk_create(eng, *[ptr(a) for a in arrs], 2, ctypes.byref(h)) == 0 and h.value
    assert lib.gh_gm17_vk_free(h) == 0
    assert lib.gh_gm17_vk_free(None) == 0
    for which in range(6):                                                                      # each null pointer
        args = [ptr(a) for a in arrs]
        args[which] = None
        assert lib.gh_gm17_vk_create(eng, *args, 2, ctypes.byref(h)) == GH_E_BAD_ARG, which
    assert lib.gh_gm17_vk_create(eng, *[ptr(a) for a in arrs], 2, None) == GH_E_BAD_ARG
    for engine in (1, 7):                                                                       # no such engine
        assert lib.gh_gm17_vk_create(engine, *[ptr(a) for a in arrs], 2, ctypes.byref(h)) == GH_E_BAD_ARG
        assert "engine" in lib.gh_last_error().decode()
    assert lib.gh_gm17_vk_create(eng, *[ptr(a) for a in arrs], 0, ctypes.byref(h)) == GH_E_BAD_ARG   # n_query = 0
    big = np.array(pyref.int_to_limbs(pr.p), dtype=np.uint64)                                   # a coefficient = p
    for which in range(6):
        for at in (0, arrs[which].size - 12):                                                   # the first and the last coefficient
            bad = [a.copy() for a in arrs]
            bad[which].reshape(-1)[at:at + 12] = big
            assert lib.gh_gm17_vk_create(eng, *[ptr(a) for a in bad], 2, ctypes.byref(h)) == GH_E_BAD_ARG, (which, at)
            assert "modulus" in lib.gh_last_error().decode()
    for which, at in ((3, 0), (5, 24 + 12)):                                                    # h_gamma, query[1] off the curve
        bad = [a.copy() for a in arrs]
        bad[which].reshape(-1)[at:at + 12] = pr.limbs(1234)
        assert lib.gh_gm17_vk_create(eng, *[ptr(a) for a in bad], 2, ctypes.byref(h)) == GH_E_BAD_ARG, which
        assert "curve" in lib.gh_last_error().decode()
    for which in (0, 1, 2, 4):                                                                  # and every other point
        bad = [a.copy() for a in arrs]
        bad[which].reshape(-1)[:12] = pr.limbs(1234)
        assert lib.gh_gm17_vk_create(eng, *[ptr(a) for a in bad], 2, ctypes.byref(h)) == GH_E_BAD_ARG, which
        assert "curve" in lib.gh_last_error().decode()
    with pytest.raises(gm17_verify.GingerHipError):
        bad = [a.copy() for a in arrs]
        bad[3].reshape(-1)[:12] = pr.limbs(1234)
        gm17_verify.PreparedVerifyingKey(*bad, engine=pr.name)
    with pytest.raises(ValueError):                                                             # two g_alpha rows
        gm17_verify.PreparedVerifyingKey(np.concatenate([arrs[0], arrs[0]]), *arrs[1:], engine=pr.name)


def test_verify_entry_point_without_gpu(gl, pr):
    """n == 0 is a no-op, bad arguments are GH_E_BAD_ARG before any device work, and without a device gh_gm17_verify returns
    GH_E_NO_DEVICE; creating a key needs no device."""
    from ginger_lib_amd import gm17_verify
    lib = gm17_verify._lib()
    engine, w = pr.name, pr.gt_words
    pvk = gm17_verify.PreparedVerifyingKey(*_vk_arrays(pr), engine=engine)
    assert pvk.num_inputs == 1 and pvk.engine == engine
    h = pvk.handle
    x = np.zeros((4, w), dtype=np.uint64)
    b = np.zeros(16, dtype=np.uint8)
    p, pb = x.ctypes.data_as(V), b.ctypes.data_as(V)
    assert lib.gh_gm17_verify(h, p, pb, p, pb, p, pb, p, 0, 1, pb) == 0                         # n == 0
    assert lib.gh_gm17_verify(h, None, None, None, None, None, None, None, 0, 1, None) == 0
    for ni in (0, 2):                                                                           # n_inputs + 1 != n_query
        assert lib.gh_gm17_verify(h, p, pb, p, pb, p, pb, p, 1, ni, pb) == GH_E_BAD_ARG
        assert "MalformedVerifyingKey" in lib.gh_last_error().decode()
    assert lib.gh_gm17_verify(h, p, pb, p, pb, p, pb, p, 0, 2, pb) == GH_E_BAD_ARG              # even for no rows
    for pos in range(8):                                                                        # null pointers with n > 0
        args = [p, pb, p, pb, p, pb, p, pb]
        args[pos] = None
        assert lib.gh_gm17_verify(h, *args[:7], 1, 1, args[7]) == GH_E_BAD_ARG, pos
    assert lib.gh_gm17_verify(None, p, pb, p, pb, p, pb, p, 1, 1, pb) < 0
    for pos, at in ((0, 12), (1, w - 12), (2, 0)):                                              # a proof coordinate = p
        bad = np.zeros((2, w), dtype=np.uint64)
        bad[0, at:at + 12] = pyref.int_to_limbs(pr.p)
        args = [p, pb, p, pb, p, pb]
        args[2 * pos] = bad.ctypes.data_as(V)
        assert lib.gh_gm17_verify(h, *args, p, 1, 1, pb) == GH_E_BAD_ARG, pos
        assert "modulus" in lib.gh_last_error().decode()
    rbad = np.zeros((1, 12), dtype=np.uint64)
    rbad[0] = pyref.int_to_limbs(pr.r)                                                          # a public input = r
    assert lib.gh_gm17_verify(h, p, pb, p, pb, p, pb, rbad.ctypes.data_as(V), 1, 1, pb) == GH_E_BAD_ARG
    assert "public input" in lib.gh_last_error().decode()
    buf = (ctypes.c_float * 9)()
    tot = ctypes.c_float()
    assert lib.gh_gm17_last_timing(buf, 9, ctypes.byref(tot)) == 9
    assert lib.gh_gm17_last_timing(buf, 12, ctypes.byref(tot)) == 9
    assert lib.gh_gm17_last_timing(None, 3, None) == GH_E_BAD_ARG
    assert lib.gh_pairing_last_timing(buf, 9, ctypes.byref(tot)) == 6                           # the pairing unit keeps its own six
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:                                                  # the library's own verdict
        assert lib.gh_gm17_verify(h, p, pb, p, pb, p, pb, p, 1, 1, pb) == GH_E_NO_DEVICE
        with pytest.raises(gm17_verify.GingerHipError):
            pvk.verify((x[:1, :24], b[:1]), (x[:1], b[:1]), (x[:1, :24], b[:1]), np.zeros((1, 1, 12), dtype=np.uint64))
    pvk.close()
    assert pvk.handle is None


def test_verify_proofs_refuses_bad_records(gl, pr):
    from ginger_lib_amd import gm17_verify
    engine, g2_rec = pr.name, 96 * pr.k + 1
    pvk = gm17_verify.PreparedVerifyingKey(*_vk_arrays(pr), engine=engine)
    try:
        rec = bytes(193 + g2_rec + 193)
        with pytest.raises(ValueError):                                                         # a wrong record length
            gm17_verify.verify_proofs(pvk, [rec[:-1]], [[1]])
        with pytest.raises(ValueError):
            gm17_verify.verify_proofs(pvk, [rec + b"\x00"], [[1]])
        with pytest.raises(ValueError):                                                         # a wrong number of inputs
            gm17_verify.verify_proofs(pvk, [rec], [[1, 2]])
        with pytest.raises(ValueError):
            gm17_verify.verify_proofs(pvk, [rec], [[]])
        with pytest.raises(ValueError):                                                         # one list of inputs per proof
            gm17_verify.verify_proofs(pvk, [rec], [[1], [2]])
        with pytest.raises(ValueError):                                                         # an input not below the modulus
            gm17_verify.verify_proofs(pvk, [rec], [[pr.r]])
        with pytest.raises(ValueError):
            gm17_verify.verify_proofs(pvk, [rec], [[-1]])
        with pytest.raises(ValueError):                                                         # a coordinate not below the modulus
            gm17_verify.verify_proofs(pvk, [pr.p.to_bytes(96, "little") + rec[96:]], [[1]])
        assert list(gm17_verify.verify_proofs(pvk, [], [])) == []
    finally:
        pvk.close()


def test_package_gm17_verify_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "gm17_verify.py")).read()
    for needle in ("tests/", "import pyref", "pairing_ref", "gm17_verify_ref", "oracle"):
        assert needle not in txt, needle
