"""Point validation without a GPU: the GH_HD code of ginger-lib_amd/csrc/sqrt29.h compiled by g++ (tests/host_shim/points_shim.cpp)
against the Python restatement of tests/points_ref.py -- the square roots of Fq, Fq2 and Fq3 on their edge inputs, compress
and decompress over the reference's known points -- the generated constants re-derived from p and r, the stand-alone
sanitised check, and the argument checks / exports of include/ginger_hip_points.h and of its Rust extern block.
Every comparison is exact."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import points_ref as pr
import pyref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ginger-lib_amd", "csrc")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "compression_kats.json")))
GH_E_BAD_ARG, GH_E_NO_DEVICE = -1, -3
V = ctypes.c_void_p
CURVE_ID = {"mnt4753_g1": 0, "mnt4753_g2": 1, "mnt6753_g1": 2, "mnt6753_g2": 3}
# field id of the shim -> the field
FIELDS = {0: pyref.Ext(pyref.P4, 1, 0), 1: pyref.Ext(pyref.P6, 1, 0), 2: pyref.CURVES["mnt4753_g2"].E, 3: pyref.CURVES["mnt6753_g2"].E}


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("points")
    lib.pts_sqrt.argtypes = [ctypes.c_int, V, V]
    lib.pts_decompress.argtypes = [ctypes.c_int, V, ctypes.c_uint8, V, V]
    lib.pts_compress.argtypes = [ctypes.c_int, V, ctypes.c_uint8, V]
    lib.pts_member.argtypes = [ctypes.c_int, V, ctypes.c_uint8]
    return lib


def words(coeffs):
    return np.array([w for c in coeffs for w in pyref.int_to_limbs(c)], dtype=np.uint64)


def ints(arr, k):
    return tuple(pyref.limbs_to_int(arr[12 * i:12 * i + 12]) for i in range(k))


def point_row(C, P):
    return np.array(pyref.ext_to_abi(C.F, P[0]) + pyref.ext_to_abi(C.F, P[1]), dtype=np.uint64)


def point_of(C, row):
    return pyref.ext_from_abi(C.F, list(row[:12 * C.deg]), C.deg), pyref.ext_from_abi(C.F, list(row[12 * C.deg:]), C.deg)


def shim_sqrt(shim, field, a):
    w = words(a)
    out = np.zeros_like(w)
    ok = shim.pts_sqrt(field, w.ctypes.data, out.ctypes.data)
    return bool(ok), ints(out, len(a))


def shim_decompress(shim, C, x, flags):
    w = words(x)
    xy = np.zeros(24 * C.deg, dtype=np.uint64)
    inf = np.zeros(1, dtype=np.uint8)
    st = shim.pts_decompress(CURVE_ID[C.name], w.ctypes.data, flags, xy.ctypes.data, inf.ctypes.data)
    return st, point_of(C, xy), int(inf[0])


def kat_point(name, which):
    d = KATS[name][which]
    return tuple(int(v, 16) for v in d["x"]), tuple(int(v, 16) for v in d["y"])


# ---- 1. the square roots
def sqrt_cases(field):
    """(label, element, whether the reference finds a root)"""
    E = FIELDS[field]
    s, t, z = pr._ts_params(E)
    rng = pyref.Rng(100 + field)
    rnd = tuple(rng.field_elem(E.p) for _ in range(E.k))
    sq = E.mul(rnd, rnd)
    cases = [("zero", E.zero(), True), ("one", E.one(), True), ("non-residue", z, False), ("p - 1", ((E.p - 1,) + (0,) * (E.k - 1)), None),
             ("a square", sq, True), ("a square times a non-residue", E.mul(sq, z), False)]
    no_round = E.pow(rnd, 1 << s)                      # its t-th power is one: Tonelli-Shanks takes no correction round
    assert pr.ts_rounds(E, no_round) == 0
    cases.append(("no round", no_round, True))
    if field != 2:                                     # Fq2 goes by the complex method, and see below
        sylow2 = E.mul(z, z)                           # the square of a generator of the 2-Sylow subgroup: every round
        assert pr.ts_rounds(E, sylow2) == s - 1
        cases.append(("all rounds", sylow2, True))
    if field == 2:
        F1 = FIELDS[0]
        nr = pr._ts_params(F1)[2][0]
        assert pr.is_square(E, (nr, 0)) and not pr.is_square(F1, (nr,))       # a root exists in Fq2 ...
        cases += [("c1 = 0, c0 a residue", (sq[0] * sq[0] % E.p, 0), True), ("c1 = 0, c0 a non-residue", (nr, 0), False)]   # ... the reference: None
        # the same quirk met in the wild: z^2 has order 2^15, so it lies in Fq and generates Fq's 2-Sylow subgroup
        assert E.mul(z, z)[1] == 0
        cases.append(("the square of a generator of the 2-Sylow subgroup", E.mul(z, z), False))
    return E, cases


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_sqrt_matches_the_restatement(shim, field):
    E, cases = sqrt_cases(field)
    for label, a, expect in cases:
        want = pr.fp2_sqrt(E, a) if field == 2 else pr.sqrt_ts(E, a)
        if expect is not None:
            assert (want is not None) == expect, label
        ok, root = shim_sqrt(shim, field, a)
        assert ok == (want is not None), label
        if ok:
            assert E.mul(root, root) == a and root in (want, E.neg(want)), label


# ---- 2. the generated constants, from p and r alone
def _macro(hdr, name):
    return re.search(r"#define %s (.*)" % name, hdr).group(1).strip()


def _arr(hdr, name):
    return [int(t.strip().rstrip("u"), 0) for t in _macro(hdr, name).strip("{}").split(",")]


def test_constants_rederived_from_p_and_r():
    hdr = open(os.path.join(CSRC, "sqrt_constants_gen.h")).read()
    from29 = lambda ws, p: sum(w << (29 * k) for k, w in enumerate(ws)) * pow(2, -754, p) % p
    for name, field, k in (("GH_P4", pyref.P4, 1), ("GH_P6", pyref.P6, 1), ("GH_P6Q3", pyref.P6, 3)):
        p = field.p
        s, t = 0, p ** k - 1
        while t % 2 == 0:
            s, t = s + 1, t // 2
        assert int(_macro(hdr, name + "_SQRT_S")) == s == {"GH_P4": 15, "GH_P6": 30, "GH_P6Q3": 30}[name]
        e = sum(w << (32 * i) for i, w in enumerate(_arr(hdr, name + "_SQRT_E32")))
        assert e == (t - 1) // 2 and int(_macro(hdr, name + "_SQRT_EBITS")) == e.bit_length()
        E = pyref.Ext(field, k, 11 if k == 3 else 0)
        z = (from29(_arr(hdr, name + "_SQRT_Z_I29"), p),) if k == 1 else tuple(from29(_arr(hdr, "%s_SQRT_Z%d_I29" % (name, i)), p) for i in range(3))
        # a non-residue to the power t: of order exactly 2^s
        assert E.pow(z, 1 << (s - 1)) == E.neg(E.one())
        if k == 1:
            assert 2 * from29(_arr(hdr, name + "_HALF_I29"), p) % p == 1
    for name, r in (("GH_MNT4_R", pyref.CURVES["mnt4753_g2"].order), ("GH_MNT6_R", pyref.CURVES["mnt6753_g2"].order)):
        d = _arr(hdr, name + "_NAF")
        assert len(d) == int(_macro(hdr, name + "_DIGITS")) and d[0] == 1 and set(d) <= {-1, 0, 1}
        assert sum(1 for v in d if v) == int(_macro(hdr, name + "_NONZERO"))
        assert all(not (a and b) for a, b in zip(d, d[1:]))                    # non-adjacent
        v = 0
        for digit in d:
            v = 2 * v + digit
        assert v == r
    assert pyref.CURVES["mnt4753_g1"].order == pyref.CURVES["mnt4753_g2"].order == pyref.P6.p
    assert pyref.CURVES["mnt6753_g1"].order == pyref.CURVES["mnt6753_g2"].order == pyref.P4.p


def test_generator_reproduces_the_committed_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_sqrt_constants as g
    assert g.render(g.derive()) == open(os.path.join(CSRC, "sqrt_constants_gen.h")).read()


# ---- 3. compress and decompress over the reference's known points (host path)
@pytest.mark.parametrize("name", sorted(CURVE_ID))
def test_kats_through_the_host_path(shim, name):
    C = pyref.CURVES[name]
    for which, parity in (("even", 0), ("odd", pr.FLAG_PARITY)):
        P = kat_point(name, which)
        assert pr.compress(C, P) == (P[0], parity)
        row = point_row(C, P)
        x = np.zeros(12 * C.deg, dtype=np.uint64)
        assert shim.pts_compress(CURVE_ID[name], row.ctypes.data, 0, x.ctypes.data) == parity
        assert ints(x, C.deg) == P[0]
        assert shim_decompress(shim, C, P[0], parity) == (pr.OK, P, 0)
        assert shim.pts_member(CURVE_ID[name], row.ctypes.data, 0) == 1
    # the other flag gives the opposite point; the restatement agrees (the subgroup test of G2 is taken from the construction)
    P = kat_point(name, "even")
    assert shim_decompress(shim, C, P[0], pr.FLAG_PARITY) == (pr.OK, C.neg(P), 0)
    assert pr.decompress(C, P[0], pr.FLAG_PARITY, check_subgroup=False) == (pr.OK, C.neg(P))


def test_statuses_through_the_host_path(shim):
    for name in sorted(CURVE_ID):
        C = pyref.CURVES[name]
        zero = C.E.zero()
        assert shim_decompress(shim, C, zero, pr.FLAG_INFINITY) == (pr.OK, (zero, C.E.one()), 1)
        for x, flags in ((zero, 3), (C.E.one(), pr.FLAG_INFINITY), (zero, 4), (zero, 0x81)):
            assert shim_decompress(shim, C, x, flags)[0] == pr.INVALID_FLAGS == pr.decompress(C, x, flags)[0]
        for bad in (C.E.p, C.E.p + 1, (1 << 768) - 1):
            x = (0,) * (C.deg - 1) + (bad,)
            assert shim_decompress(shim, C, x, 3) == (pr.INVALID_FIELD_ELEMENT, (zero, zero), 0)      # before the flags, as the reference
        # x = 0: b is a square on both G1 (either parity decompresses, curves/mnt4753/tests.rs:102-110), the twisted b is not
        want = pr.OK if C.deg == 1 else pr.NOT_ON_CURVE
        assert pr.is_square(C.E, C.b) == (C.deg == 1)
        for flags in (0, pr.FLAG_PARITY):
            st, P, inf = shim_decompress(shim, C, zero, flags)
            assert st == want and inf == 0
            if st == pr.OK:
                assert C.on_curve(P) and pr.is_odd(P[1]) == bool(flags)


def test_g2_point_outside_the_subgroup(shim):
    """an on-curve point of the twist found by the Python root is outside the subgroup of order r: NotPrimeOrder, not a member"""
    for name in ("mnt4753_g2", "mnt6753_g2"):
        C = pyref.CURVES[name]
        x = (5,) + (1,) + (0,) * (C.deg - 2)
        while pr.field_sqrt(C, pr.rhs(C, x)) is None:
            x = (x[0] + 1,) + x[1:]
        st, T = pr.decompress(C, x, 0, check_subgroup=False)
        assert st == pr.OK and C.on_curve(T) and not pr.membership(C, T)
        assert shim_decompress(shim, C, x, 0)[0] == pr.NOT_PRIME_ORDER
        assert shim.pts_member(CURVE_ID[name], point_row(C, T).ctypes.data, 0) == 0
        assert shim.pts_member(CURVE_ID[name], point_row(C, T).ctypes.data, 1) == 1          # flagged as infinity: a member


def test_bit_vectors_round_trip():
    from __graft_entry__ import _load_pkg
    mod = sys.modules.get("ginger_lib_amd") or _load_pkg()
    from ginger_lib_amd import points
    for name in sorted(CURVE_ID):
        C = pyref.CURVES[name]
        P = kat_point(name, "odd")
        bits = pr.to_bits(*pr.compress(C, P))
        assert len(bits) == C.deg * 753 + 2 and pr.from_bits(bits, C.deg) == (P[0], pr.FLAG_PARITY)
        x, flags = points.bits_to_limbs(C.deg, [bits])
        assert ints(x[0], C.deg) == P[0] and list(flags) == [pr.FLAG_PARITY]
        assert points.limbs_to_bits(x, flags)[0].tolist() == bits
    # read_bits tolerates leading zeros over a prime field; a coordinate that is too long is above the modulus
    x, flags = points.bits_to_limbs(1, [[0] * 40 + pr.to_bits((77,), 1), [1] + [0] * 800 + [0, 0]])
    assert ints(x[0], 1) == (77,) and ints(x[1], 1) == ((1 << 768) - 1,) and list(flags) == [1, 0]
    with pytest.raises(ValueError):
        points.bits_to_limbs(2, [[0] * 100])
    assert mod is not None


# ---- 4. the stand-alone check under the host sanitizers: a program of its own, nothing sanitised is loaded into python
def test_sanitized_standalone_check(tmp_path):
    out = shim_build.sanitized_check("points_check.cpp", str(tmp_path / "points_check"))
    assert out.returncode == 0 and (out.stdout + out.stderr).strip().endswith("ok"), (out.stdout + out.stderr)[-2000:]


# ---- 5. the C ABI without a device
def test_points_symbols_exported_and_kept_apart(gl):
    from ginger_lib_amd import ecvrf, gm17_verify, pairing, points, poseidon, schnorr
    lib = gl.load_library()
    for s in points.POINTS_SYMBOLS:
        assert hasattr(lib, s), s
    others = (gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS + schnorr.SCHNORR_SYMBOLS + ecvrf.ECVRF_SYMBOLS +
              pairing.PAIRING_SYMBOLS + gm17_verify.GM17_SYMBOLS)
    assert not set(points.POINTS_SYMBOLS) & set(others)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_points.h")).read()
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(points.POINTS_SYMBOLS) and len(declared) == 6


def test_entry_points_without_gpu(gl):
    """n == 0 is a no-op, bad arguments are GH_E_BAD_ARG before any device work, and without a device the compute entry points
    return GH_E_NO_DEVICE"""
    from ginger_lib_amd import pairing, points
    import pairing_ref
    lib = points._lib()
    x = np.zeros((2, 72), dtype=np.uint64)
    b = np.zeros(8, dtype=np.uint8)
    p, pb = x.ctypes.data_as(V), b.ctypes.data_as(V)
    for curve in range(4):
        assert lib.gh_group_membership(curve, None, None, 0, None) == 0
        assert lib.gh_points_decompress(curve, None, None, 0, None, None, None) == 0
        assert lib.gh_points_compress(curve, None, None, 0, None, None) == 0
        for hole in range(3):
            args = [p, pb, pb]
            args[hole] = None
            assert lib.gh_group_membership(curve, args[0], args[1], 1, args[2]) == GH_E_BAD_ARG
        for hole in range(5):
            args = [p, pb, p, pb, pb]
            args[hole] = None
            assert lib.gh_points_decompress(curve, args[0], args[1], 1, *args[2:]) == GH_E_BAD_ARG
        for hole in range(4):
            args = [p, pb, p, pb]
            args[hole] = None
            assert lib.gh_points_compress(curve, args[0], args[1], 1, *args[2:]) == GH_E_BAD_ARG
        bad = np.zeros((1, 72), dtype=np.uint64)
        bad[0, :12] = pyref.int_to_limbs(pyref.P4.p if curve < 2 else pyref.P6.p)
        pbad = bad.ctypes.data_as(V)
        assert lib.gh_group_membership(curve, pbad, pb, 1, pb) == GH_E_BAD_ARG and "modulus" in lib.gh_last_error().decode()
        assert lib.gh_points_compress(curve, pbad, pb, 1, p, pb) == GH_E_BAD_ARG
    for curve in (-1, 4, 99):
        assert lib.gh_group_membership(curve, p, pb, 1, pb) == GH_E_BAD_ARG and "curve" in lib.gh_last_error().decode()
        assert lib.gh_points_decompress(curve, p, pb, 1, p, pb, pb) == GH_E_BAD_ARG
        assert lib.gh_points_compress(curve, p, pb, 1, p, pb) == GH_E_BAD_ARG
    buf = (ctypes.c_float * 3)()
    tot = ctypes.c_float()
    assert lib.gh_points_last_timing(buf, 3, ctypes.byref(tot)) == 3
    assert lib.gh_points_last_timing(None, 3, None) == GH_E_BAD_ARG
    # the two verifiers: the checks of gh_groth16_verify, and compressed coordinates are data, not arguments
    m4 = pairing_ref.engine("mnt4753")
    C1, C2 = m4.C1, m4.C2
    gt = m4.gt_row(m4.ONE).reshape(1, 48)
    gamma, delta = m4.g2_row(C2.mul(3, C2.G)).reshape(1, 48), m4.g2_row(C2.mul(5, C2.G)).reshape(1, 48)
    abc = np.stack([m4.g1_row(C1.mul(k, C1.G)) for k in (2, 7)])
    pvk = pairing.PreparedVerifyingKey(gt, gamma, delta, abc)
    h = pvk.handle
    for fn in (lib.gh_groth16_verify_checked, lib.gh_groth16_verify_compressed):
        assert fn(h, p, pb, p, pb, p, pb, p, 0, 1, pb, None) == 0
        assert fn(h, p, pb, p, pb, p, pb, p, 1, 2, pb, pb) == GH_E_BAD_ARG and "MalformedVerifyingKey" in lib.gh_last_error().decode()
        assert fn(None, p, pb, p, pb, p, pb, p, 1, 1, pb, pb) < 0
        for hole in range(8):
            args = [p, pb, p, pb, p, pb, p, pb]
            args[hole] = None
            assert fn(h, *args[:7], 1, 1, args[7], None) == GH_E_BAD_ARG, hole
        rbad = np.zeros((1, 12), dtype=np.uint64)
        rbad[0] = pyref.int_to_limbs(m4.r)
        assert fn(h, p, pb, p, pb, p, pb, rbad.ctypes.data_as(V), 1, 1, pb, pb) == GH_E_BAD_ARG
    big = np.zeros((1, 48), dtype=np.uint64)
    big[0, :12] = pyref.int_to_limbs(m4.p)
    pbig = big.ctypes.data_as(V)
    assert lib.gh_groth16_verify_checked(h, pbig, pb, p, pb, p, pb, p, 1, 1, pb, pb) == GH_E_BAD_ARG
    gm17_h = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))                # not a Groth16 key
    assert lib.gh_groth16_verify_checked(gm17_h, p, pb, p, pb, p, pb, p, 1, 1, pb, pb) < 0
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:                                                  # the library's own verdict
        for curve in range(4):
            assert lib.gh_group_membership(curve, p, pb, 1, pb) == GH_E_NO_DEVICE
            assert lib.gh_points_decompress(curve, p, pb, 1, p, pb, pb) == GH_E_NO_DEVICE
            assert lib.gh_points_compress(curve, p, pb, 1, p, pb) == GH_E_NO_DEVICE
        assert lib.gh_groth16_verify_checked(h, p, pb, p, pb, p, pb, p, 1, 1, pb, pb) == GH_E_NO_DEVICE
        assert lib.gh_groth16_verify_compressed(h, pbig, pb, p, pb, p, pb, p, 1, 1, pb, pb) == GH_E_NO_DEVICE     # x = p is a row's status
        with pytest.raises(points.GingerHipError):
            points.group_membership_test("mnt4753_g2", (x[:1, :48], b[:1]))
    pvk.close()


def test_package_points_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "points.py")).read()
    for needle in ("tests/", "import pyref", "points_ref", "pairing_ref", "oracle"):
        assert needle not in txt, needle


# ---- the Rust side (delivered as files: no Rust toolchain checks them here)
def test_rust_points_extern_block_is_generated_from_the_header():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    src = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")
    rs = open(os.path.join(src, "points.rs")).read()
    block = rs[rs.index("// ---- GENERATED by"):rs.index("// ---- GENERATED: end")]
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (gh_\w+)\((.*?)\)", block)}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ginger_hip_points.h")).read(), flags=re.S)
    c = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(gh_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)}
    assert sorted(rust) == sorted(c) and len(c) == 6
    for name, params in c.items():
        assert params.count(",") == rust[name].count(","), name
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "pub mod points;" in lib[lib.index("// ---- GENERATED: end"):]
    assert "gh_points" not in lib and "gh_group_membership" not in lib       # the crate's main extern block stays the two headers
