"""The polynomial unit without a GPU: the referee's closed forms against the reference's loops (tests/poly_ref.py), the level
arithmetic of ginger-lib_amd/csrc/poly_plan.h and the lane bodies of poly_kernels.h compiled by g++
(tests/host_shim/poly_shim.cpp) against the referee on the shapes the GPU tests run, the argument checks of
include/ginger_hip_poly.h, and the stand-alone sanitised check.  Every comparison is exact and covers every row."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import poly_ref as ref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_BAD_ARG, GH_E_UNSUPPORTED = -1, -2
V, U64, U32, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
FIELD_ID = {"mnt4753_fr": 0, "mnt6753_fr": 1}
CASES = ref.cases()
TUNED = CASES["tuning"]


@pytest.fixture(scope="module")
def poly(gl):
    return importlib.import_module("ginger_lib_amd.poly")


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("poly")
    lib.poly_shim_evaluate.argtypes = [I, V, U64, V, U64, U32, U32, V]
    lib.poly_shim_divide_linear.argtypes = [I, V, U64, V, U32, U32, V, V]
    lib.poly_shim_divide_vanishing.argtypes = [I, V, U64, U32, U32, V, V]
    lib.poly_shim_axpy.argtypes = [I, I, V, U64, V, U64, V, V]
    lib.poly_shim_mul_vanishing.argtypes = [I, V, U64, U32, V]
    lib.poly_shim_trimmed_len.argtypes = lib.poly_shim_count_zero.argtypes = [V, U64]
    lib.poly_shim_trimmed_len.restype = lib.poly_shim_count_zero.restype = U64
    lib.poly_shim_elements.argtypes = [I, V, U32, V]
    lib.poly_shim_sparse.argtypes = [I, V, V, V, U64, U32, V]
    lib.poly_shim_fold_cover.argtypes = lib.poly_shim_fold_levels.argtypes = [U64, U32, U32]
    lib.poly_shim_scan_cover.argtypes = [U64, U64, U32, U32]
    return lib


def P(a):
    return a.ctypes.data_as(V) if a is not None and a.size else None


def mont(vals, p):
    R = (1 << 768) % p
    raw = b"".join((v % p * R % p).to_bytes(96, "little") for v in vals)
    return np.frombuffer(raw + b"\0" * (0 if vals else 96), dtype=np.uint64).reshape(-1, 12).copy()


def ints(rows, n, p):
    rinv = pow(1 << 768, -1, p)
    raw = np.ascontiguousarray(rows, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[96 * i:96 * i + 96], "little") * rinv % p for i in range(n)]


def out_rows(n):
    return np.full((max(n, 1), 12), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


# ---- 1. the referee
@pytest.mark.parametrize("field", ref.FIELDS)
def test_closed_forms_match_the_reference_loops(field):
    ref.check_closed_forms(field)


# ---- 2. the plans
def test_every_plan_terminates_bounds_its_lanes_and_covers_every_index_once(shim):
    for n in CASES["plan_n"]:
        for run_len, direct_max, seg_max in (TUNED, (0, 0, 0)):
            assert shim.poly_shim_fold_cover(n, run_len, direct_max) == 0, (n, run_len)
            assert shim.poly_shim_scan_cover(n, 1, run_len or 32, direct_max or 32) == 0, (n, run_len)
            for N in (1, 2, 64, 1 << 15, 1 << 23):
                if n >= 1 << 20 and N == 2:
                    continue
                assert shim.poly_shim_scan_cover(n, N, seg_max or 64, seg_max or 64) == 0, (n, N, seg_max)
    assert shim.poly_shim_fold_levels(1000, 4, 4) == 5 and shim.poly_shim_fold_levels(1 << 24, 0, 0) == 5
    assert shim.poly_shim_fold_levels(0, 0, 0) == 0


# ---- 3. the lane bodies on the host
@pytest.mark.parametrize("field", ref.FIELDS)
def test_evaluate_lanes(shim, field):
    p, f = ref.MODULUS[field], FIELD_ID[field]
    pts = ref.points(field)
    for tuned, sizes in ((TUNED, CASES["evaluate_tuned"]), ((0, 0, 0), [n for n in CASES["evaluate_default"] if n <= 1025])):
        for n in sizes:
            for kind in ("random", "zero", "zero_top"):
                c = ref.coeffs(field, n, "ev", kind)
                want = [ref.evaluate(c, z, p) for z in pts]
                for k in CASES["evaluate_k"] + [len(pts)]:
                    out = out_rows(k)
                    shim.poly_shim_evaluate(f, P(mont(c, p)), n, P(mont(pts[-k:], p)), k, tuned[0], tuned[1], P(out))
                    assert ints(out, k, p) == want[-k:], (n, kind, k)


@pytest.mark.parametrize("field", ref.FIELDS)
def test_divide_by_linear_lanes(shim, field):
    p, f = ref.MODULUS[field], FIELD_ID[field]
    for tuned, sizes in ((TUNED, CASES["linear_tuned"]), ((0, 0, 0), [1025])):
        for n in sizes:
            c = ref.coeffs(field, n, "lin")
            zs = ref.points(field)[:3] + ref.points(field)[4:5]
            if n >= 2:                                          # a root planted by construction: p = q0 (x - root)
                root = ref.points(field)[5]
                q0 = ref.coeffs(field, n - 1, "root")
                planted = [((q0[i - 1] if i else 0) - root * (q0[i] if i < n - 1 else 0)) % p for i in range(n)]
            for z, cc in [(z, c) for z in zs] + ([(root, planted)] if n >= 2 else []):
                q, rem = out_rows(max(n, 1) - 1), out_rows(1)
                shim.poly_shim_divide_linear(f, P(mont(cc, p)), n, P(mont([z], p)), tuned[0], tuned[1], P(q), P(rem))
                wq, wr = ref.divide_by_linear_closed(cc, z, p)
                assert ints(q, len(wq), p) == wq and ints(rem, 1, p) == [wr], (n, z)
                if cc is not c:
                    assert wr == 0 and wq == q0


@pytest.mark.parametrize("field", ref.FIELDS)
def test_vanishing_lanes(shim, field):
    p, f = ref.MODULUS[field], FIELD_ID[field]
    shapes = [(lg, n, 4) for lg in CASES["vanishing_log_n"] for n in CASES["vanishing_n"](1 << lg)]
    shapes += [CASES["vanishing_two_pass"] + (4,), (0, 300, 0), (2, 1025, 0)]
    for log_n, n, seg in shapes:
        N = 1 << log_n
        for kind in ("random", "zero_top"):
            c = ref.coeffs(field, n, "van", kind)
            out = out_rows(n + N)
            shim.poly_shim_mul_vanishing(f, P(mont(c, p)), n, log_n, P(out))
            prod = ints(out, n + N, p)
            assert ref.trim(prod) == ref.mul_by_vanishing(c, N, p), (N, n)
            q, r = out_rows(max(n, N) - N), out_rows(N)
            shim.poly_shim_divide_vanishing(f, P(mont(c, p)), n, log_n, seg, P(q), P(r))
            wq, wr = ref.divide_by_vanishing_closed(c, N, p)
            assert (ints(q, len(wq), p), ints(r, N, p)) == (wq, wr), (N, n, seg)
            rr = ref.coeffs(field, N, "rem")                    # divide(mul_by_vanishing(p) + r) = (p, r)
            full = [(prod[i] + (rr[i] if i < N else 0)) % p for i in range(n + N)]
            q2, r2 = out_rows(n), out_rows(N)
            shim.poly_shim_divide_vanishing(f, P(mont(full, p)), n + N, log_n, seg, P(q2), P(r2))
            assert (ints(q2, n, p), ints(r2, N, p)) == (c, rr), (N, n)


@pytest.mark.parametrize("field", ref.FIELDS)
def test_elementwise_and_reduction_lanes(shim, field):
    p, f = ref.MODULUS[field], FIELD_ID[field]
    scale = ref.points(field)[4]
    for na in CASES["axpy"]:
        for nb in CASES["axpy"]:
            a, b = ref.coeffs(field, na, "a"), ref.coeffs(field, nb, "b")
            rows = max(na, nb)
            pad = lambda v: v + [0] * (rows - len(v))
            want = {0: [(x + y) % p for x, y in zip(pad(a), pad(b))], 1: [(x - y) % p for x, y in zip(pad(a), pad(b))],
                    2: [(x + scale * y) % p for x, y in zip(pad(a), pad(b))]}
            for op, w in want.items():
                out = out_rows(rows)
                shim.poly_shim_axpy(f, op, P(mont(a, p)), na, P(mont(b, p)), nb, P(mont([scale], p)), P(out))
                assert ints(out, rows, p) == w, (op, na, nb)
        out = out_rows(na)
        shim.poly_shim_axpy(f, 3, P(mont(a, p)), na, None, 0, None, P(out))
        assert ints(out, na, p) == [-x % p for x in a]
    for n in CASES["trimmed_len"]:
        for last in sorted({0, n - 1, 255, 256, 2047, 2048, -1}):
            if last >= n:
                continue
            c = [0] * n
            if last >= 0:
                c[last] = p - 1
                c[0] = c[0] or 5
            rows = mont(c, p)
            assert shim.poly_shim_trimmed_len(P(rows), n) == len(ref.trim(c)), (n, last)
            assert shim.poly_shim_count_zero(P(rows), n) == c.count(0), (n, last)


@pytest.mark.parametrize("field", ref.FIELDS)
def test_domain_lanes(shim, field):
    p, f = ref.MODULUS[field], FIELD_ID[field]
    for log_n in CASES["domain_log_n"]:
        N = 1 << log_n
        g = pow(17, (p - 1) >> log_n, p)
        out = out_rows(N)
        shim.poly_shim_elements(f, P(mont([g], p)), log_n, P(out))
        assert ints(out, N, p) == [pow(g, i, p) for i in range(N)]
        for terms in ([(0, p - 1), (N, 1)], [(0, 2), (1, 2)], [(3, 7), (N + 5, p - 2), (3 * N, 9)], []):
            exps = np.array([e for e, _ in terms], dtype=np.uint64)
            shim.poly_shim_sparse(f, P(mont([g], p)), P(exps), P(mont([c for _, c in terms], p)), len(terms), log_n, P(out))
            assert ints(out, N, p) == [ref.sparse_evaluate(terms, pow(g, i, p), p) for i in range(N)], (log_n, terms)


# ---- 4. the C ABI without a device: the order and the messages of the argument checks
def test_header_prototypes_match_the_binding(poly):
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_poly.h")).read()
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(poly.POLY_SYMBOLS)
    for name, types in poly._ARGTYPES.items():
        params = re.search(r"^int %s\(([^;]*?)\);" % name, hdr, re.M | re.S).group(1)
        assert len(types) == params.count(",") + 1, name
    lib = poly._lib()
    for s in poly.POLY_SYMBOLS:
        assert hasattr(lib, s), s


def test_argument_checks_come_in_order_with_their_messages(poly):
    lib = poly._lib()
    buf = np.zeros((8, 12), dtype=np.uint64)
    b = P(buf)
    n_out = ctypes.c_size_t()
    nref = ctypes.byref(n_out)
    err = lambda: lib.gh_last_error().decode()
    # an unknown field is found before a null pointer, a null pointer before k = 0, k = 0 and the pointers before the domain
    calls_unknown_field = [
        lambda fld: lib.gh_poly_evaluate_dev(fld, None, 4, None, 0, None), lambda fld: lib.gh_poly_evaluate(fld, None, 4, None, 0, None),
        lambda fld: lib.gh_poly_resize_dev(fld, None, 4, None, 4), lambda fld: lib.gh_poly_trimmed_len_dev(fld, None, 4, None),
        lambda fld: lib.gh_poly_add_dev(fld, None, 4, None, 4, None), lambda fld: lib.gh_poly_sub_dev(fld, None, 4, None, 4, None),
        lambda fld: lib.gh_poly_add_scaled_dev(fld, None, 4, None, 4, None, None), lambda fld: lib.gh_poly_neg_dev(fld, None, 4, None),
        lambda fld: lib.gh_poly_mul_by_vanishing_dev(fld, None, 4, 40, None), lambda fld: lib.gh_poly_divide_by_vanishing_dev(fld, None, 4, 40, None, None),
        lambda fld: lib.gh_poly_divide_by_vanishing(fld, None, 4, 40, None, None), lambda fld: lib.gh_poly_divide_by_linear_dev(fld, None, 4, None, None, None),
        lambda fld: lib.gh_poly_divide_by_linear(fld, None, 4, None, None, None), lambda fld: lib.gh_poly_mul_dev(fld, None, 4, None, 4, None, 8, None),
        lambda fld: lib.gh_poly_mul(fld, None, 4, None, 4, None, 8, None), lambda fld: lib.gh_evals_div_dev(fld, None, None, 4, None),
        lambda fld: lib.gh_domain_elements_dev(fld, 40, None), lambda fld: lib.gh_poly_sparse_evaluate_over_domain_dev(fld, None, None, 2, 40, None)]
    for call in calls_unknown_field:
        assert call(7) == GH_E_BAD_ARG and err() == "unknown field id"
        assert call(0) == GH_E_BAD_ARG and err() == "null argument"
    assert lib.gh_poly_evaluate_dev(0, b, 4, None, 0, None) == GH_E_BAD_ARG and err() == "k: at least one point"
    assert lib.gh_poly_evaluate(0, b, 4, b, 0, b) == GH_E_BAD_ARG and err() == "k: at least one point"
    assert lib.gh_poly_evaluate_dev(0, None, 4, b, 0, b) == GH_E_BAD_ARG and err() == "null argument"
    for field, adicity in ((0, 30), (1, 15)):
        for call in (lambda lg: lib.gh_poly_mul_by_vanishing_dev(field, b, 4, lg, b), lambda lg: lib.gh_poly_divide_by_vanishing_dev(field, b, 4, lg, b, b),
                     lambda lg: lib.gh_poly_divide_by_vanishing(field, b, 4, lg, b, b), lambda lg: lib.gh_domain_elements_dev(field, lg, b),
                     lambda lg: lib.gh_poly_sparse_evaluate_over_domain_dev(field, b, b, 1, lg, b)):
            assert call(adicity) == GH_E_UNSUPPORTED and err() == "domain exceeds the field's 2-adicity"
            assert call(64) == GH_E_UNSUPPORTED
    assert lib.gh_poly_set_tuning(1, 0, 0) == GH_E_BAD_ARG and lib.gh_poly_set_tuning(0, 0, 1) == GH_E_BAD_ARG
    assert lib.gh_poly_set_tuning(4, 4, 4) == 0 and lib.gh_poly_set_tuning(0, 0, 0) == 0
    ms = ctypes.c_float(-1)
    assert lib.gh_poly_last_timing(ctypes.byref(ms)) == 0 and ms.value >= 0 and lib.gh_poly_last_timing(None) == 0
    # nothing to do is no error and needs no device
    assert lib.gh_poly_add_dev(0, None, 0, None, 0, None) in (0, -3) and lib.gh_poly_resize_dev(0, None, 0, None, 0) == 0
    assert n_out.value == 0 and nref is not None


def test_package_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "poly.py")).read()
    for needle in ("tests/", "import pyref", "poly_ref", "oracle"):
        assert needle not in txt, needle


# ---- 5. the stand-alone check under the host sanitizers: a program of its own, nothing sanitised is loaded into python
def test_sanitized_standalone_check(tmp_path):
    out = shim_build.sanitized_check("poly_check.cpp", str(tmp_path / "poly_check"))
    assert out.returncode == 0 and (out.stdout + out.stderr).strip().endswith("ok"), (out.stdout + out.stderr)[-2000:]
