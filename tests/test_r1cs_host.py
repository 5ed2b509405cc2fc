"""The sparse R1CS products without a GPU: the referee (tests/r1cs_ref.py) against the existing host path, the schedule of
ginger-lib_amd/csrc/r1cs_plan.h compiled by g++ (tests/host_shim/r1cs_shim.cpp) -- its shape, its transposition, and its
host executor against the referee on the cases the GPU tests run --, the refusals and handle checks of
include/ginger_hip_r1cs.h, the stand-alone sanitised check and the generated Rust block.  Every comparison is exact."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pyref
import r1cs_ref as ref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_BAD_ARG, GH_E_UNSUPPORTED, GH_E_NO_DEVICE, GH_E_BAD_HANDLE = -1, -2, -3, -6
V = ctypes.c_void_p
U64, U32 = ctypes.c_uint64, ctypes.c_uint32
PAIRINGS = ("mnt4753", "mnt6753")
FIELD_ID = {"mnt4753": 0, "mnt6753": 1}
MODULUS = {"mnt4753": pyref.P6.p, "mnt6753": pyref.P4.p}         # the scalar field of a pairing is the other curve's base field


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("r1cs")
    lib.r1cs_shim_check.argtypes = [U64, U64, V, V, V, U64, ctypes.POINTER(ctypes.c_char_p)]
    lib.r1cs_shim_run.argtypes = [ctypes.c_int, U64, U64, V, V, V, V, U64, U32, ctypes.c_int, V, V]
    lib.r1cs_shim_classify.argtypes = [ctypes.c_int, V, U64, V, V]
    lib.r1cs_shim_transpose.argtypes = [U64, U64, V, V, V, V, V, V]
    lib.r1cs_shim_row_levels.argtypes = [U64, U32]
    lib.r1cs_shim_row_levels.restype = U32
    lib.r1cs_shim_shape.argtypes = [U64, U64, V, V, V, U64, U32, V, V, V, V, U32, ctypes.POINTER(ctypes.c_int)]
    lib.r1cs_shim_shape.restype = U32
    return lib


@pytest.fixture(scope="module")
def r1cs(gl):
    return importlib.import_module("ginger_lib_amd.r1cs")


@pytest.fixture(scope="module")
def groth16(gl):
    return importlib.import_module("ginger_lib_amd.groth16")


def P(a):
    return a.ctypes.data_as(V) if a is not None and a.size else None


def mont(vals, r):
    R = (1 << 768) % r
    return np.array([pyref.int_to_limbs(v * R % r) for v in vals], dtype=np.uint64).reshape(-1, 12)


def ints(rows, r):
    rinv = pow(1 << 768, -1, r)
    return [pyref.limbs_to_int(list(row)) * rinv % r for row in np.asarray(rows, dtype=np.uint64).reshape(-1, 12)]


def shim_matvec(shim, r1cs, pairing, rows, n_cols, x, S, transpose):
    """y = M x (or M^T x) through the level builder and the host executor"""
    r = MODULUS[pairing]
    row_ptr, col, ids, vals = r1cs.flatten(rows, r)
    n_out = n_cols if transpose else len(rows)
    y = np.full((max(n_out, 1), 12), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    xm = mont(x, r)
    assert shim.r1cs_shim_run(FIELD_ID[pairing], len(rows), n_cols, P(row_ptr), P(col), P(ids), P(vals), len(vals), S, int(transpose), P(xm), P(y)) == 0
    return ints(y[:n_out], r)


# ---- 1. the referee against the existing path
@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("n", [13, 253])
def test_referee_evaluate_equals_benchmark_circuit_rows(groth16, pairing, n):
    r = MODULUS[pairing]
    assert importlib.import_module("ginger_lib_amd.limbs").MODULUS[pairing] == r
    num_inputs, assignment, A, B, C = groth16.benchmark_circuit_rows(pairing, n)
    lcs = groth16.benchmark_circuit_lcs(n)
    assert lcs[0] == num_inputs and lcs[0] + lcs[1] == len(assignment)
    a, b, c = ref.evaluate(lcs, assignment, r)
    size = ref.domain_size(n, num_inputs)
    assert len(a) == len(b) == len(c) == size
    assert a[:n] == A and b[:n] == B and c[:n] == C
    assert a[n:n + num_inputs] == [1] + assignment[1:num_inputs]
    assert not any(a[n + num_inputs:]) and not any(b[n:]) and not any(c[n:])


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_referee_instance_map_equals_the_generators_loop(groth16, pairing):
    import groth16_ref as G
    import support as S
    n = 13
    _, info = G.generate_parameters(pairing, n, seed=21)
    F = S.FIELD_OF[pairing + "_fr"]
    u = G.lagrange_coefficients(F, info["log_n"], info["toxic"][4])
    lcs = groth16.benchmark_circuit_lcs(n)
    assert (lcs[2], lcs[3], lcs[4]) == (info["at"], info["bt"], info["ct"])
    a, b, c = ref.instance_map(lcs, u, F.p)
    assert (a, b, c) == tuple(info["qap"][:3])


# ---- 2. the host executor of the schedule against the referee, on the cases of the GPU tests
def executor_cases(groth16, r):
    """(name, lcs, segment lengths)"""
    out = [("hand_built", ref.hand_built_system(r), (4, 2, 32))]
    for nc in (1, 63, 64, 65, 130):
        out.append(("edges_%d" % nc, ref.random_system(nc, 9, r, seed=nc), (4,)))
    out.append(("nnz0", (2, 5, [[] for _ in range(9)], [[] for _ in range(9)], [[] for _ in range(9)]), (4,)))
    out.append(("benchmark_1100", groth16.benchmark_circuit_lcs(1100), (32, 4)))
    out.append(("benchmark_253", groth16.benchmark_circuit_lcs(253), (4,)))
    return out


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_host_executor_equals_referee(shim, r1cs, groth16, pairing):
    r = MODULUS[pairing]
    for name, lcs, segs in executor_cases(groth16, r):
        ni, na, at, bt, ct = lcs
        nv, nc = ni + na, len(at)
        x = ref.hand_built_vector(nv, r, seed=len(name))
        u = ref.hand_built_vector(nc, r, seed=len(name) + 1)
        for rows in (at, bt, ct):
            want = ref.matvec(rows, x, r)
            want_t = ref.matvec(rows, u, r, num_out=nv, transpose=True)
            for S in segs:
                assert shim_matvec(shim, r1cs, pairing, rows, nv, x, S, False) == want, (name, S)
                assert shim_matvec(shim, r1cs, pairing, rows, nv, u, S, True) == want_t, (name, S, "transposed")


def test_matvec_referee_is_the_reference_shaped_referee(groth16):
    """ref.matvec, which the executor is compared with, agrees with ref.evaluate / ref.instance_map on a system with general
    coefficients, so the two reference restatements referee every case"""
    r = MODULUS["mnt4753"]
    lcs = ref.hand_built_system(r)
    ni, na, at, bt, ct = lcs
    z = ref.hand_built_vector(ni + na, r)
    a, b, c = ref.evaluate(lcs, z, r)
    assert [a[:130], b[:130], c[:130]] == [ref.matvec(m, z, r) for m in (at, bt, ct)]
    u = ref.hand_built_vector(256, r, seed=9)
    a, b, c = ref.instance_map(lcs, u, r)
    at_u = ref.matvec(at, u, r, num_out=ni + na, transpose=True)
    assert a == [(v + (u[130 + i] if i < ni else 0)) % r for i, v in enumerate(at_u)]
    assert b == ref.matvec(bt, u, r, num_out=ni + na, transpose=True) and c == ref.matvec(ct, u, r, num_out=ni + na, transpose=True)


# ---- 3. the shape of the schedule
def ceil_log(t, S):
    k, cap = 0, 1
    while cap < t:
        cap *= S
        k += 1
    return k


def shape_of(shim, row_ptr, col, ids, n_cols, S, max_levels=40):
    rows = len(row_ptr) - 1
    nnz = int(row_ptr[-1])
    seen = np.zeros(max(nnz, 1), dtype=np.uint32)
    finals = np.zeros(max(rows, 1), dtype=np.uint32)
    segs = np.zeros(max_levels, dtype=np.uint32)
    parts = np.zeros(max_levels, dtype=np.uint32)
    bad = ctypes.c_int(0)
    levels = shim.r1cs_shim_shape(rows, n_cols, P(row_ptr), P(col), P(ids), 1, S, P(seen), P(finals), P(segs), P(parts), max_levels, ctypes.byref(bad))
    return levels, seen[:nnz], finals[:rows], segs[:levels], parts[:levels], bad.value


@pytest.mark.parametrize("S", [2, 3, 4, 32])
def test_level_count_is_ceil_log(shim, S):
    """ceil(log_S t) levels for t = S, S + 1, S^2, S^2 + 1; a row of one term (and an empty row) takes one level, not
    ceil(log_S 1) = 0: its lane still applies the coefficient and writes the row"""
    for t in (1, S, S + 1, S * S, S * S + 1):
        want = max(1, ceil_log(t, S))
        assert shim.r1cs_shim_row_levels(t, S) == want
        row_ptr = np.array([0, t], dtype=np.uint64)
        col = np.zeros(t, dtype=np.uint32)
        levels, seen, finals, segs, parts, bad = shape_of(shim, row_ptr, col, col, 1, S)
        assert levels == want and not bad and (seen == 1).all() and list(finals) == [1], (S, t)
        assert segs[0] == -(-t // S) and parts[-1] == 0
    assert shim.r1cs_shim_row_levels(0, S) == 1
    assert shim.r1cs_shim_row_levels(1 << 20, 32) == 4


def test_every_term_once_on_level_zero_and_every_row_closed_once(shim, r1cs, groth16):
    r = MODULUS["mnt4753"]
    for lcs in (ref.hand_built_system(r), groth16.benchmark_circuit_lcs(1100)):
        ni, na, at, bt, ct = lcs
        for rows in (at, bt, ct):
            row_ptr, col, ids, _ = r1cs.flatten(rows, r)
            for S in (2, 4, 32):
                levels, seen, finals, segs, parts, bad = shape_of(shim, row_ptr, col, np.zeros_like(ids), ni + na, S)
                longest = max(len(row) for row in rows)
                assert not bad and (seen == 1).all() and (finals == 1).all()
                assert levels == max(1, ceil_log(longest, S))
                assert segs[0] == sum(max(1, -(-len(row) // S)) for row in rows)


def test_transposition_is_stable_in_row_order(shim, r1cs):
    r = MODULUS["mnt6753"]
    ni, na, at, _, _ = ref.hand_built_system(r)
    nv = ni + na
    row_ptr, col, ids, _ = r1cs.flatten(at, r)
    nnz = len(col)
    t_ptr, t_col, t_ids = np.zeros(nv + 1, dtype=np.uint64), np.zeros(nnz, dtype=np.uint32), np.zeros(nnz, dtype=np.uint32)
    shim.r1cs_shim_transpose(len(at), nv, P(row_ptr), P(col), P(ids), P(t_ptr), P(t_col), P(t_ids))
    want = [[] for _ in range(nv)]
    k = 0
    for i, row in enumerate(at):                           # terms of a column in row order, a repeated index twice in its order
        for _ in row:
            want[col[k]].append((i, ids[k]))
            k += 1
    got = [[(int(t_col[j]), int(t_ids[j])) for j in range(int(t_ptr[v]), int(t_ptr[v + 1]))] for v in range(nv)]
    assert got == want and int(t_ptr[-1]) == nnz
    assert got[69] == [] and len(got[2]) >= 100            # the unused variable, the long column


def test_dictionary_classes(shim):
    for pairing in PAIRINGS:
        r = MODULUS[pairing]
        vals = [0, 1, r - 1, 2, r - 2, 15, r - 15, 16, r - 16, r // 2, 3]
        codes = np.zeros(len(vals), dtype=np.uint32)
        counts = np.zeros(6, dtype=np.uint32)
        shim.r1cs_shim_classify(FIELD_ID[pairing], P(mont(vals, r)), len(vals), P(codes), P(counts))
        cls = [int(c) & 7 for c in codes]
        assert cls == [0, 1, 2, 3, 4, 3, 4, 5, 5, 5, 3]
        assert [int(c) >> 3 for c in codes][:7] == [0, 1, 1, 2, 2, 15, 15] and int(codes[7]) >> 3 == 7
        assert list(counts) == [1, 1, 1, 3, 2, 3]


# ---- 4. the C ABI without a device
def upload_args(r1cs, lcs, r):
    ni, na, at, bt, ct = lcs
    arrays = [r1cs.flatten(rows, r) for rows in (at, bt, ct)]
    return ni, na, len(at), arrays


def call_upload(r1cs, field, ni, na, nc, arrays, segment=0):
    ms = (r1cs.Matrix * 3)()
    for m, (row_ptr, col, ids, vals) in zip(ms, arrays):
        m.row_ptr, m.col, m.coeff_id, m.coeff_values = P(row_ptr), P(col), P(ids), P(vals)
        m.num_coeffs = 0 if vals is None else len(vals)
    h = V()
    rc = r1cs._lib().gh_r1cs_upload(field, ni, na, nc, ms, segment, ctypes.byref(h))
    return rc, h


def test_symbols_exported_and_declared(gl, r1cs):
    from ginger_lib_amd import ecvrf, gm17_verify, pairing, points, poseidon, schnorr
    lib = gl.load_library()
    for s in r1cs.R1CS_SYMBOLS:
        assert hasattr(lib, s), s
    others = (gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS + schnorr.SCHNORR_SYMBOLS + ecvrf.ECVRF_SYMBOLS +
              pairing.PAIRING_SYMBOLS + gm17_verify.GM17_SYMBOLS + points.POINTS_SYMBOLS)
    assert not set(r1cs.R1CS_SYMBOLS) & set(others)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_r1cs.h")).read()
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(r1cs.R1CS_SYMBOLS) and len(declared) == 10
    assert ctypes.sizeof(r1cs.Info) == 160 and ctypes.sizeof(r1cs.Matrix) == 40


def test_upload_refusals_come_before_any_device_call(gl, r1cs):
    """every refusal of gh_r1cs_upload is GH_E_BAD_ARG / GH_E_UNSUPPORTED on a machine with or without a device; the valid
    upload next to them gets as far as the device (GH_E_NO_DEVICE where there is none)"""
    lib = r1cs._lib()
    r = MODULUS["mnt4753"]
    lcs = ref.random_system(20, 9, r, seed=4)
    ni, na, nc, good = upload_args(r1cs, lcs, r)

    names = "row_ptr col coeff_id coeff_values".split()

    def variant(k, **change):
        arrays = [list(a) for a in good]
        for name, val in change.items():
            arrays[k][names.index(name)] = val
        return [tuple(a) for a in arrays]
    for k in range(3):                                     # the fault in A, B or C
        row_ptr, col, ids, vals = good[k]
        assert len(col) > 2 and row_ptr[4] > 0
        bad_ptr0 = row_ptr.copy(); bad_ptr0[0] = 1
        bad_mono = row_ptr.copy(); bad_mono[4] = bad_mono[3] - 1 if bad_mono[3] else bad_mono[5] + 1
        bad_col = col.copy(); bad_col[1] = ni + na
        bad_id = ids.copy(); bad_id[0] = len(vals)
        bad_val = vals.copy(); bad_val[0] = pyref.int_to_limbs(r)
        refusals = [("null col", dict(col=None)), ("null coeff_id", dict(coeff_id=None)), ("null row_ptr", dict(row_ptr=None)),
                    ("row_ptr[0]", dict(row_ptr=bad_ptr0)), ("monotone", dict(row_ptr=bad_mono)), ("column", dict(col=bad_col)),
                    ("coeff_id", dict(coeff_id=bad_id)), ("modulus", dict(coeff_values=bad_val)), ("null values", dict(coeff_values=None))]
        for name, change in refusals:
            rc, h = call_upload(r1cs, 0, ni, na, nc, variant(k, **change))
            assert rc == GH_E_BAD_ARG and not h.value, (name, k, rc, lib.gh_last_error())
            if name == "modulus":
                assert "modulus" in lib.gh_last_error().decode()
    row_ptr, col, ids, vals = good[1]
    assert call_upload(r1cs, 0, 0, na + ni, nc, good)[0] == GH_E_BAD_ARG                       # num_inputs == 0
    assert call_upload(r1cs, 0, ni, na, nc, good, segment=1)[0] == GH_E_BAD_ARG                # segment_terms == 1
    assert call_upload(r1cs, 7, ni, na, nc, good)[0] == GH_E_BAD_ARG                           # unknown field
    assert r1cs._lib().gh_r1cs_upload(0, ni, na, nc, None, 0, ctypes.byref(V())) == GH_E_BAD_ARG
    # a value below the modulus of MNT4-753 Fr but not of MNT6-753 Fr is judged by the handle's own field
    p4, p6 = MODULUS["mnt6753"], MODULUS["mnt4753"]
    lo, hi = min(p4, p6), max(p4, p6)
    between = vals.copy(); between[0] = pyref.int_to_limbs(lo)
    rcs = [call_upload(r1cs, f, ni, na, nc, variant(1, coeff_values=between))[0] for f in (0, 1)]
    small_field = 0 if p6 == lo else 1
    assert rcs[small_field] == GH_E_BAD_ARG and rcs[1 - small_field] != GH_E_BAD_ARG
    # EvaluationDomain::new(num_constraints + num_inputs) is None from 2^14 + 1 on: MNT6-753 Fr has 2-adicity 15 (domain.rs:69-71)
    n_ok = (1 << 14) - 2                                   # with 2 inputs: exactly 2^14
    empty = lambda n: [(np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), vals)] * 3
    assert call_upload(r1cs, 1, 2, 3, n_ok + 1, empty(n_ok + 1))[0] == GH_E_UNSUPPORTED
    rc_ok, h_ok = call_upload(r1cs, 1, 2, 3, n_ok, empty(n_ok))
    assert rc_ok in (0, GH_E_NO_DEVICE)
    if h_ok.value:
        lib.gh_r1cs_free(h_ok)
    rc, h = call_upload(r1cs, 0, ni, na, nc, good)
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:
        assert rc == GH_E_NO_DEVICE and not h.value
        with pytest.raises(r1cs.GingerHipError):
            r1cs.ResidentR1CS(gl, "mnt4753", lcs)
    else:
        assert rc == 0
        lib.gh_r1cs_free(h)


def test_entry_points_refuse_null_and_foreign_handles(r1cs):
    lib = r1cs._lib()
    buf = np.zeros((4, 12), dtype=np.uint64)
    p = P(buf)
    foreign = V(ctypes.addressof(ctypes.create_string_buffer(4096)))          # memory that is no R1CS handle
    info = r1cs.Info()
    for h in (None, foreign):
        assert lib.gh_r1cs_info(h, ctypes.byref(info)) == GH_E_BAD_HANDLE
        assert lib.gh_r1cs_matvec_dev(h, 0, 0, p, p) == GH_E_BAD_HANDLE
        assert lib.gh_r1cs_evaluate_dev(h, p, p, p, p) == GH_E_BAD_HANDLE
        assert lib.gh_r1cs_evaluate(h, p, p, p, p) == GH_E_BAD_HANDLE
        assert lib.gh_r1cs_witness_map_dev(h, p, p, p, p, p, None) == GH_E_BAD_HANDLE
        assert lib.gh_r1cs_instance_map_dev(h, p, p, p, p) == GH_E_BAD_HANDLE
        assert lib.gh_r1cs_instance_map(h, p, p, p, p) == GH_E_BAD_HANDLE
        assert "R1CS handle" in lib.gh_last_error().decode()
    assert lib.gh_r1cs_free(None) == 0 and lib.gh_r1cs_free(foreign) == GH_E_BAD_HANDLE
    t = (ctypes.c_float * 4)()
    assert lib.gh_r1cs_last_timing(t, 4, None) >= 0 and lib.gh_r1cs_last_timing(None, 4, None) == GH_E_BAD_ARG


def test_package_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "r1cs.py")).read()
    for needle in ("tests/", "import pyref", "r1cs_ref", "groth16_ref", "oracle"):
        assert needle not in txt, needle


# ---- 5. the stand-alone check under the host sanitizers: a program of its own, nothing sanitised is loaded into python
def test_sanitized_standalone_check(tmp_path):
    out = shim_build.sanitized_check("r1cs_check.cpp", str(tmp_path / "r1cs_check"))
    assert out.returncode == 0 and (out.stdout + out.stderr).strip().endswith("ok"), (out.stdout + out.stderr)[-2000:]


# ---- 6. the Rust side (delivered as files: no Rust toolchain checks them here)
def test_rust_r1cs_extern_block_is_generated_from_the_header(r1cs):
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    src = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")
    rs = open(os.path.join(src, "r1cs.rs")).read()
    for s in r1cs.R1CS_SYMBOLS:
        assert "pub fn %s(" % s in rs, s
    assert "pub mod r1cs;" in open(os.path.join(src, "lib.rs")).read()
