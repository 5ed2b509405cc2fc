"""GM17's R1CS -> SAP maps without a GPU: the referee (tests/sap_ref.py) against the existing host path, the lanes of
ginger-lib_amd/csrc/sap_rows.h compiled by g++ (tests/host_shim/sap_shim.cpp) over the host executor's products against the
referee on the shapes the GPU tests run, the handle checks of include/ginger_hip_sap.h, the stand-alone sanitised check and
the generated Rust block.  Every comparison is exact."""
import ctypes
import importlib
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import pyref
import r1cs_ref
import sap_ref as ref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_BAD_ARG, GH_E_UNSUPPORTED, GH_E_NO_DEVICE, GH_E_BAD_HANDLE = -1, -2, -3, -6
V = ctypes.c_void_p
U64, U32 = ctypes.c_uint64, ctypes.c_uint32
PAIRINGS = ("mnt4753", "mnt6753")
FIELD_ID = {"mnt4753": 0, "mnt6753": 1}
MODULUS = {"mnt4753": pyref.P6.p, "mnt6753": pyref.P4.p}         # the scalar field of a pairing is the other curve's base field


@pytest.fixture(scope="module")
def r1cs(gl):
    return importlib.import_module("ginger_lib_amd.r1cs")


@pytest.fixture(scope="module")
def sap(gl):
    return importlib.import_module("ginger_lib_amd.sap")


@pytest.fixture(scope="module")
def mods(gl):
    return importlib.import_module("ginger_lib_amd.groth16"), importlib.import_module("ginger_lib_amd.gm17")


@pytest.fixture(scope="module")
def shim(r1cs):
    lib = shim_build.host_shim("sap")
    M = ctypes.POINTER(r1cs.Matrix)
    lib.sap_shim_info.argtypes = [ctypes.c_int, U64, U64, U64, ctypes.POINTER(U32), ctypes.POINTER(U64), ctypes.POINTER(U64)]
    lib.sap_shim_rows.argtypes = [ctypes.c_int, U64, U64, U64, M, U32, V, V, V, V, V, V]
    lib.sap_shim_instance_map.argtypes = [ctypes.c_int, U64, U64, U64, M, U32, V, V, V]
    return lib


def P(a):
    return a.ctypes.data_as(V) if a is not None and a.size else None


def mont(vals, r):
    R = (1 << 768) % r
    return np.array([pyref.int_to_limbs(v * R % r) for v in vals], dtype=np.uint64).reshape(-1, 12)


def ints(rows, r):
    rinv = pow(1 << 768, -1, r)
    return [pyref.limbs_to_int(list(row)) * rinv % r for row in np.asarray(rows, dtype=np.uint64).reshape(-1, 12)]


def plain(rows):
    return [pyref.limbs_to_int(list(row)) for row in np.asarray(rows, dtype=np.uint64).reshape(-1, 12)]


def matrices(r1cs, lcs, r):
    """(the three gh_r1cs_matrix_t, the arrays they point into)"""
    keep = [r1cs.flatten(rows, r) for rows in lcs[2:]]
    ms = (r1cs.Matrix * 3)()
    for m, (row_ptr, col, ids, vals) in zip(ms, keep):
        m.row_ptr, m.col, m.coeff_id, m.coeff_values, m.num_coeffs = P(row_ptr), P(col), P(ids), P(vals), len(vals)
    return ms, keep


def filled(rows):
    return np.full((max(rows, 1), 12), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


# ---- 1. the referee against the existing path
def referee_systems(groth16, pairing):
    """(lcs, assignment): the Benchmark circuit at its own witness, and random systems with empty rows, repeated indices
    (r1cs_ref.random_system draws both) and 1, 2 and 5 inputs"""
    r = MODULUS[pairing]
    out = [(groth16.benchmark_circuit_lcs(n), groth16.benchmark_circuit_rows(pairing, n)[1]) for n in (13, 125)]
    for ni in (1, 2, 5):
        lcs = r1cs_ref.random_system(40, 11, r, seed=ni, max_terms=6, num_inputs=ni)
        assert any(not row for row in lcs[2]) and any(len({ix for _, ix in row}) < len(row) for row in lcs[2])
        out.append((lcs, r1cs_ref.hand_built_vector(11, r, seed=ni)))
    return out


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_referee_rows_equal_sap_rows_from_r1cs(mods, pairing):
    groth16, gm17 = mods
    r = MODULUS[pairing]
    for lcs, z in referee_systems(groth16, pairing):
        ni, nc = lcs[0], len(lcs[2])
        A, B, C = (r1cs_ref.matvec(rows, z, r) for rows in lcs[2:])
        full, a, c, log_n = gm17.sap_rows_from_r1cs(pairing, ni, z, A, B, C)
        got = ref.rows(lcs, z, r)
        assert got == (full, a, c)
        assert 1 << log_n == ref.domain_size(nc, ni) == len(got[1]) and len(full) == ref.sap_num_variables(lcs) + 1


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_referee_instance_map_equals_the_generators_loop(mods, pairing):
    groth16, gm17 = mods
    r = MODULUS[pairing]
    rng = random.Random(3)
    for lcs, _ in referee_systems(groth16, pairing):
        u = [rng.randrange(r) for _ in range(ref.domain_size(len(lcs[2]), lcs[0]))]
        assert ref.instance_map(lcs, u, r) == gm17.sap_instance_map_host(lcs, u, r)


@pytest.mark.parametrize("pairing", PAIRINGS)
def test_referee_rows_square_to_c_for_a_satisfying_assignment(mods, pairing):
    groth16, _ = mods
    r = MODULUS[pairing]
    systems = [(groth16.benchmark_circuit_lcs(13), groth16.benchmark_circuit_rows(pairing, 13)[1]), ref.satisfying_system(33, 12, r, seed=8, num_inputs=4)]
    for lcs, z in systems:
        _, a, c = ref.rows(lcs, z, r)
        used = 2 * len(lcs[2]) + 2 * (lcs[0] - 1) + 1
        assert all(x * x % r == y for x, y in zip(a[:used], c[:used]))
        assert not any(a[used:]) and not any(c[used:])
    lcs, z = systems[1]
    z[5] = (z[5] + 1) % r                                   # and not for another one
    _, a, c = ref.rows(lcs, z, r)
    assert any(x * x % r != y for x, y in zip(a, c))


# ---- 2. the lanes of sap_rows.h over the host executor's products, on the shapes of the GPU tests
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_host_lanes_equal_referee(shim, r1cs, pairing):
    r = MODULUS[pairing]
    rng = random.Random(11)
    for name, lcs in ref.cases(r):
        ni, na, nc = lcs[0], lcs[1], len(lcs[2])
        nv, sap_nv, size = ni + na, ref.sap_num_variables(lcs), ref.domain_size(nc, ni)
        log_n, got_nv, lanes = U32(), U64(), U64()
        assert shim.sap_shim_info(FIELD_ID[pairing], ni, na, nc, log_n, got_nv, lanes) == 0
        assert (1 << log_n.value, got_nv.value, lanes.value) == (size, sap_nv, size - nc - ni + 1), name
        ms, keep = matrices(r1cs, lcs, r)
        z = r1cs_ref.hand_built_vector(nv, r, seed=len(name))
        full, a, c = ref.rows(lcs, z, r)
        for with_scalars in (False, True):
            ga, gc, gs, gx, gf = filled(size), filled(size), filled(sap_nv), filled(sap_nv - (ni - 1)), filled(sap_nv + 1)
            assert shim.sap_shim_rows(FIELD_ID[pairing], ni, na, nc, ms, 4, P(mont(z, r)), P(ga), P(gc), P(gs) if with_scalars else None,
                                      P(gx) if with_scalars else None, None if with_scalars else P(gf)) == 0
            assert ints(ga, r) == a and ints(gc, r) == c, name
            if with_scalars:
                assert plain(gs[:sap_nv]) == full[1:] and plain(gx[:sap_nv - (ni - 1)]) == full[ni:], name
            else:
                assert ints(gf, r) == full, name
        u = [rng.randrange(r) for _ in range(size)]
        ga, gc = filled(sap_nv + 1), filled(sap_nv + 1)
        assert shim.sap_shim_instance_map(FIELD_ID[pairing], ni, na, nc, ms, 4, P(mont(u, r)), P(ga), P(gc)) == 0
        assert (ints(ga, r), ints(gc, r)) == ref.instance_map(lcs, u, r), name
        assert not ga[nv:].any(), name                      # the extra variables do not occur in A


def test_shim_domain_refusal(shim):
    """EvaluationDomain::new(2 nc + 2 (ni - 1) + 1) is None from 2^14 + 1 on over MNT6-753 Fr (2-adicity 15)"""
    out = (U32(), U64(), U64())
    assert shim.sap_shim_info(1, 3, 0, (1 << 13) - 3, *out) == 0 and out[0].value == 14
    assert shim.sap_shim_info(1, 3, 0, (1 << 13) - 2, *out) == GH_E_UNSUPPORTED
    assert shim.sap_shim_info(0, 3, 0, (1 << 13) - 2, *out) == 0 and out[0].value == 15


# ---- 3. the C ABI without a device
def test_symbols_exported_and_declared(gl, r1cs, sap):
    from ginger_lib_amd import ecvrf, gm17_verify, pairing, points, poseidon, schnorr
    lib = gl.load_library()
    for s in sap.SAP_SYMBOLS:
        assert hasattr(lib, s), s
    others = (gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS + schnorr.SCHNORR_SYMBOLS + ecvrf.ECVRF_SYMBOLS +
              pairing.PAIRING_SYMBOLS + gm17_verify.GM17_SYMBOLS + points.POINTS_SYMBOLS + r1cs.R1CS_SYMBOLS)
    assert not set(sap.SAP_SYMBOLS) & set(others)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_sap.h")).read()
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(sap.SAP_SYMBOLS) and len(declared) == 7
    assert ctypes.sizeof(sap.Info) == 24
    for name, types in sap._ARGTYPES.items():               # one ctypes argument per parameter of the prototype
        params = re.search(r"^int %s\(([^;]*?)\);" % name, hdr, re.M | re.S).group(1)
        assert len(types) == params.count(",") + 1, name


def test_entry_points_refuse_null_and_foreign_handles(sap):
    lib = sap._lib()
    buf = np.zeros((4, 12), dtype=np.uint64)
    p = P(buf)
    foreign = V(ctypes.addressof(ctypes.create_string_buffer(4096)))          # memory that is no R1CS handle
    info = sap.Info()
    for h in (None, foreign):
        assert lib.gh_sap_info(h, ctypes.byref(info)) == GH_E_BAD_HANDLE
        assert lib.gh_sap_rows_dev(h, p, p, p, None, None) == GH_E_BAD_HANDLE
        assert lib.gh_sap_rows(h, p, p, p, p) == GH_E_BAD_HANDLE
        assert lib.gh_sap_r1cs_witness_map_dev(h, p, p, p, p, None, None) == GH_E_BAD_HANDLE
        assert lib.gh_sap_instance_map_dev(h, p, p, p) == GH_E_BAD_HANDLE
        assert lib.gh_sap_instance_map(h, p, p, p) == GH_E_BAD_HANDLE
        assert "R1CS handle" in lib.gh_last_error().decode()
    t = (ctypes.c_float * 4)()
    assert lib.gh_sap_last_timing(t, 4, None) >= 0 and lib.gh_sap_last_timing(None, 4, None) == GH_E_BAD_ARG


def test_valid_calls_reach_the_device_or_report_its_absence(gl, r1cs, sap):
    """a handle exists only where a device does: without one the upload itself is GH_E_NO_DEVICE and the wrappers raise; with
    one, null pointers are GH_E_BAD_ARG and a domain beyond the field's 2-adicity GH_E_UNSUPPORTED, on a live handle"""
    lib = sap._lib()
    r = MODULUS["mnt6753"]
    lcs = r1cs_ref.random_system(20, 9, r, seed=4)
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:
        with pytest.raises(r1cs.GingerHipError):
            r1cs.ResidentR1CS(gl, "mnt6753", lcs)
        return
    h = r1cs.ResidentR1CS(gl, "mnt6753", lcs)
    nc = (1 << 13) - 2                                      # the QAP domain 2^13 + 1 fits, the SAP domain 2^14 + 1 does not
    empty = (np.zeros(nc + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((1, 12), dtype=np.uint64))
    big = r1cs.ResidentR1CS.from_csr(gl, "mnt6753", 3, 0, nc, [empty] * 3)
    try:
        buf = np.zeros((64, 12), dtype=np.uint64)
        p = P(buf)
        assert lib.gh_sap_info(h.handle, None) == GH_E_BAD_ARG
        assert lib.gh_sap_rows_dev(h.handle, None, p, p, None, None) == GH_E_BAD_ARG
        assert lib.gh_sap_rows(h.handle, p, p, p, None) == GH_E_BAD_ARG
        assert lib.gh_sap_r1cs_witness_map_dev(h.handle, p, None, p, p, None, None) == GH_E_BAD_ARG
        assert lib.gh_sap_instance_map_dev(h.handle, p, None, p) == GH_E_BAD_ARG
        assert lib.gh_sap_instance_map(h.handle, p, p, None) == GH_E_BAD_ARG
        assert sap.sap_info(h)["sap_log_n"] == 6 and sap.sap_info(h)["sap_num_variables"] == 2 + 7 + 20
        info = sap.Info()
        assert lib.gh_sap_info(big.handle, ctypes.byref(info)) == GH_E_UNSUPPORTED
        assert lib.gh_sap_rows_dev(big.handle, p, p, p, None, None) == GH_E_UNSUPPORTED
        assert lib.gh_sap_instance_map_dev(big.handle, p, p, p) == GH_E_UNSUPPORTED
    finally:
        h.free()
        big.free()


def test_package_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "sap.py")).read()
    for needle in ("tests/", "import pyref", "r1cs_ref", "sap_ref", "oracle"):
        assert needle not in txt, needle


# ---- 4. the stand-alone check under the host sanitizers: a program of its own, nothing sanitised is loaded into python
def test_sanitized_standalone_check(tmp_path):
    out = shim_build.sanitized_check("sap_check.cpp", str(tmp_path / "sap_check"))
    assert out.returncode == 0 and (out.stdout + out.stderr).strip().endswith("ok"), (out.stdout + out.stderr)[-2000:]


# ---- 5. the Rust side (delivered as files: no Rust toolchain checks them here)
def test_rust_sap_extern_block_is_generated_from_the_header(sap):
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    src = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")
    rs = open(os.path.join(src, "sap.rs")).read()
    for s in sap.SAP_SYMBOLS:
        assert "pub fn %s(" % s in rs, s
    assert "pub struct GhSapInfo" in rs and "pub mod sap;" in open(os.path.join(src, "lib.rs")).read()
