"""GM17's R1CS -> SAP maps on the device (include/ginger_hip_sap.h, ginger-lib_amd/sap.py) against the referee of
tests/sap_ref.py, and the prover / generator paths above them against the existing host paths, byte for byte.  The shapes are
sap_ref.cases: the smallest at which the kernels can still go wrong, at segment length 4 so that the products reach their upper
levels; both fields.  Every comparison is exact and covers every row; output buffers hold 0xFF before a call."""
import importlib
import random

import numpy as np
import pytest

import pyref
import r1cs_ref
import sap_ref as ref
import support as S

pytestmark = pytest.mark.gpu
PAIRINGS = ("mnt4753", "mnt6753")
MODULUS = {"mnt4753": pyref.P6.p, "mnt6753": pyref.P4.p}
GH_E_BAD_ARG = -1


@pytest.fixture(scope="module")
def r1cs(gpu):
    return importlib.import_module("ginger_lib_amd.r1cs")


@pytest.fixture(scope="module")
def sap(gpu):
    return importlib.import_module("ginger_lib_amd.sap")


@pytest.fixture(scope="module")
def groth16(gpu):
    return importlib.import_module("ginger_lib_amd.groth16")


@pytest.fixture(scope="module")
def gm17(gpu):
    return importlib.import_module("ginger_lib_amd.gm17")


def mont(vals, r):
    R = (1 << 768) % r
    return np.array([pyref.int_to_limbs(v * R % r) for v in vals], dtype=np.uint64).reshape(-1, 12)


def ints(rows, r):
    rinv = pow(1 << 768, -1, r)
    return [pyref.limbs_to_int(list(row)) * rinv % r for row in np.asarray(rows, dtype=np.uint64).reshape(-1, 12)]


def plain(rows):
    return [pyref.limbs_to_int(list(row)) for row in np.asarray(rows, dtype=np.uint64).reshape(-1, 12)]


def filled(gpu, rows):
    """a device buffer of `rows` rows (at least one) that holds 0xFF"""
    n = max(rows, 1) * 96
    return gpu.DeviceBuffer(n).upload(np.full(n, 0xFF, dtype=np.uint8))


def rows_of(buf, rows):
    return buf.download()[:rows * 12].reshape(rows, 12)


# ---- 1. the rows, with and without each scalar destination
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_rows_equal_referee(gpu, r1cs, sap, pairing):
    r = MODULUS[pairing]
    for name, lcs in ref.cases(r):
        ni, nc = lcs[0], len(lcs[2])
        nv, sap_nv, size = ni + lcs[1], ref.sap_num_variables(lcs), ref.domain_size(nc, ni)
        n_aux = sap_nv - (ni - 1)
        z = r1cs_ref.hand_built_vector(nv, r, seed=len(name))
        full, a, c = ref.rows(lcs, z, r)
        h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
        d_z = gpu.DeviceBuffer(nv * 96).upload(mont(z, r))
        try:
            info = sap.sap_info(h)
            assert (info["size"], info["sap_num_variables"]) == (size, sap_nv) and info["scratch_bytes"] > 2 * size * 96, name
            for with_s, with_x in ((False, False), (True, False), (False, True), (True, True)):
                bufs = [filled(gpu, n) for n in (size, size, sap_nv, n_aux)]
                try:
                    sap.sap_rows_dev(h, d_z, bufs[0], bufs[1], bufs[2] if with_s else None, bufs[3] if with_x else None)
                    assert ints(rows_of(bufs[0], size), r) == a and ints(rows_of(bufs[1], size), r) == c, (name, with_s, with_x)
                    got_s, got_x = rows_of(bufs[2], sap_nv), rows_of(bufs[3], n_aux)
                    if with_s:
                        assert plain(got_s) == full[1:], name
                    else:
                        assert (got_s == 0xFFFFFFFFFFFFFFFF).all(), name
                    if with_x:
                        assert plain(got_x) == full[ni:], name
                    else:
                        assert (got_x == 0xFFFFFFFFFFFFFFFF).all(), name
                    if with_s and with_x:
                        assert (got_s[ni - 1:] == got_x).all(), name        # the two scalar outputs agree row for row
                finally:
                    for b in bufs:
                        b.free()
            g_full, g_a, g_c = sap.sap_rows(h, mont(z, r))                       # the host-pointer form
            assert ints(g_full, r) == full and ints(g_a, r) == a and ints(g_c, r) == c, name
            phases, total = sap.last_timing()
            assert len(phases) >= 3 and total >= 0
        finally:
            d_z.free()
            h.free()


# ---- 2. the instance map
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_instance_map_equals_referee(gpu, r1cs, sap, pairing):
    r = MODULUS[pairing]
    rng = random.Random(23)
    for name, lcs in ref.cases(r):
        ni, nc = lcs[0], len(lcs[2])
        nv, rows, size = ni + lcs[1], ref.sap_num_variables(lcs) + 1, ref.domain_size(nc, ni)
        u = [rng.randrange(r) for _ in range(size)]
        want_a, want_c = ref.instance_map(lcs, u, r)
        if ni > 1:
            assert want_a[0] != (r1cs_ref.matvec(lcs[2], [(u[2 * i] + u[2 * i + 1]) % r for i in range(nc)], r, num_out=nv, transpose=True)[0] +
                                 r1cs_ref.matvec(lcs[3], [(u[2 * i] - u[2 * i + 1]) % r for i in range(nc)], r, num_out=nv, transpose=True)[0]) % r
        h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
        d_u = gpu.DeviceBuffer(size * 96).upload(mont(u, r))
        d_a, d_c = filled(gpu, rows), filled(gpu, rows)
        try:
            sap.sap_instance_map_dev(h, d_u, d_a, d_c)
            got_a, got_c = rows_of(d_a, rows), rows_of(d_c, rows)
            assert ints(got_a, r) == want_a and ints(got_c, r) == want_c, name
            assert not got_a[nv:].any(), name                                    # the extra variables do not occur in A
            host = sap.sap_instance_map(h, mont(u, r))                           # the host-pointer form
            assert (host[0] == got_a).all() and (host[1] == got_c).all(), name
        finally:
            for b in (d_u, d_a, d_c):
                b.free()
            h.free()


def test_null_pointers_and_wrong_sizes_are_refused(gpu, r1cs, sap):
    r = MODULUS["mnt4753"]
    lcs = r1cs_ref.random_system(20, 9, r, seed=4)
    h = r1cs.ResidentR1CS(gpu, "mnt4753", lcs)
    buf = gpu.DeviceBuffer(64 * 96)
    try:
        lib = sap._lib()
        assert lib.gh_sap_rows_dev(h.handle, None, buf.ptr, buf.ptr, None, None) == GH_E_BAD_ARG
        assert lib.gh_sap_instance_map_dev(h.handle, buf.ptr, None, buf.ptr) == GH_E_BAD_ARG
        assert lib.gh_sap_r1cs_witness_map_dev(h.handle, buf.ptr, None, None, buf.ptr, None, None) == GH_E_BAD_ARG
        with pytest.raises(ValueError):
            sap.sap_rows(h, np.zeros((8, 12), dtype=np.uint64))
        with pytest.raises(ValueError):
            sap.sap_instance_map(h, np.zeros((32, 12), dtype=np.uint64))
    finally:
        buf.free()
        h.free()


# ---- 3. create_proof_r1cs end to end
_KEYS = {}


def gm17_parameters(gpu, gm17, groth16, pairing, n):
    """(pk, info, lcs, args) of the Benchmark circuit with n constraints, made once by the device generator: a real key, with the
    `_inf` flags of the extra variables"""
    if (pairing, n) not in _KEYS:
        C1, C2 = pyref.CURVES[pairing + "_g1"], pyref.CURVES[pairing + "_g2"]
        rng = pyref.Rng(2000 + n)
        alpha, beta, gamma, t = (rng.field_elem(MODULUS[pairing]) for _ in range(4))
        g1, g2 = C1.mul(rng.next_u64() | 1, C1.G), C2.mul(rng.next_u64() | 1, C2.G)
        lcs = groth16.benchmark_circuit_lcs(n)
        args = (alpha, beta, gamma, t, S.proj_array(C1, g1), S.proj_array(C2, g2))
        pk, info = gm17.generate_parameters(gpu, pairing, lcs, *args)
        assert pk["a_query_inf"].any()
        _KEYS[(pairing, n)] = (pk, info, lcs, args)
    return _KEYS[(pairing, n)]


@pytest.mark.parametrize("pairing,n", [("mnt4753", 13), ("mnt4753", 253), ("mnt6753", 125)])
def test_create_proof_r1cs_equals_create_proof(gpu, r1cs, gm17, groth16, pairing, n):
    r = MODULUS[pairing]
    pk, _, lcs, _ = gm17_parameters(gpu, gm17, groth16, pairing, n)
    rows = groth16.benchmark_circuit_rows(pairing, n)
    rng = pyref.Rng(11 * n)
    blind = [tuple(rng.field_elem(r) for _ in range(3))]
    if n == 13:
        blind.append((0, 0, rng.field_elem(r)))                                  # d1 = d2 = 0
    h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
    zm = mont(rows[1], r)
    try:
        for precompute in (False, True):
            key = gm17.ResidentGm17Key(gpu, pairing, pk, rows[0], precompute=precompute)
            try:
                for d1, d2, r_ in blind:
                    want = gm17.proof_bytes(pairing, key.create_proof(rows, d1, d2, r_))
                    timing = {}
                    got = key.create_proof_r1cs(h, zm, d1, d2, r_, timing=timing)
                    assert gm17.proof_bytes(pairing, got) == want, (precompute, d1)
                    assert set(timing) == {"assignment_upload_ms", "witness_map_ms", "msm_stage_ms"}
                assert gm17.proof_bytes(pairing, key.create_proof_r1cs(h, rows[1], *blind[-1])) == want      # integers are converted first
            finally:
                key.free()
    finally:
        h.free()
    gpu.dev_trim()


# ---- 4. generate_parameters over the resident matrices
@pytest.mark.parametrize("pairing,n", [("mnt4753", 13), ("mnt6753", 125)])
def test_generate_parameters_with_r1cs_returns_the_same_key(gpu, r1cs, gm17, groth16, pairing, n):
    pk, info, lcs, args = gm17_parameters(gpu, gm17, groth16, pairing, n)
    h = r1cs.ResidentR1CS(gpu, pairing, lcs)
    try:
        pk_r, info_r = gm17.generate_parameters(gpu, pairing, lcs, *args, r1cs=h)
        assert sorted(pk_r) == sorted(pk)
        for name in pk:
            assert (np.asarray(pk_r[name]) == np.asarray(pk[name])).all(), name
        assert info_r == info
        other = r1cs.ResidentR1CS(gpu, pairing, groth16.benchmark_circuit_lcs(n + 2))
        try:
            with pytest.raises(ValueError):
                gm17.generate_parameters(gpu, pairing, lcs, *args, r1cs=other)
        finally:
            other.free()
    finally:
        h.free()
    gpu.dev_trim()


# ---- 5. one handle behind both provers: the shared scratch is sized for both, before and after a trim
def test_one_handle_serves_groth16_then_gm17_and_survives_a_trim(gpu, r1cs, gm17, groth16):
    pairing, n = "mnt4753", 13
    r = MODULUS[pairing]
    pk, _, lcs, (alpha, beta, gamma, t, g1_xyz, g2_xyz) = gm17_parameters(gpu, gm17, groth16, pairing, n)
    rows = groth16.benchmark_circuit_rows(pairing, n)
    blob, _ = groth16.generate_parameters(gpu, pairing, lcs, alpha, beta, gamma, (alpha + 1) % r, t, g1_xyz, g2_xyz)
    zm = mont(rows[1], r)
    h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
    k16 = groth16.ResidentProvingKey.from_parameters(gpu, pairing, blob, rows[0])
    k17 = gm17.ResidentGm17Key(gpu, pairing, pk, rows[0])
    try:
        assert k16.create_proof_r1cs(h, zm, 1, 2, 3, 4, 5) == k16.create_proof(rows, 1, 2, 3, 4, 5)
        want = gm17.proof_bytes(pairing, k17.create_proof(rows, 6, 7, 8))
        assert gm17.proof_bytes(pairing, k17.create_proof_r1cs(h, zm, 6, 7, 8)) == want
        gpu.dev_trim()
        assert gm17.proof_bytes(pairing, k17.create_proof_r1cs(h, zm, 6, 7, 8)) == want
        assert k16.create_proof_r1cs(h, zm, 1, 2, 3, 4, 5) == k16.create_proof(rows, 1, 2, 3, 4, 5)
    finally:
        k16.free()
        k17.free()
        h.free()
    gpu.dev_trim()
