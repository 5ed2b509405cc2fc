"""The sparse R1CS products on the device (include/ginger_hip_r1cs.h, ginger-lib_amd/r1cs.py) against the referee of
tests/r1cs_ref.py, and the prover / generator paths above them against the existing paths, byte for byte.  The shapes are the
smallest at which the kernels can still go wrong: segment length 4 unless stated, so that rows of 5, 17 and 65 terms reach the
second and third level of the schedule; both fields.  Every comparison is exact and covers every row."""
import importlib
import random

import numpy as np
import pytest

import pyref
import r1cs_ref as ref
import support as S

pytestmark = pytest.mark.gpu
PAIRINGS = ("mnt4753", "mnt6753")
MODULUS = {"mnt4753": pyref.P6.p, "mnt6753": pyref.P4.p}


@pytest.fixture(scope="module")
def r1cs(gpu):
    return importlib.import_module("ginger_lib_amd.r1cs")


@pytest.fixture(scope="module")
def groth16(gpu):
    return importlib.import_module("ginger_lib_amd.groth16")


def mont(vals, r):
    R = (1 << 768) % r
    return np.array([pyref.int_to_limbs(v * R % r) for v in vals], dtype=np.uint64).reshape(-1, 12)


def ints(rows, r):
    rinv = pow(1 << 768, -1, r)
    return [pyref.limbs_to_int(list(row)) * rinv % r for row in np.asarray(rows, dtype=np.uint64).reshape(-1, 12)]


def ceil_log(t, seg):
    k, cap = 0, 1
    while cap < t:
        cap *= seg
        k += 1
    return k


def check_products(handle, lcs, r, seed):
    """matvec in both orientations for A, B and C against the referee"""
    ni, na, at, bt, ct = lcs
    nv, nc = ni + na, len(at)
    x = ref.hand_built_vector(nv, r, seed=seed)
    u = ref.hand_built_vector(nc, r, seed=seed + 1)
    xm, um = mont(x, r), mont(u, r)
    for which, rows in zip("ABC", (at, bt, ct)):
        assert ints(handle.matvec(which, xm), r) == ref.matvec(rows, x, r), which
        assert ints(handle.matvec(which, um, transpose=True), r) == ref.matvec(rows, u, r, num_out=nv, transpose=True), which + "^T"


# ---- 1. matvec in both orientations on the hand-built system
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_matvec_hand_built_system(gpu, r1cs, pairing):
    r = MODULUS[pairing]
    lcs = ref.hand_built_system(r)
    h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
    try:
        info = h.info()
        assert (info["num_inputs"], info["num_aux"], info["num_constraints"], info["log_n"], info["segment_terms"]) == (3, 67, 130, 8, 4)
        assert info["longest_row"]["A"][0] == 65 and info["levels"]["A"][0] == ceil_log(65, 4) == 4    # 17, 5, 2 partials, then one
        long_column = sum(1 for row in lcs[2] for _, ix in row if ix == 2)
        assert info["longest_row"]["A"][1] == long_column >= 100 and info["levels"]["A"][1] == ceil_log(long_column, 4)
        assert all(info["class_counts"][c] > 0 for c in r1cs.CLASSES) and info["device_bytes"] > 0
        assert info["nnz"]["A"][0] == info["nnz"]["A"][1] == sum(len(row) for row in lcs[2])
        check_products(h, lcs, r, seed=3)
    finally:
        h.free()


# ---- 2. the wave and block edges, and a matrix without terms
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_matvec_wave_and_block_edges(gpu, r1cs, pairing):
    r = MODULUS[pairing]
    cases = [ref.random_system(nc, 9, r, seed=nc) for nc in (1, 63, 64, 65, 130)]
    cases.append((2, 7, [[] for _ in range(9)], [[] for _ in range(9)], [[] for _ in range(9)]))       # nnz = 0
    for lcs in cases:
        h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
        try:
            check_products(h, lcs, r, seed=len(lcs[2]))
        finally:
            h.free()


# ---- 3. evaluate: tail rows and padding over buffers that held 0xFF
@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("nc", [61, 62])                   # nc + num_inputs = 64 exactly, and 65: the domain doubles
def test_evaluate_writes_inputs_and_padding(gpu, r1cs, pairing, nc):
    r = MODULUS[pairing]
    lcs = ref.random_system(nc, 12, r, seed=40 + nc, max_terms=9, num_inputs=3)
    z = ref.hand_built_vector(12, r, seed=nc)
    z[0] = 5                                               # a[nc] is the constant one whatever the caller put into z_0
    want = ref.evaluate(lcs, z, r)
    size = ref.domain_size(nc, 3)
    assert size == (64 if nc == 61 else 128)
    h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
    d_z = gpu.DeviceBuffer(12 * 96).upload(mont(z, r))
    outs = [gpu.DeviceBuffer(size * 96).upload(np.full(size * 96, 0xFF, dtype=np.uint8)) for _ in range(3)]
    try:
        assert h.size == size
        h.evaluate_dev(d_z, *outs)
        got = [o.download().reshape(size, 12) for o in outs]
        for g, w, name in zip(got, want, "abc"):
            assert ints(g, r) == w, name
        assert ints(got[0][nc:nc + 3], r) == [1, z[1], z[2]]
        assert not got[0][nc + 3:].any() and not got[1][nc:].any() and not got[2][nc:].any()
        host = h.evaluate(mont(z, r))                      # the host-pointer form
        assert all((a == b).all() for a, b in zip(host, got))
    finally:
        for buf in [d_z] + outs:
            buf.free()
        h.free()


# ---- 4. the default segment length on a long row; two handles alive with different segment lengths
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_default_segment_on_the_benchmark_circuits_closing_row(gpu, r1cs, groth16, pairing):
    r = MODULUS[pairing]
    n = 1100
    lcs = groth16.benchmark_circuit_lcs(n)
    assert len(lcs[2][-1]) == n + 1 and [ix for _, ix in lcs[2][-1]].count(1) == 2        # 1101 terms, variable 1 listed twice
    assignment = groth16.benchmark_circuit_rows(pairing, n)[1]
    want = ref.evaluate(lcs, assignment, r)
    zm = mont(assignment, r)
    h4 = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
    h0 = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=0)
    try:
        seg = h0.info()["segment_terms"]
        assert seg >= 2 and n + 1 > seg                    # the closing row needs at least two levels at the default
        assert h0.info()["levels"]["A"][0] >= 2 and h0.info()["levels"]["B"][0] >= 2
        assert h0.info()["levels"]["A"][0] == ceil_log(n + 1, seg)
        assert h4.info()["levels"]["A"][0] == 6            # 4^5 < 1101 <= 4^6
        got0, got4 = h0.evaluate(zm), h4.evaluate(zm)
        for g0, g4, w, name in zip(got0, got4, want, "abc"):
            assert ints(g0, r) == w, name
            assert (g0 == g4).all(), name
    finally:
        h4.free()
        h0.free()


# ---- 5. instance_map
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_instance_map(gpu, r1cs, groth16, pairing):
    r = MODULUS[pairing]
    rng = random.Random(17)
    for lcs in (ref.hand_built_system(r), groth16.benchmark_circuit_lcs(253)):
        h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
        try:
            u = [rng.randrange(r) for _ in range(h.size)]
            want = ref.instance_map(lcs, u, r)
            assert any(want[0][i] != ref.matvec(lcs[2], u, r, num_out=lcs[0] + lcs[1], transpose=True)[i] for i in range(lcs[0]))
            got = h.instance_map(mont(u, r))
            for g, w, name in zip(got, want, "abc"):
                assert ints(g, r) == w, name
        finally:
            h.free()


# ---- 6. create_proof_r1cs end to end
_KEYS = {}


def proving_parameters(gpu, groth16, pairing, n):
    """(Parameters::write bytes, lcs) of the Benchmark circuit with n constraints, made once by the device generator"""
    if (pairing, n) not in _KEYS:
        C1, C2 = pyref.CURVES[pairing + "_g1"], pyref.CURVES[pairing + "_g2"]
        rng = pyref.Rng(1000 + n)
        alpha, beta, gamma, delta, t = (rng.field_elem(MODULUS[pairing]) for _ in range(5))
        g1, g2 = C1.mul(rng.next_u64() | 1, C1.G), C2.mul(rng.next_u64() | 1, C2.G)
        lcs = groth16.benchmark_circuit_lcs(n)
        args = (alpha, beta, gamma, delta, t, S.proj_array(C1, g1), S.proj_array(C2, g2))
        blob, _ = groth16.generate_parameters(gpu, pairing, lcs, *args)
        _KEYS[(pairing, n)] = (blob, lcs, args)
    return _KEYS[(pairing, n)]


@pytest.mark.parametrize("pairing", PAIRINGS)
@pytest.mark.parametrize("n", [13, 253])
def test_create_proof_r1cs_equals_create_proof(gpu, r1cs, groth16, pairing, n):
    r = MODULUS[pairing]
    blob, lcs, _ = proving_parameters(gpu, groth16, pairing, n)
    rows = groth16.benchmark_circuit_rows(pairing, n)
    rng = pyref.Rng(7 * n)
    blind = [tuple(rng.field_elem(r) for _ in range(5))]
    if n == 13:
        blind.append((0, 0, 0) + tuple(rng.field_elem(r) for _ in range(2)))              # d1 = d2 = d3 = 0
    h = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
    zm = mont(rows[1], r)
    try:
        for precompute in (False, True):
            key = groth16.ResidentProvingKey.from_parameters(gpu, pairing, blob, rows[0], precompute=precompute)
            try:
                for d1, d2, d3, r_, s_ in blind:
                    want = key.create_proof(rows, d1, d2, d3, r_, s_)
                    timing = {}
                    assert key.create_proof_r1cs(h, zm, d1, d2, d3, r_, s_, timing=timing) == want, (precompute, d1)
                    assert set(timing) == {"assignment_upload_ms", "witness_map_ms", "msm_stage_ms"}
                assert key.create_proof_r1cs(h, rows[1], *blind[-1]) == want               # an assignment of integers is converted first
            finally:
                key.free()
    finally:
        h.free()
    gpu.dev_trim()


# ---- 7. generate_parameters over the resident matrices
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_generate_parameters_with_r1cs_emits_the_same_bytes(gpu, r1cs, groth16, pairing):
    blob, lcs, args = proving_parameters(gpu, groth16, pairing, 61)
    h = r1cs.ResidentR1CS(gpu, pairing, lcs)
    try:
        blob_r, info = groth16.generate_parameters(gpu, pairing, lcs, *args, r1cs=h)
        assert blob_r == blob and info["log_n"] == 6
        other = r1cs.ResidentR1CS(gpu, pairing, groth16.benchmark_circuit_lcs(13))
        try:
            with pytest.raises(ValueError):
                groth16.generate_parameters(gpu, pairing, lcs, *args, r1cs=other)
        finally:
            other.free()
    finally:
        h.free()
    gpu.dev_trim()


# ---- 8. independence and lifetime
def test_handles_are_independent_and_survive_a_trim(gpu, r1cs):
    pairing = "mnt4753"
    r = MODULUS[pairing]
    lcs = ref.hand_built_system(r)
    small = ref.random_system(65, 9, r, seed=65)
    x = mont(ref.hand_built_vector(70, r), r)
    a = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=4)
    b = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=7)
    c = r1cs.ResidentR1CS(gpu, "mnt6753", small, segment_terms=2)
    try:
        assert a.info()["levels"]["A"][0] == 4 and b.info()["levels"]["A"][0] == 3 and (a.info()["segment_terms"], b.info()["segment_terms"]) == (4, 7)
        ya = a.matvec("A", x)
        assert (b.matvec("A", x) == ya).all()
        check_products(c, small, MODULUS["mnt6753"], seed=1)                  # another field in between
        b.free()                                                             # free, then reuse the others
        b.free()
        assert (a.matvec("A", x) == ya).all()
        gpu.dev_trim()                                                       # the products' scratch comes from the pool
        assert (a.matvec("A", x) == ya).all()
        d = r1cs.ResidentR1CS(gpu, pairing, lcs, segment_terms=32)
        try:
            assert d.info()["levels"]["A"][0] == 2 and (d.matvec("A", x) == ya).all()
        finally:
            d.free()
        phases, total = r1cs.last_timing()
        assert len(phases) >= 3 and total >= 0
    finally:
        a.free()
        c.free()
