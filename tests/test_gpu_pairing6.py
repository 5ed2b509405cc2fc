"""Batched MNT6-753 pairings and Groth16 verification on the device (engine 2 of include/ginger_hip_pairing.h through
ginger-lib_amd/pairing.py) against the Python restatement tests/pairing_ref.py (engine "mnt6753"), which is pinned to the
reference's known answer by tests/test_pairing_host.py.  The tests that both engines share are tests/pairing_device_cases.py's.
Every comparison is exact integer equality on the value after the final exponentiation; no row is skipped."""
import importlib
import random

import numpy as np
import pytest

import pairing_device_cases as shared
import pairing_ref
import pyref
from groth16_exp_key import ExpKey

pytestmark = pytest.mark.gpu
ENGINE = "mnt6753"
pr = pairing_ref.engine(ENGINE)
C1, C2, r = pr.C1, pr.C2, pr.r
g1_batch, g2_batch = pr.g1_batch, pr.g2_batch


@pytest.fixture(scope="module")
def pairing(gpu):
    return importlib.import_module("ginger_lib_amd.pairing")


# ---- 1. the reference's known answer (curves/mnt6753/tests.rs:319-590)
def test_known_answer(pairing):
    shared.known_answer(pairing, pr)


# ---- 2. bilinearity at wave and block edges: one row per lane, 64 lanes per block
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_bilinearity(pairing, n):
    shared.bilinearity(pairing, pr, n, seed=6000 + n)


# ---- 3. products of two and three pairs under one final exponentiation
@pytest.mark.parametrize("k", [2, 3])
def test_products(pairing, k):
    shared.products(pairing, pr, k, seed=60 + k)


# ---- 4. Groth16 on a key known in the exponent (tests/groth16_exp_key.py), two public inputs
@pytest.fixture(scope="module")
def exp_key():
    """the seven rows of the verification tests and the restatement's verdicts: two valid proofs, C + G, a changed input, -B,
    A at infinity, A off its curve"""
    K = ExpKey(pr, 66)
    rng = random.Random(67)
    s = [rng.randrange(1, r), rng.randrange(1, r)]
    rows = []
    for _ in range(2):
        a, b = rng.randrange(1, r), rng.randrange(1, 1 << 20)
        rows.append((K.g1(a), C2.mul(b, C2.G), K.g1(K.c_of(a, b, s)), list(s)))
    A, B, C, _ = rows[0]
    off = ((A[0][0],), ((A[1][0] + 1) % pr.p,))
    assert not C1.on_curve(off)
    rows += [(A, B, C1.add(C, C1.G), list(s)), (A, B, C, [s[0], (s[1] + 1) % r]), (A, C2.neg(B), C, list(s)), (None, B, C, list(s)),
             (off, B, C, list(s))]
    ref = []
    for A, B, C, x in rows:
        on = all(P is None or Cv.on_curve(P) for P, Cv in ((A, C1), (B, C2), (C, C1)))
        ref.append(2 if not on else int(pr.groth16_verify(K.vk, (A, B, C), x)))
    assert ref == [1, 1, 0, 0, 0, 0, 2]
    return {"key": K, "rows": rows, "expected": ref}


@pytest.mark.parametrize("tables", [None, "1", "0"])
def test_groth16_known_exponents(pairing, exp_key, tables, monkeypatch):
    """a fresh key for each setting of GH_GROTH16_TABLES (unset: both inputs by fixed-base tables; 1: the first by a table, the
    second by the variable-base kernels; 0: both by the variable-base kernels), read when a key is first used"""
    if tables is None:
        monkeypatch.delenv("GH_GROTH16_TABLES", raising=False)
    else:
        monkeypatch.setenv("GH_GROTH16_TABLES", tables)
    pvk = exp_key["key"].pvk(pairing)
    try:
        assert pvk.num_inputs == 2 and pvk.engine == ENGINE
        assert exp_key["key"].device_statuses(pvk, exp_key["rows"]) == exp_key["expected"]
        tm, _ = pairing.last_timing()
        assert all(tm[ph] > 0 for ph in ("g_ic", "miller", "final_exp"))
        with pytest.raises(pairing.GingerHipError):                             # MalformedVerifyingKey
            pvk.verify(g1_batch([C1.G]), g2_batch([C2.G]), g1_batch([C1.G]), np.zeros((1, 12), dtype=np.uint64))
    finally:
        pvk.close()


def test_groth16_batch_and_another_pairing_value(pairing, exp_key):
    """the seven rows in a seeded shuffle over three blocks; a key with another alpha_g1_beta_g2 rejects the valid rows"""
    order = [i % 7 for i in range(130)]
    random.Random(6130).shuffle(order)
    K = exp_key["key"]
    pvk = K.pvk(pairing)
    try:
        got = K.device_statuses(pvk, [exp_key["rows"][i] for i in order])
    finally:
        pvk.close()
    assert got == [exp_key["expected"][i] for i in order]
    gt = K.vk["alpha_g1_beta_g2"]
    other = K.pvk(pairing, gt=pr.mul(gt, gt))
    try:
        assert K.device_statuses(other, exp_key["rows"]) == [0, 0, 0, 0, 0, 0, 2]
    finally:
        other.close()


# ---- 5. one real proof: MNT6 parameters of the Benchmark circuit, the device prover, the device verifier
def test_groth16_real_proof(gpu, pairing):
    import groth16_ref as G
    groth16 = importlib.import_module("ginger_lib_amd.groth16")
    blob, info = G.generate_parameters(ENGINE, 13, seed=66)
    rows = groth16.benchmark_circuit_rows(ENGINE, 13)
    rng = pyref.Rng(6)
    rpk = groth16.ResidentProvingKey.from_parameters(gpu, ENGINE, blob, info["num_inputs"])
    try:
        proof = rpk.create_proof(rows, 0, 0, 0, rng.field_elem(r), rng.field_elem(r))
    finally:
        rpk.free()
    assert len(proof) == 193 + 577 + 193
    inputs = list(info["assignment"][1:info["num_inputs"]])
    key = info["key"]
    patched = pairing.parameters_with_pairing(blob, ENGINE)
    gt = pr.pairing(key["alpha_g1"], key["beta_g2"])
    assert patched[:576] == b"".join(v.to_bytes(96, "little") for v in pr.tower(gt)) and patched[576:] == blob[576:]
    pvk = pairing.PreparedVerifyingKey.from_parameters(patched, pairing=ENGINE)
    try:
        assert pvk.num_inputs == len(inputs) == 2
        assert [int(v) for v in pairing.verify_proofs(pvk, [proof], [inputs])] == [1]
        assert [int(v) for v in pairing.verify_proofs(pvk, [proof], [[inputs[0], (inputs[1] + 1) % r]])] == [0]
    finally:
        pvk.close()
    with pytest.raises(ValueError):                                              # the filler bytes of the unpatched stream are no Fq6 element
        pairing.PreparedVerifyingKey.from_parameters(blob, pairing=ENGINE)


# ---- 6. the chunks of launch_pairs after the first (tests/slab_chunks.py)
def test_pairing_product_in_three_slab_chunks(pairing, monkeypatch, capfd):
    shared.product_in_three_slab_chunks(pairing, pr, 1, 6261, monkeypatch, capfd)


@pytest.mark.parametrize("tables", [None, "1"])
def test_groth16_verify_in_three_slab_chunks(pairing, tables, monkeypatch, capfd):
    """261 proofs on the key known in the exponent, every point and every input of a row its own: a = a0 + i, b = b0 + 7 i,
    c = c0 + 3 i, s0 = i + 1 and s1 solved.  Every fifth row has its first input increased (status 0), one row has A at infinity
    and one A off its curve.  With GH_GROTH16_TABLES=1 the second input's part of g_ic goes through vb_single across the chunks."""
    import slab_chunks as K
    key = ExpKey(pr, 6262)
    rng = random.Random(6263)
    a0, b0, c0 = (rng.randrange(1 << 19, 1 << 20) for _ in range(3))
    A, B, C = C1.mul(a0, C1.G), C2.mul(b0, C2.G), C1.mul(c0, C1.G)
    G3, H2 = C1.mul(3, C1.G), C2.mul(7, C2.G)
    x2i, gi = pow(key.x[2], -1, r), pow(key.gamma, -1, r)
    rows, expected = [], []
    for i in range(K.N):
        g = ((a0 + i) * (b0 + 7 * i) - key.ab0 - (c0 + 3 * i) * key.delta) * gi % r
        s = [i + 1, (g - key.x[0] - (i + 1) * key.x[1]) * x2i % r]
        assert key.g_of(s) == g
        st = 1
        if i % 5 == 3:
            s[0], st = s[0] + K.N, 0                                             # another input: distinct from every row's
        rows.append((A, B, C, s))
        expected.append(st)
        A, B, C = C1.add(A, C1.G), C2.add(B, H2), C1.add(C, G3)
    K.assert_rows_differ([row[0] for row in rows], [row[1] for row in rows], [row[2] for row in rows], [row[3][0] for row in rows],
                         [row[3][1] for row in rows])
    rows[131] = (None,) + rows[131][1:]                                          # A at infinity: in the second chunk
    expected[131] = 0
    A = rows[257][0]
    rows[257] = (((A[0][0],), ((A[1][0] + 1) % pr.p,)),) + rows[257][1:]         # A off its curve: in the tail
    expected[257] = 2
    assert expected[128] == 0 and expected[256] == 1 and expected[260] == 1
    if tables is None:
        monkeypatch.delenv("GH_GROTH16_TABLES", raising=False)
    else:
        monkeypatch.setenv("GH_GROTH16_TABLES", tables)                          # read when a key is first used
    pvk = key.pvk(pairing)
    try:
        plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: key.device_statuses(pvk, rows))
    finally:
        pvk.close()
    assert K.chunk_lines(err, "launch_pairs_mnt6") == K.THREE, err
    assert K.chunk_lines(err, "vb_single") == (K.THREE if tables else []), err
    assert plain == cut
    assert cut == expected
    if tables is None:                                                           # the restatement's verdicts at the chunk edges, once
        for i in K.SAMPLE:
            A, B, C, s = rows[i]
            assert int(pr.groth16_verify(key.vk, (A, B, C), s)) == expected[i], i
