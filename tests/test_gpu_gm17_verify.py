"""Batched GM17 verification on the device (include/ginger_hip_gm17.h through ginger-lib_amd/gm17_verify.py), both engines,
against the closed form of a key known in the exponent (tests/gm17_verify_ref.py, whose restatement of verifier.rs is pinned to
that closed form by tests/test_gm17_verify_host.py), and one real proof made by the device prover.  Statuses are compared
exactly; no row is skipped."""
import importlib
import random

import numpy as np
import pytest

import gm17_verify_ref as R
import pairing_ref
import pyref

pytestmark = pytest.mark.gpu
LOOP = {"mnt4753": "launch_pairs", "mnt6753": "launch_pairs_mnt6"}


@pytest.fixture(scope="module")
def gv(gpu):
    return importlib.import_module("ginger_lib_amd.gm17_verify")


@pytest.fixture(scope="module", params=pairing_ref.ENGINES)
def engine(request):
    return request.param


@pytest.fixture(scope="module")
def pr(engine):
    return pairing_ref.engine(engine)


@pytest.fixture(scope="module")
def edge(pr):
    key = R.ExpKey(pr, 1711)
    rows, expected, _ = R.edge_rows(key)
    return {"key": key, "rows": rows, "expected": expected}


# ---- 1. the edge rows on a fresh key, for every setting of GH_GROTH16_TABLES
@pytest.mark.parametrize("tables", [None, "1", "0"])
def test_edge_rows(gv, pr, engine, edge, tables, monkeypatch):
    """unset: both inputs of g_psi by fixed-base tables; 1: the second by the variable-base kernels; 0: both (the knob is read
    when a key is first used)"""
    if tables is None:
        monkeypatch.delenv("GH_GROTH16_TABLES", raising=False)
    else:
        monkeypatch.setenv("GH_GROTH16_TABLES", tables)
    pvk = R.pvk_of(gv, edge["key"])
    try:
        assert pvk.num_inputs == 2 and pvk.engine == engine
        got = R.device_statuses(pr, pvk, edge["rows"])
        print(engine, tables, got)
        assert got == edge["expected"]
        tm, total = gv.last_timing()
        assert all(tm[ph] > 0 for ph in ("test1_miller", "test1_final_exp", "test2_miller", "test2_final_exp")) and total > 0
        with pytest.raises(gv.GingerHipError):                                  # one input too few: MalformedVerifyingKey
            pvk.verify(pr.g1_batch([pr.C1.G]), pr.g2_batch([pr.C2.G]), pr.g1_batch([pr.C1.G]), np.zeros((1, 1, 12), dtype=np.uint64))
    finally:
        pvk.close()


# ---- 2. three blocks, and a key with another h_beta
def test_batch_and_another_h_beta(gv, pr, edge):
    """the edge rows in a seeded shuffle over 130 rows (64 rows per block); a key with h_beta + H rejects every row that was
    valid but one, by the closed form: with A and B at infinity the sums are g_alpha and h_beta themselves, and
    e(-g_alpha, h_beta) e(g_alpha, h_beta) = 1 whatever h_beta is"""
    m = len(edge["rows"])
    order = [i % m for i in range(130)]
    random.Random(1730).shuffle(order)
    key = edge["key"]
    pvk = R.pvk_of(gv, key)
    try:
        got = R.device_statuses(pr, pvk, [edge["rows"][i] for i in order])
    finally:
        pvk.close()
    assert got == [edge["expected"][i] for i in order]
    other = R.ExpKey(pr, 1711, beta=(key.beta + 1) % key.r)
    assert other.vk["h_beta_g2"] != key.vk["h_beta_g2"] and other.vk["query"] == key.vk["query"] and other.alpha == key.alpha
    opvk = R.pvk_of(gv, other)
    try:
        got = R.device_statuses(pr, opvk, edge["rows"])
    finally:
        opvk.close()
    print(got)
    exps = R.edge_exponents(key)
    want = [other.status(*e) for e in exps] + [2, 2]
    assert got == want
    was_valid = [i for i, e in enumerate(edge["expected"]) if e == 1]
    assert len(was_valid) == 8 and [i for i in was_valid if want[i] == 1] == [10] and exps[10][:2] == (0, 0)


# ---- 3. the chunks of both launch_pairs calls after the first (tests/slab_chunks.py)
def test_verify_in_three_slab_chunks(gv, pr, engine, monkeypatch, capfd):
    """261 proofs, every point and every input of a row its own: a_i = b_i = a0 + i, s0 = i + 1, c_i = c0 + 3 i and s1 solved.
    Every fifth row has its first input changed (status 0 by test1), every seventh has b_i shifted and c_i solved again (status 0
    by test2 only); one row has A at infinity in the second chunk, one has A off its curve in the tail."""
    import slab_chunks as K
    key = R.ExpKey(pr, 1761)
    C1, C2 = pr.C1, pr.C2
    rng = random.Random(1762)
    a0, c0 = (rng.randrange(1 << 19, 1 << 20) for _ in range(2))
    A, B, C = C1.mul(a0, C1.G), C2.mul(a0, C2.G), C1.mul(c0, C1.G)
    G3, H9 = C1.mul(3, C1.G), C2.mul(1 << 30, C2.G)
    rows, expected = [], []
    for i in range(K.N):
        a = b = a0 + i
        c = c0 + 3 * i
        Bi, Ci = B, C
        s = [i + 1, key.s1_of(a, b, c, i + 1)]
        if i % 7 == 2:
            b, Bi = b + (1 << 30), C2.add(B, H9)                                 # test2 fails; c is solved for this b: test1 holds
            c = key.c_of(a, b, s)
            Ci = C1.mul(c, C1.G)
        if i % 5 == 3:
            s[0] += K.N                                                          # another input: distinct from every row's
        rows.append((A, Bi, Ci, s))
        expected.append(key.status(a, b, c, s))
        assert expected[-1] == int(i % 7 != 2 and i % 5 != 3)
        if i % 7 == 2 and i % 5 != 3:
            assert key.tests(a, b, c, s) == (True, False)
        A, B, C = C1.add(A, C1.G), C2.add(B, C2.G), C1.add(C, G3)
    K.assert_rows_differ([row[0] for row in rows], [row[1] for row in rows], [row[2] for row in rows], [row[3][0] for row in rows],
                         [row[3][1] for row in rows])
    assert rows[K.N - 1][0] == C1.mul(a0 + K.N - 1, C1.G) and rows[K.N - 1][2] == C1.mul(c0 + 3 * (K.N - 1), C1.G)
    _, Bq, Cq, sq = rows[131]
    rows[131] = (None, Bq, Cq, sq)                                               # A at infinity: in the second chunk
    expected[131] = key.status(0, a0 + 131, c0 + 3 * 131, sq)
    assert expected[131] == 0
    Aq = rows[257][0]
    rows[257] = (((Aq[0][0],), ((Aq[1][0] + 1) % pr.p,)),) + rows[257][1:]       # A off its curve: in the tail
    expected[257] = 2
    assert expected[128] == 0 and expected[129] == 1 and expected[256] == 1 and expected[260] == 1
    monkeypatch.delenv("GH_GROTH16_TABLES", raising=False)
    pvk = R.pvk_of(gv, key)
    try:
        plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: R.device_statuses(pr, pvk, rows))
    finally:
        pvk.close()
    assert K.chunk_lines(err, LOOP[engine]) == K.THREE * 2, err                  # test1 and test2
    other = [v for k, v in LOOP.items() if k != engine][0]
    assert K.chunk_lines(err, other) == [], err                                  # the other engine's launches keep their own name
    assert plain == cut
    assert cut == expected


# ---- 4. one real proof: parameters of the Benchmark circuit generated on the device, the device prover, the device verifier
@pytest.mark.parametrize("pairing", ["mnt4753", "mnt6753"])
def test_real_proof(gpu, gv, pairing):
    import support as S
    gm17 = importlib.import_module("ginger_lib_amd.gm17")
    groth16 = importlib.import_module("ginger_lib_amd.groth16")
    C1, C2 = pyref.CURVES[pairing + "_g1"], pyref.CURVES[pairing + "_g2"]
    r = C1.order
    n_con = 13
    rng = pyref.Rng(1717)
    alpha, beta, t, r_, d1, d2 = (rng.field_elem(r) for _ in range(6))
    gamma = 1                                                                    # generate_random_parameters (generator.rs:27): the
    assert r_ and d1 and d2                                                      # generator's C queries fit the verifier for gamma = 1 only
    g1, g2 = C1.mul(rng.next_u64() | 1, C1.G), C2.mul(rng.next_u64() | 1, C2.G)
    g1_xyz, g2_xyz = S.proj_array(C1, g1), S.proj_array(C2, g2)
    pk, info = gm17.generate_parameters(gpu, pairing, groth16.benchmark_circuit_lcs(n_con), alpha, beta, gamma, t, g1_xyz, g2_xyz)
    vk = gm17.verifying_key(gpu, pairing, pk, alpha, beta, gamma, g1_xyz, g2_xyz)
    rows = groth16.benchmark_circuit_rows(pairing, n_con)
    ni = rows[0]
    assert ni == info["num_inputs"] == 3 and vk["query"].shape == (ni, 24)
    key = gm17.ResidentGm17Key(gpu, pairing, pk, ni)
    try:
        proof = key.create_proof(rows, d1, d2, r_)
    finally:
        key.free()
        gpu.dev_trim()
    blob = gm17.proof_bytes(pairing, proof)
    inputs = [int(v) for v in rows[1][1:ni]]
    pvk = gv.PreparedVerifyingKey.from_key(vk)
    try:
        assert pvk.num_inputs == len(inputs) == 2 and pvk.engine == pairing
        assert [int(v) for v in gv.verify_proofs(pvk, [blob], [inputs])] == [1]
        assert [int(v) for v in gv.verify_proofs(pvk, [blob], [[inputs[0], (inputs[1] + 1) % r]])] == [0]
        g1_rec = 193
        swapped = blob[-g1_rec:] + blob[g1_rec:-g1_rec] + blob[:g1_rec]          # A and C swapped
        assert swapped != blob and len(swapped) == len(blob)
        assert [int(v) for v in gv.verify_proofs(pvk, [swapped], [inputs])] == [0]
    finally:
        pvk.close()
