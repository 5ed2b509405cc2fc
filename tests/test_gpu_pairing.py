"""Batched MNT4-753 pairings and Groth16 verification on the device (include/ginger_hip_pairing.h through
ginger-lib_amd/pairing.py) against the Python restatement tests/pairing_ref.py, which is pinned to the reference's known
answer by tests/test_pairing_host.py.  Every comparison is exact integer equality on the value after the final
exponentiation; no row is skipped."""
import importlib
import random

import numpy as np
import pytest

import pairing_ref as pr
import pyref
from pairing_ref import fq4_of, fq4_row, g1_batch, g2_batch

pytestmark = pytest.mark.gpu
C1, C2 = pr.C1, pr.C2
r = pr.r


@pytest.fixture(scope="module")
def pairing(gpu):
    return importlib.import_module("ginger_lib_amd.pairing")


@pytest.fixture(scope="module")
def e0():
    """e(G1, G2): the one Python pairing the bilinearity tests share"""
    return pr.pairing(C1.G, C2.G)


def device_product(pairing, pairs_per_row):
    k = len(pairs_per_row[0])
    flat = [pq for row in pairs_per_row for pq in row]
    out = pairing.pairing_product(g1_batch([P for P, _ in flat]), g2_batch([Q for _, Q in flat]), k=k)
    return [fq4_of(row) for row in out]


# ---- 1. the reference's known answer (curves/mnt4753/tests.rs:266-467)
def test_known_answer(pairing):
    P, Q, want = pr.kat()
    out = pairing.pairing_product(g1_batch([P]), g2_batch([Q]))
    assert [int(v) for v in out[0]] == [int(v) for v in fq4_row(want)]           # all four Fq words, in the order of Fp4::write
    assert pairing.gt_to_bytes(out[0]) == b"".join(v.to_bytes(96, "little") for v in pr.tower(want))
    tm, total = pairing.last_timing()
    assert tm["miller"] > 0 and tm["final_exp"] > 0 and tm["g_ic"] == 0 and total > 0


# ---- 2. bilinearity at wave and block edges: one row per lane, 64 lanes per block
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_bilinearity(pairing, e0, n):
    rng = random.Random(1000 + n)
    ab = [(rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 20)) for _ in range(n)]
    rows = [[(C1.mul(a, C1.G), C2.mul(b, C2.G))] for a, b in ab]
    exp = [pr.fpow(e0, a * b) for a, b in ab]
    if n >= 3:
        rows[n // 2][0] = (None, rows[n // 2][0][1])                             # P at infinity
        exp[n // 2] = pr.ONE
        rows[n - 1][0] = (rows[n - 1][0][0], None)                               # Q at infinity, in the last lane
        exp[n - 1] = pr.ONE
    b0 = ab[0][1]
    rows[0][0] = (C1.mul(r - 1, C1.G), rows[0][0][1])                            # a = r - 1: e0^(-b)
    exp[0] = pr.inv(pr.fpow(e0, b0))
    got = device_product(pairing, rows)
    assert len(got) == n
    bad = [i for i in range(n) if got[i] != exp[i]]
    assert not bad, bad


# ---- 3. products of two and three pairs under one final exponentiation
@pytest.mark.parametrize("k", [2, 3])
def test_products(pairing, k):
    rng = random.Random(k)
    pt1 = lambda: C1.mul(rng.randrange(1, 1 << 20), C1.G)
    pt2 = lambda: C2.mul(rng.randrange(1, 1 << 20), C2.G)
    rows = [[(pt1(), pt2()) for _ in range(k)] for _ in range(5)]
    P, Q = rows[0][0]
    rows[1] = [(P, Q), (C1.neg(P), Q)] + [(None, pt2())] * (k - 2)               # the product is one
    rows[2][k - 1] = (pt1(), None)                                               # one pair drops out
    if k == 3:
        rows[3] = [(C1.mul(2, C1.G), C2.mul(3, C2.G)), (C1.mul(5, C1.G), C2.G), (C1.mul(r - 11, C1.G), C2.G)]   # 6 + 5 - 11 = 0
    exp = [pr.product(row) for row in rows]
    assert exp[1] == pr.ONE and (k == 2 or exp[3] == pr.ONE)
    got = device_product(pairing, rows)
    assert got == exp


# ---- 4. - 7. Groth16
@pytest.fixture(scope="module")
def g16(gpu, pairing):
    """MNT4 parameters of the Benchmark circuit at 13 constraints (tests/groth16_ref.py), two proofs of the device prover with
    different (r, s), and the seven rows of the verification tests with the restatement's verdicts"""
    import groth16_ref as G
    groth16 = importlib.import_module("ginger_lib_amd.groth16")
    blob, info = G.generate_parameters("mnt4753", 13, seed=16)
    key = info["key"]
    rows = groth16.benchmark_circuit_rows("mnt4753", 13)
    rng = pyref.Rng(5)
    rpk = groth16.ResidentProvingKey.from_parameters(gpu, "mnt4753", blob, info["num_inputs"])
    try:
        proofs = [rpk.create_proof(rows, 0, 0, 0, rng.field_elem(r), rng.field_elem(r)) for _ in range(2)]   # d1 = d2 = d3 = 0, as create_random_proof passes them (prover.rs:192-198)
    finally:
        rpk.free()
    assert proofs[0] != proofs[1]
    inputs = list(info["assignment"][1:info["num_inputs"]])
    assert len(inputs) == 2

    def parse(proof):
        pt = lambda C, b: None if b[-1] else tuple(tuple(int.from_bytes(b[96 * (C.deg * c + d):96 * (C.deg * c + d) + 96], "little")
                                                        for d in range(C.deg)) for c in range(2))
        return pt(C1, proof[:193]), pt(C2, proof[193:578]), pt(C1, proof[578:])
    (A1, B1, Cc1), (A2, B2, Cc2) = parse(proofs[0]), parse(proofs[1])
    off = ((A1[0][0],), ((A1[1][0] + 1) % pr.p,))
    assert not C1.on_curve(off)
    cases = [((A1, B1, Cc1), inputs), ((A2, B2, Cc2), inputs), ((C1.neg(A1), C2.neg(B1), Cc1), inputs),
             ((A1, B1, C1.add(Cc1, C1.G)), inputs), ((A1, B1, Cc1), [inputs[0], (inputs[1] + 1) % r]), ((None, B1, Cc1), inputs),
             ((off, B1, Cc1), inputs)]
    return {"blob": blob, "key": key, "cases": cases, "expected": [1, 1, 1, 0, 0, 0, 2]}


def _verify(pairing, pvk, cases):
    G = importlib.import_module("groth16_ref")
    proofs = [G.wire(C1, A) + G.wire(C2, B) + G.wire(C1, C) for (A, B, C), _ in cases]
    return [int(s) for s in pairing.verify_proofs(pvk, proofs, [x for _, x in cases])]


def test_groth16_end_to_end(pairing, g16):
    key = g16["key"]
    # alpha_g1_beta_g2 by the device pairing, spliced into the stream: equal to the restatement's value
    blob = pairing.parameters_with_pairing(g16["blob"])
    gt = pr.pairing(key["alpha_g1"], key["beta_g2"])
    assert blob[:384] == b"".join(v.to_bytes(96, "little") for v in pr.tower(gt)) and blob[384:] == g16["blob"][384:]
    vk = {"alpha_g1_beta_g2": gt, "gamma_g2": key["gamma_g2"], "delta_g2": key["delta_g2"], "gamma_abc_g1": key["gamma_abc_g1"]}
    ref = []
    for (A, B, C), x in g16["cases"]:
        on = all(P is None or Cv.on_curve(P) for P, Cv in ((A, C1), (B, C2), (C, C1)))
        ref.append(2 if not on else int(pr.groth16_verify(vk, (A, B, C), x)))
    assert ref == g16["expected"]
    pvk = pairing.PreparedVerifyingKey.from_parameters(blob)
    try:
        assert pvk.num_inputs == 2
        assert _verify(pairing, pvk, g16["cases"]) == ref
        tm, _ = pairing.last_timing()
        assert all(tm[ph] > 0 for ph in ("g_ic", "miller", "final_exp"))
        assert _verify(pairing, pvk, g16["cases"][:1]) == [1]                    # the tables are built once and stay
        with pytest.raises(pairing.GingerHipError):                             # MalformedVerifyingKey
            pvk.verify(g1_batch([C1.G]), g2_batch([C2.G]), g1_batch([C1.G]), np.zeros((1, 12), dtype=np.uint64))
    finally:
        pvk.close()
    with pytest.raises(ValueError):                                              # the filler bytes of the unpatched stream are no Fq4 element
        pairing.PreparedVerifyingKey.from_parameters(g16["blob"])
    # a key with another pairing value rejects the valid proofs
    other = pairing.PreparedVerifyingKey.from_parameters(pairing.gt_to_bytes(fq4_row(pr.mul(gt, gt))) + blob[384:])
    try:
        assert _verify(pairing, other, g16["cases"]) == [0, 0, 0, 0, 0, 0, 2]
    finally:
        other.close()


def test_groth16_batch(pairing, g16):
    """the same rows in a seeded shuffle over three blocks: statuses are known by construction"""
    order = [i % 7 for i in range(130)]
    random.Random(130).shuffle(order)
    pvk = pairing.PreparedVerifyingKey.from_parameters(pairing.parameters_with_pairing(g16["blob"]))
    try:
        got = _verify(pairing, pvk, [g16["cases"][i] for i in order])
    finally:
        pvk.close()
    assert got == [g16["expected"][i] for i in order]


def test_groth16_variable_base_inputs(pairing, g16, monkeypatch):
    """g_ic through the variable-base kernels (the path of a key with more inputs than fixed-base tables fit): GH_GROTH16_TABLES
    is read when a key is first used"""
    monkeypatch.setenv("GH_GROTH16_TABLES", "1")                                 # one input by table, one by variable base
    pvk = pairing.PreparedVerifyingKey.from_parameters(pairing.parameters_with_pairing(g16["blob"]))
    try:
        assert _verify(pairing, pvk, g16["cases"]) == g16["expected"]
    finally:
        pvk.close()


def test_groth16_no_public_inputs(pairing, e0):
    """n_abc = 1: a key from random scalars, so that a valid (A, B, C) is known in the exponent:
    a b = alpha beta + x gamma + c delta  with gamma_abc_g1 = [x G1]"""
    rng = random.Random(6)
    alpha, beta, gamma, delta, x, a, b = (rng.randrange(1, r) for _ in range(7))
    c = (a * b - alpha * beta - x * gamma) * pow(delta, -1, r) % r
    gt = pr.fpow(e0, alpha * beta % r)
    pvk = pairing.PreparedVerifyingKey(fq4_row(gt), pr.g2_row(C2.mul(gamma, C2.G)), pr.g2_row(C2.mul(delta, C2.G)),
                                       pr.g1_row(C1.mul(x, C1.G)))
    try:
        assert pvk.num_inputs == 0
        A, B, C = C1.mul(a, C1.G), C2.mul(b, C2.G), C1.mul(c, C1.G)
        cases = [((A, B, C), []), ((A, B, C1.add(C, C1.G)), []), ((C1.add(A, C1.G), B, C), []), ((A, C2.neg(B), C), [])]
        assert _verify(pairing, pvk, cases) == [1, 0, 0, 0]
    finally:
        pvk.close()
