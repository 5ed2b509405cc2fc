"""Batched MNT4-753 pairings and Groth16 verification on the device (include/ginger_hip_pairing.h through
ginger-lib_amd/pairing.py) against the Python restatement tests/pairing_ref.py, which is pinned to the reference's known
answer by tests/test_pairing_host.py.  The tests that both engines share are tests/pairing_device_cases.py's.  Every
comparison is exact integer equality on the value after the final exponentiation; no row is skipped."""
import importlib
import random

import numpy as np
import pytest

import pairing_device_cases as shared
import pairing_ref
import pyref
from groth16_exp_key import ExpKey

pytestmark = pytest.mark.gpu
pr = pairing_ref.engine("mnt4753")
C1, C2, r = pr.C1, pr.C2, pr.r
g1_batch, g2_batch = pr.g1_batch, pr.g2_batch


@pytest.fixture(scope="module")
def pairing(gpu):
    return importlib.import_module("ginger_lib_amd.pairing")


# ---- 1. the reference's known answer (curves/mnt4753/tests.rs:266-467)
def test_known_answer(pairing):
    shared.known_answer(pairing, pr)


# ---- 2. bilinearity at wave and block edges: one row per lane, 64 lanes per block
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_bilinearity(pairing, n):
    shared.bilinearity(pairing, pr, n, seed=1000 + n)


# ---- 3. products of two and three pairs under one final exponentiation
@pytest.mark.parametrize("k", [2, 3])
def test_products(pairing, k):
    shared.products(pairing, pr, k, seed=k)


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
    other = pairing.PreparedVerifyingKey.from_parameters(pairing.gt_to_bytes(pr.gt_row(pr.mul(gt, gt))) + blob[384:])
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


def test_groth16_no_public_inputs(pairing):
    """n_abc = 1: a key from random scalars, so that a valid (A, B, C) is known in the exponent:
    a b = alpha beta + x gamma + c delta  with gamma_abc_g1 = [x G1]"""
    key = ExpKey(pr, 6, n_inputs=0)
    a, b = key.rng.randrange(1, r), key.rng.randrange(1, r)
    c = key.c_of(a, b, [])
    pvk = key.pvk(pairing)
    try:
        assert pvk.num_inputs == 0
        A, B, C = C1.mul(a, C1.G), C2.mul(b, C2.G), C1.mul(c, C1.G)
        cases = [((A, B, C), []), ((A, B, C1.add(C, C1.G)), []), ((C1.add(A, C1.G), B, C), []), ((A, C2.neg(B), C), [])]
        assert _verify(pairing, pvk, cases) == [1, 0, 0, 0]
    finally:
        pvk.close()


# ---- 8. the chunks of launch_pairs after the first (tests/slab_chunks.py)
@pytest.mark.parametrize("k", [1, 3])
def test_pairing_product_in_three_slab_chunks(pairing, k, monkeypatch, capfd):
    shared.product_in_three_slab_chunks(pairing, pr, k, 261 + k, monkeypatch, capfd)


@pytest.mark.parametrize("tables", [None, "1"])
def test_groth16_verify_in_three_slab_chunks(pairing, g16, tables, monkeypatch, capfd):
    """test_groth16_batch's seeded shuffle of the seven cases at 261 rows, so that the rows of status 2 and the skipped pairs fall
    into every chunk; with GH_GROTH16_TABLES=1 the second input's part of g_ic goes through vb_single across the chunks too"""
    import slab_chunks as K
    for seed in range(K.N, K.N + 100):                                           # the first shuffle that puts a skipped pair (case 5, A at
        order = [i % 7 for i in range(K.N)]                                      # infinity) and a row of status 2 (case 6) into every chunk,
        random.Random(seed).shuffle(order)                                       # the tail of 5 rows included
        if all({5, 6} <= set(order[lo:hi]) for lo, hi in ((0, 128), (128, 256), (256, K.N))):
            break
    else:
        raise AssertionError("no shuffle found")
    cases = [g16["cases"][i] for i in order]
    blob = pairing.parameters_with_pairing(g16["blob"])
    if tables is None:
        monkeypatch.delenv("GH_GROTH16_TABLES", raising=False)
    else:
        monkeypatch.setenv("GH_GROTH16_TABLES", tables)                          # read when a key is first used
    pvk = pairing.PreparedVerifyingKey.from_parameters(blob)
    try:
        plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: _verify(pairing, pvk, cases))
    finally:
        pvk.close()
    assert K.chunk_lines(err, "launch_pairs") == K.THREE, err
    assert K.chunk_lines(err, "vb_single") == (K.THREE if tables else []), err
    assert plain == cut
    assert cut == [g16["expected"][i] for i in order]


# ---- 9. g_ic and the proof points at their edges, on a key with known exponents
@pytest.fixture(scope="module")
def edge_key():
    """The shared key known in the exponent with three inputs (tests/groth16_exp_key.py).  The rows: every input row once with c
    solved (status 1) and once with one input increased by 1 (status 0), then the proof-point rows."""
    key = ExpKey(pr, 19, n_inputs=3)
    rng, x, g1, g_of, ab0, gamma, delta = key.rng, key.x, key.g1, key.g_of, key.ab0, key.gamma, key.delta
    inv = lambda v: pow(v, -1, r)
    rnd = lambda: rng.randrange(2, r - 1)
    s4, s5, s7 = [x[0] * inv(x[1]) % r, rnd(), rnd()], [-x[0] * inv(x[1]) % r, rnd(), rnd()], [rnd(), rnd(), 0]
    s7[2] = -(x[0] + s7[0] * x[1] + s7[1] * x[2]) * inv(x[3]) % r
    s_rows = [[0, 0, 0], [1, r - 1, 0], [r - 1, r - 1, r - 1],
              s4,                                                                # x0 G1 + s1 x1 G1: the first accumulation is a doubling
              s5,                                                                # ... passes through the point at infinity
              [rnd(), 0, rnd()],                                                 # a zero input between non-zero inputs
              s7]                                                                # g_ic ends at the point at infinity
    assert (x[0] + s4[0] * x[1]) % r == 2 * x[0] % r and (x[0] + s5[0] * x[1]) % r == 0 and g_of(s7) == 0
    rows, expected = [], []                                                      # (A, B, C, inputs)

    def proof(s, a=None, b=None, c=None):
        """a valid proof for the inputs s; of a, b, c at most two given, the third solved"""
        a = rng.randrange(1, 1 << 64) if a is None else a
        if c is None:
            b = rng.randrange(1, 1 << 20) if b is None else b
            c = key.c_of(a, b, s)
        elif b is None:
            b = (ab0 + g_of(s) * gamma + c * delta) * inv(a) % r
        return a, b, c

    for j, s in enumerate(s_rows):
        a, b, c = proof(s)
        A, B, C = g1(a), C2.mul(b, C2.G), g1(c)
        rows.append((A, B, C, list(s)))
        t = list(s)
        t[j % 3] = (t[j % 3] + 1) % r
        rows.append((A, B, C, t))
        expected += [1, 0]
    s = [rnd(), rnd(), rnd()]
    g = g_of(s)
    a, b, _ = proof(s, c=0)                                                      # C at infinity, b = (alpha beta + g gamma) / a
    rows.append((g1(a), C2.mul(b, C2.G), None, s))
    c = -(ab0 + g * gamma) * inv(delta) % r                                      # B at infinity: e(A, B) is one
    rows.append((g1(rng.randrange(1, r)), None, g1(c), s))
    a, b, c = proof(s)
    A, B, C = g1(a), C2.mul(b, C2.G), g1(c)
    B_off = (B[0], (B[1][0], (B[1][1] + 1) % pr.p))
    C_off = (C[0], ((C[1][0] + 1) % pr.p,))
    assert C2.on_curve(B) and not C2.on_curve(B_off) and C1.on_curve(C) and not C1.on_curve(C_off)
    rows += [(A, B_off, C, s), (A, B, C_off, s), (A, B, C, s)]                   # the last row: A's infinity byte is set below
    expected += [1, 1, 2, 2, 0]
    n = len(rows)
    a_xy, a_inf = pr.g1_batch([row[0] for row in rows])
    a_xy[n - 1] = np.array(pr.limbs(1) + pr.limbs(1), dtype=np.uint64)           # the point at infinity with coordinates (1, 1):
    a_inf[n - 1] = 1                                                             # on the curve, so evaluated as A = infinity
    return {"key": key, "rows": rows, "expected": expected, "a": (a_xy, a_inf), "b": pr.g2_batch([row[1] for row in rows]),
            "c": pr.g1_batch([row[2] for row in rows]), "inputs": pr.input_rows([row[3] for row in rows])}


@pytest.mark.parametrize("tables", [None, "0", "1"])
def test_groth16_g_ic_and_proof_point_edges(pairing, edge_key, tables, monkeypatch):
    """inputs 0, 1 and r - 1, an accumulation that doubles, one that passes through infinity and one that ends there; B and C
    off their curves, B, C and A at infinity.  A g_ic at infinity contributes one to the product: this pins the deviation that
    include/ginger_hip_pairing.h documents.  A fresh key for each setting of GH_GROTH16_TABLES (unset: every input by a
    fixed-base table; 0: every input by the variable-base kernels; 1: the first by a table, the others by variable base)."""
    K = edge_key
    if tables is None:
        monkeypatch.delenv("GH_GROTH16_TABLES", raising=False)
    else:
        monkeypatch.setenv("GH_GROTH16_TABLES", tables)
    pvk = K["key"].pvk(pairing)
    try:
        assert pvk.num_inputs == 3
        got = [int(v) for v in pvk.verify(K["a"], K["b"], K["c"], K["inputs"])]
        assert got == K["expected"]
        # the pooled buffers of the batch serve a shorter call on the same key
        first = pvk.verify(tuple(v[:5] for v in K["a"]), tuple(v[:5] for v in K["b"]), tuple(v[:5] for v in K["c"]), K["inputs"][:5])
        assert [int(v) for v in first] == K["expected"][:5]
    finally:
        pvk.close()


def test_groth16_edge_rows_against_the_restatement(edge_key):
    """two of the rows above through the restatement's groth16_verify: the valid proof whose g_ic is the point at infinity, and
    the rejected twin of the row whose accumulation doubles"""
    K = edge_key
    for i in (12, 7):
        A, B, C, s = K["rows"][i]
        assert int(pr.groth16_verify(K["key"].vk, (A, B, C), s)) == K["expected"][i], i
