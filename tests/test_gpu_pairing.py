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


# ---- 8. the chunks of launch_pairs after the first (tests/slab_chunks.py)
@pytest.mark.parametrize("k", [1, 3])
def test_pairing_product_in_three_slab_chunks(pairing, e0, k, monkeypatch, capfd):
    """gh_pairing_product of 261 rows in chunks of 128, 128 and 5 rows: pair t = i k + j of row i is ((a0 + t) G1, (b0 + 7 t) G2),
    so no two rows share a point, and the row's value is e0^(sum_j a b): every row against the restatement, not a sample"""
    import slab_chunks as K
    rng = random.Random(261 + k)
    a0, b0 = rng.randrange(1 << 19, 1 << 20), rng.randrange(1 << 19, 1 << 20)
    m = K.N * k
    P, Q, H2 = C1.mul(a0, C1.G), C2.mul(b0, C2.G), C2.mul(7, C2.G)
    ps, qs = [], []
    for _ in range(m):
        ps.append(P)
        qs.append(Q)
        P, Q = C1.add(P, C1.G), C2.add(Q, H2)
    assert len(set(ps)) == m and len(set(qs)) == m
    assert ps[m - 1] == C1.mul(a0 + m - 1, C1.G) and qs[m - 1] == C2.mul(b0 + 7 * (m - 1), C2.G)
    ab = [[(a0 + i * k + j, b0 + 7 * (i * k + j)) for j in range(k)] for i in range(K.N)]
    ps[131 * k] = None                                                           # P at infinity: in the second chunk only
    ab[131][0] = (0, 0)
    qs[258 * k + k - 1] = None                                                   # Q at infinity: in the tail only
    ab[258][k - 1] = (0, 0)
    g1, g2 = g1_batch(ps), g2_batch(qs)
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: pairing.pairing_product(g1, g2, k=k))
    assert K.chunk_lines(err, "launch_pairs") == K.THREE, err
    assert K.identical(plain, cut)
    exp = [pr.fpow(e0, sum(a * b for a, b in row) % r) for row in ab]
    if k == 1:
        assert exp[131] == exp[258] == pr.ONE
    bad = [i for i in range(K.N) if fq4_of(cut[i]) != exp[i]]
    assert not bad, bad


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
def edge_key(e0):
    """gamma_abc_g1 = [x0 G1 .. x3 G1], alpha_g1_beta_g2 = e0^(alpha beta), gamma_g2 = gamma G2, delta_g2 = delta G2: for
    inputs s, g_ic = g G1 with g = x0 + s1 x1 + s2 x2 + s3 x3, and (a G1, b G2, c G1) is valid iff a b = alpha beta + g gamma + c delta.
    The rows: every input row once with c solved (status 1) and once with one input increased by 1 (status 0), then the
    proof-point rows."""
    import schnorr_ref
    assert pyref.P6.p == r
    rng = random.Random(19)
    g1 = lambda k: schnorr_ref.mul(C1, k % r, C1.G)
    inv = lambda v: pow(v, -1, r)
    alpha, beta, gamma, delta = (rng.randrange(1, r) for _ in range(4))
    x = [rng.randrange(1, r) for _ in range(4)]
    ab0 = alpha * beta % r
    g_of = lambda s: (x[0] + sum(si * xi for si, xi in zip(s, x[1:]))) % r
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
        g = g_of(s)
        a = rng.randrange(1, 1 << 64) if a is None else a
        if c is None:
            b = rng.randrange(1, 1 << 20) if b is None else b
            c = (a * b - ab0 - g * gamma) * inv(delta) % r
        elif b is None:
            b = (ab0 + g * gamma + c * delta) * inv(a) % r
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
    a_xy, a_inf = g1_batch([row[0] for row in rows])
    a_xy[n - 1] = np.array(pr.limbs(1) + pr.limbs(1), dtype=np.uint64)           # the point at infinity with coordinates (1, 1):
    a_inf[n - 1] = 1                                                             # on the curve, so evaluated as A = infinity
    inputs = np.array([[pyref.int_to_limbs(pyref.P6.to_mont(v)) for v in row[3]] for row in rows], dtype=np.uint64).reshape(n, 3, 12)
    vk = {"alpha_g1_beta_g2": pr.fpow(e0, ab0), "gamma_g2": C2.mul(gamma, C2.G), "delta_g2": C2.mul(delta, C2.G),
          "gamma_abc_g1": [g1(v) for v in x]}
    return {"vk": vk, "rows": rows, "expected": expected, "a": (a_xy, a_inf), "b": g2_batch([row[1] for row in rows]),
            "c": g1_batch([row[2] for row in rows]), "inputs": inputs}


@pytest.mark.parametrize("tables", [None, "0", "1"])
def test_groth16_g_ic_and_proof_point_edges(pairing, edge_key, tables, monkeypatch):
    """inputs 0, 1 and r - 1, an accumulation that doubles, one that passes through infinity and one that ends there; B and C
    off their curves, B, C and A at infinity.  A g_ic at infinity contributes one to the product: this pins the deviation that
    include/ginger_hip_pairing.h documents.  A fresh key for each setting of GH_GROTH16_TABLES (unset: every input by a
    fixed-base table; 0: every input by the variable-base kernels; 1: the first by a table, the others by variable base)."""
    K = edge_key
    vk = K["vk"]
    if tables is None:
        monkeypatch.delenv("GH_GROTH16_TABLES", raising=False)
    else:
        monkeypatch.setenv("GH_GROTH16_TABLES", tables)
    pvk = pairing.PreparedVerifyingKey(fq4_row(vk["alpha_g1_beta_g2"]), pr.g2_row(vk["gamma_g2"]), pr.g2_row(vk["delta_g2"]),
                                       np.stack([pr.g1_row(P) for P in vk["gamma_abc_g1"]]))
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
    """two of the rows above through pairing_ref.groth16_verify: the valid proof whose g_ic is the point at infinity, and the
    rejected twin of the row whose accumulation doubles"""
    K = edge_key
    for i in (12, 7):
        A, B, C, s = K["rows"][i]
        assert int(pr.groth16_verify(K["vk"], (A, B, C), s)) == K["expected"][i], i
