"""Batched MNT6-753 pairings and Groth16 verification on the device (engine 2 of include/ginger_hip_pairing.h through
ginger-lib_amd/pairing.py) against the Python restatement tests/pairing6_ref.py, which is pinned to the reference's known
answer by tests/test_pairing6_host.py.  Every comparison is exact integer equality on the value after the final
exponentiation; no row is skipped."""
import importlib
import random

import numpy as np
import pytest

import pairing6_ref as pr
import pyref
from pairing6_ref import fq6_of, fq6_row, g1_batch, g2_batch

pytestmark = pytest.mark.gpu
ENGINE = "mnt6753"
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
    out = pairing.pairing_product(g1_batch([P for P, _ in flat]), g2_batch([Q for _, Q in flat]), k=k, engine=ENGINE)
    assert out.shape == (len(pairs_per_row), 72)
    return [fq6_of(row) for row in out]


# ---- 1. the reference's known answer (curves/mnt6753/tests.rs:319-590)
def test_known_answer(pairing):
    P, Q, want = pr.kat()
    out = pairing.pairing_product(g1_batch([P]), g2_batch([Q]), engine=ENGINE)
    assert [int(v) for v in out[0]] == [int(v) for v in fq6_row(want)]           # all six Fq words, in the order of Fp6::write
    assert pairing.gt_to_bytes(out[0], ENGINE) == b"".join(v.to_bytes(96, "little") for v in pr.tower(want))
    tm, total = pairing.last_timing()
    assert tm["miller"] > 0 and tm["final_exp"] > 0 and tm["g_ic"] == 0 and total > 0


# ---- 2. bilinearity at wave and block edges: one row per lane, 64 lanes per block
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_bilinearity(pairing, e0, n):
    rng = random.Random(6000 + n)
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
    rng = random.Random(60 + k)
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


# ---- 4. Groth16 on a key known in the exponent, two public inputs
class ExpKey:
    """gamma_abc_g1 = [x0 G1, x1 G1, x2 G1], alpha_g1_beta_g2 = e0^(alpha beta), gamma_g2 = gamma G2, delta_g2 = delta G2: for
    inputs s, g_ic = g G1 with g = x0 + s0 x1 + s1 x2, and (a G1, b G2, c G1) is valid iff a b = alpha beta + g gamma + c delta"""

    def __init__(self, e0, seed):
        import schnorr_ref
        rng = random.Random(seed)
        self.g1 = lambda k: schnorr_ref.mul(C1, k % r, C1.G) if k % r else None
        self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(1, r) for _ in range(4))
        self.x = [rng.randrange(1, r) for _ in range(3)]
        self.ab0 = self.alpha * self.beta % r
        self.vk = {"alpha_g1_beta_g2": pr.fpow(e0, self.ab0), "gamma_g2": C2.mul(self.gamma, C2.G), "delta_g2": C2.mul(self.delta, C2.G),
                   "gamma_abc_g1": [self.g1(v) for v in self.x]}

    def g_of(self, s):
        return (self.x[0] + s[0] * self.x[1] + s[1] * self.x[2]) % r

    def c_of(self, a, b, s):
        return (a * b - self.ab0 - self.g_of(s) * self.gamma) * pow(self.delta, -1, r) % r

    def pvk(self, pairing, gt=None):
        vk = self.vk
        return pairing.PreparedVerifyingKey(fq6_row(gt if gt is not None else vk["alpha_g1_beta_g2"]), pr.g2_row(vk["gamma_g2"]),
                                            pr.g2_row(vk["delta_g2"]), np.stack([pr.g1_row(P) for P in vk["gamma_abc_g1"]]), engine=ENGINE)


def _verify_rows(pvk, rows):
    """rows: (A, B, C, inputs) with pyref points -> the device's statuses"""
    n = len(rows)
    x = np.array([[pyref.int_to_limbs(pyref.P4.to_mont(v)) for v in row[3]] for row in rows], dtype=np.uint64).reshape(n, -1, 12)
    a_xy, a_inf = g1_batch([row[0] for row in rows])
    for i, row in enumerate(rows):
        if row[0] is not None and not C1.on_curve(row[0]):
            assert a_inf[i] == 0
    return [int(v) for v in pvk.verify((a_xy, a_inf), g2_batch([row[1] for row in rows]), g1_batch([row[2] for row in rows]), x)]


@pytest.fixture(scope="module")
def exp_key(e0):
    """the seven rows of the verification tests and the restatement's verdicts: two valid proofs, C + G, a changed input, -B,
    A at infinity, A off its curve"""
    assert pyref.P4.p == r
    K = ExpKey(e0, 66)
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
        assert _verify_rows(pvk, exp_key["rows"]) == exp_key["expected"]
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
        got = _verify_rows(pvk, [exp_key["rows"][i] for i in order])
    finally:
        pvk.close()
    assert got == [exp_key["expected"][i] for i in order]
    gt = K.vk["alpha_g1_beta_g2"]
    other = K.pvk(pairing, gt=pr.mul(gt, gt))
    try:
        assert _verify_rows(other, exp_key["rows"]) == [0, 0, 0, 0, 0, 0, 2]
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
def test_pairing_product_in_three_slab_chunks(pairing, e0, monkeypatch, capfd):
    """gh_pairing_product of 261 rows in chunks of 128, 128 and 5 rows: row i is ((a0 + i) G1, (b0 + 7 i) G2), so no two rows
    share a point; every row against e0^(a b), the rows of SAMPLE against the restatement's own pairing"""
    import slab_chunks as K
    rng = random.Random(6261)
    a0, b0 = rng.randrange(1 << 19, 1 << 20), rng.randrange(1 << 19, 1 << 20)
    P, Q, H2 = C1.mul(a0, C1.G), C2.mul(b0, C2.G), C2.mul(7, C2.G)
    ps, qs = [], []
    for _ in range(K.N):
        ps.append(P)
        qs.append(Q)
        P, Q = C1.add(P, C1.G), C2.add(Q, H2)
    K.assert_rows_differ(ps, qs)
    assert ps[K.N - 1] == C1.mul(a0 + K.N - 1, C1.G) and qs[K.N - 1] == C2.mul(b0 + 7 * (K.N - 1), C2.G)
    ab = [(a0 + i, b0 + 7 * i) for i in range(K.N)]
    ps[131] = None                                                               # P at infinity: in the second chunk only
    ab[131] = (0, 0)
    qs[258] = None                                                               # Q at infinity: in the tail only
    ab[258] = (0, 0)
    g1, g2 = g1_batch(ps), g2_batch(qs)
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: pairing.pairing_product(g1, g2, engine=ENGINE))
    assert K.chunk_lines(err, "launch_pairs_mnt6") == K.THREE, err
    assert K.chunk_lines(err, "launch_pairs") == [], err                         # MNT4's launches keep their own name
    assert K.identical(plain, cut)
    exp = [pr.fpow(e0, a * b % r) for a, b in ab]
    assert exp[131] == exp[258] == pr.ONE
    bad = [i for i in range(K.N) if fq6_of(cut[i]) != exp[i]]
    assert not bad, bad
    for i in K.SAMPLE:
        assert fq6_of(cut[i]) == pr.pairing(ps[i], qs[i]), i


@pytest.mark.parametrize("tables", [None, "1"])
def test_groth16_verify_in_three_slab_chunks(pairing, e0, tables, monkeypatch, capfd):
    """261 proofs on the key known in the exponent, every point and every input of a row its own: a = a0 + i, b = b0 + 7 i,
    c = c0 + 3 i, s0 = i + 1 and s1 solved.  Every fifth row has its first input increased (status 0), one row has A at infinity
    and one A off its curve.  With GH_GROTH16_TABLES=1 the second input's part of g_ic goes through vb_single across the chunks."""
    import slab_chunks as K
    key = ExpKey(e0, 6262)
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
        plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: _verify_rows(pvk, rows))
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
