"""The device tests that MNT4-753 and MNT6-753 share, written once over an engine object `pr` of tests/pairing_ref.py and a seed:
tests/test_gpu_pairing.py and tests/test_gpu_pairing6.py call them with their own engine, cases and seeds.  Every comparison is
exact integer equality on the value after the final exponentiation; no row is skipped.  Test infrastructure."""
import random

LOOP = {"mnt4753": "launch_pairs", "mnt6753": "launch_pairs_mnt6"}


def device_product(pairing, pr, pairs_per_row):
    k = len(pairs_per_row[0])
    flat = [pq for row in pairs_per_row for pq in row]
    out = pairing.pairing_product(pr.g1_batch([P for P, _ in flat]), pr.g2_batch([Q for _, Q in flat]), k=k, engine=pr.name)
    assert out.shape == (len(pairs_per_row), pr.gt_words)
    return [pr.gt_of(row) for row in out]


# ---- 1. the reference's known answer (curves/mnt4753/tests.rs:266-467, curves/mnt6753/tests.rs:319-590)
def known_answer(pairing, pr):
    P, Q, want = pr.kat()
    out = pairing.pairing_product(pr.g1_batch([P]), pr.g2_batch([Q]), engine=pr.name)
    assert [int(v) for v in out[0]] == [int(v) for v in pr.gt_row(want)]        # all k Fq words, in the order of Fp4::write / Fp6::write
    assert pairing.gt_to_bytes(out[0], pr.name) == b"".join(v.to_bytes(96, "little") for v in pr.tower(want))
    tm, total = pairing.last_timing()
    assert tm["miller"] > 0 and tm["final_exp"] > 0 and tm["g_ic"] == 0 and total > 0


# ---- 2. bilinearity at wave and block edges: one row per lane, 64 lanes per block
def bilinearity(pairing, pr, n, seed):
    C1, C2, r, e0 = pr.C1, pr.C2, pr.r, pr.e0
    rng = random.Random(seed)
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
    got = device_product(pairing, pr, rows)
    assert len(got) == n
    bad = [i for i in range(n) if got[i] != exp[i]]
    assert not bad, bad


# ---- 3. products of two and three pairs under one final exponentiation
def products(pairing, pr, k, seed):
    C1, C2, r = pr.C1, pr.C2, pr.r
    rng = random.Random(seed)
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
    got = device_product(pairing, pr, rows)
    assert got == exp


# ---- 4. the chunks of launch_pairs after the first (tests/slab_chunks.py)
def product_in_three_slab_chunks(pairing, pr, k, seed, monkeypatch, capfd):
    """gh_pairing_product of 261 rows in chunks of 128, 128 and 5 rows: pair t = i k + j of row i is ((a0 + t) G1, (b0 + 7 t) G2),
    so no two rows share a point, and the row's value is e0^(sum_j a b): every row against that, not a sample; over MNT6 the
    rows of SAMPLE against the restatement's own pairing too"""
    import slab_chunks as K
    engine = pr.name
    C1, C2, r, e0 = pr.C1, pr.C2, pr.r, pr.e0
    rng = random.Random(seed)
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
    g1, g2 = pr.g1_batch(ps), pr.g2_batch(qs)
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: pairing.pairing_product(g1, g2, k=k, engine=engine))
    assert K.chunk_lines(err, LOOP[engine]) == K.THREE, err
    if engine == "mnt6753":
        assert K.chunk_lines(err, "launch_pairs") == [], err                     # MNT4's launches keep their own name
    assert K.identical(plain, cut)
    exp = [pr.fpow(e0, sum(a * b for a, b in row) % r) for row in ab]
    if k == 1:
        assert exp[131] == exp[258] == pr.ONE
    bad = [i for i in range(K.N) if pr.gt_of(cut[i]) != exp[i]]
    assert not bad, bad
    if engine == "mnt6753":
        for i in K.SAMPLE:
            assert pr.gt_of(cut[i]) == pr.pairing(ps[i], qs[i]), i
