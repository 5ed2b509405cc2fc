"""Batched group membership, decompression and compression of points on the device, and Groth16 verification of validated
proofs over both engines (include/ginger_hip_points.h through ginger-lib_amd/points.py and pairing.py), against the Python
restatement tests/points_ref.py and the reference's known points (tests/golden/compression_kats.json).  Every comparison is
exact and no row is skipped.  What a row must give is known from how it was built; the Python reference evaluates r P in full
for a few rows per curve only.  Batch sizes are the wave and block edges 1, 63, 65, 130 (one row per lane, 64 lanes a block)."""
import importlib
import json
import os
import random

import numpy as np
import pytest

import pairing_ref
import points_ref as pr
import pyref
from groth16_exp_key import ExpKey

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "compression_kats.json")))
CURVES = ["mnt4753_g1", "mnt4753_g2", "mnt6753_g1", "mnt6753_g2"]
SIZES = [1, 63, 65, 130]


@pytest.fixture(scope="module")
def points(gpu):
    return importlib.import_module("ginger_lib_amd.points")


# ---- layouts
def point_row(C, P):
    if P is None:
        return np.zeros(24 * C.deg, dtype=np.uint64)
    return np.array(pyref.ext_to_abi(C.F, P[0]) + pyref.ext_to_abi(C.F, P[1]), dtype=np.uint64)


def batch(C, pts):
    return np.stack([point_row(C, P) for P in pts]), np.array([P is None for P in pts], dtype=np.uint8)


def point_of(C, row):
    row = [int(v) for v in row]
    return pyref.ext_from_abi(C.F, row[:12 * C.deg], C.deg), pyref.ext_from_abi(C.F, row[12 * C.deg:], C.deg)


def x_row(x):
    return np.array([w for c in x for w in pyref.int_to_limbs(c)], dtype=np.uint64)


def x_of(row, deg):
    return tuple(pyref.limbs_to_int(row[12 * c:12 * c + 12]) for c in range(deg))


def kat_point(name, which):
    d = KATS[name][which]
    return tuple(int(v, 16) for v in d["x"]), tuple(int(v, 16) for v in d["y"])


def outside_point(C):
    """an on-curve point of a G2 found by the Python root: outside the subgroup of order r (the Python reference evaluates r T)"""
    x = (5, 1) + (0,) * (C.deg - 2)
    while pr.field_sqrt(C, pr.rhs(C, x)) is None:
        x = (x[0] + 1,) + x[1:]
    st, T = pr.decompress(C, x, 0, check_subgroup=False)
    assert st == pr.OK and C.on_curve(T)
    return T


def spread(pool, n, seed):
    """indices of n entries of the pool in a seeded order, every entry present where n allows"""
    rng = random.Random(seed)
    idx = [i % len(pool) for i in range(n)]
    rng.shuffle(idx)
    return idx


# ---------------------------------------------------------------------------------------------------- membership
@pytest.fixture(scope="module")
def member_pools():
    """per curve: [(point, expected verdict)]; the verdict is known from the construction, and the Python reference's r P
    confirms at most 8 rows per curve"""
    pools = {}
    for name in CURVES:
        C = pyref.CURVES[name]
        G = C.G
        inside = [C.mul(k, G) for k in (1, 2, 3, 7, 1000003)]
        off = [(P[0], C.E.add(P[1], C.E.one())) for P in inside[:2]] + [(C.E.one(), C.E.one())]
        assert not any(C.on_curve(P) for P in off)
        pool = [(P, True) for P in inside] + [(None, True), (C.neg(inside[2]), True)] + [(P, False) for P in off]
        checked = [inside[0], inside[4]]
        if C.deg > 1:
            T = outside_point(C)
            shifted = [C.add(T, P) for P in inside[:3]]              # T + k G: outside, because k G is inside and T is not
            multiples = [C.mul(j, T) for j in (2, 3)]
            pool += [(P, False) for P in [T] + shifted + multiples]
            checked += [T, shifted[0]] + multiples
        assert len(checked) <= 8
        for P in checked:                                            # r P in full, by the Python reference
            assert pr.membership(C, P) == dict((id(Q), v) for Q, v in pool)[id(P)]
        pools[name] = pool
    return pools


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", CURVES)
def test_group_membership(points, member_pools, name, n):
    C, pool = pyref.CURVES[name], member_pools[name]
    idx = spread(pool, n, 7000 + n)
    bad = next(i for i, (_, v) in enumerate(pool) if not v and pool[i][0] is not None and (C.deg == 1 or C.on_curve(pool[i][0])))
    for lane in (0, 63, 64, n - 1):                                  # a failing row in the first and the last lane of a block
        if lane < n:
            idx[lane] = bad
    if n > 2:
        idx[1] = pool.index((None, True))
    got = points.group_membership_test(name, batch(C, [pool[i][0] for i in idx]))
    assert got.shape == (n,)
    wrong = [k for k in range(n) if bool(got[k]) != pool[idx[k]][1]]
    assert not wrong, wrong
    tm, total = points.last_timing()
    assert tm["validate"] > 0 and total > 0


# ---------------------------------------------------------------------------------------------------- decompression
def rhs_c1_zero_rows(C):
    """MNT4-753 G2: two x = (x0, x1) with (x^3 + a x + b).c1 = 0, one whose c0 is a residue of Fq and one whose c0 is not, with
    the reference's answers.  c1 is 3 x1 x0^2 + c1(rhs(0, x1)): pick x1, solve the quadratic for x0."""
    F1 = pyref.Ext(C.F, 1, 0)
    p = C.E.p
    found = {}
    x1 = 1
    while len(found) < 2:
        sq = -pr.rhs(C, (0, x1))[1] * pow(3 * x1, -1, p) % p
        x0 = pr.sqrt_ts(F1, (sq,))
        if x0 is not None:
            x = (x0[0], x1)
            c0, c1 = pr.rhs(C, x)
            assert c1 == 0
            found.setdefault(pr.is_square(F1, (c0,)), x)
        x1 += 1
    rows = []
    for residue, x in sorted(found.items()):
        st, P = pr.decompress(C, x, 0)                               # the reference's answer, r P in full where a root exists
        assert st == (pr.NOT_ON_CURVE if not residue else st) and (residue or pr.is_square(C.E, pr.rhs(C, x)))   # the quirk: a root exists in Fq2
        rows.append((x, 0, st, P))
    assert rows[0][2] == pr.NOT_ON_CURVE and rows[1][2] in (pr.OK, pr.NOT_PRIME_ORDER)
    return rows


@pytest.fixture(scope="module")
def decompress_pools():
    """per curve: [(x coefficients as sent, flags, expected status, expected point or None)]"""
    pools = {}
    for name in CURVES:
        C = pyref.CURVES[name]
        E, p, zero = C.E, C.E.p, C.E.zero()
        pool = []
        for which in ("even", "odd"):                                # the reference's known points
            P = kat_point(name, which)
            pool.append((P[0], pr.FLAG_PARITY if which == "odd" else 0, pr.OK, P))
        for k in (1, 2, 5, 11, 1000003):                             # k G, and -k G by the other parity
            P = C.mul(k, C.G)
            x, fl = pr.compress(C, P)
            pool += [(x, fl, pr.OK, P), (x, fl ^ pr.FLAG_PARITY, pr.OK, C.neg(P))]
        gx = C.G[0]
        pool.append((zero, pr.FLAG_INFINITY, pr.OK, None))           # the one legal way to write infinity
        pool += [(x, fl, pr.INVALID_FLAGS, None) for x, fl in ((zero, 3), (gx, 1), (gx, 3), (gx, 4), (gx, 6), (zero, 0x80), (zero, 5), (gx, 0xfd))]
        for pos in range(C.deg):                                     # a coefficient at the modulus and above it, before any flag counts
            for bad in (p, p + 1, (1 << 768) - 1):
                x = tuple(bad if c == pos else gx[c] for c in range(C.deg))
                pool += [(x, 0, pr.INVALID_FIELD_ELEMENT, None), (x, 7, pr.INVALID_FIELD_ELEMENT, None)]
        x = (2,) + (0,) * (C.deg - 1)                                # no root: Euler's criterion in Python decides
        none = []
        while len(none) < 2:
            if not pr.is_square(E, pr.rhs(C, x)):
                none.append(x)
            x = (x[0] + 1,) + x[1:]
        pool += [(x, fl, pr.NOT_ON_CURVE, None) for x in none for fl in (0, 2)]
        if C.deg == 1:                                               # x = 0: b is a square on both G1, either parity decompresses
            for fl in (0, 2):
                st, P = pr.decompress(C, zero, fl)
                assert st == pr.OK and pr.is_odd(P[1]) == bool(fl)
                pool.append((zero, fl, pr.OK, P))
        else:                                                        # the twisted b is not a square
            assert not pr.is_square(E, C.b)
            pool += [(zero, 0, pr.NOT_ON_CURVE, None), (zero, 2, pr.NOT_ON_CURVE, None)]
            T = outside_point(C)                                     # on the twist, outside the subgroup
            assert not pr.membership(C, T)
            pool += [(T[0], 0, pr.NOT_PRIME_ORDER, None), (T[0], 2, pr.NOT_PRIME_ORDER, None)]
            TG = C.add(T, C.G)
            pool.append(pr.compress(C, TG) + (pr.NOT_PRIME_ORDER, None))
        if name == "mnt4753_g2":
            pool += rhs_c1_zero_rows(C)
        pools[name] = pool
    return pools


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", CURVES)
def test_decompress(points, decompress_pools, name, n):
    C, pool = pyref.CURVES[name], decompress_pools[name]
    idx = spread(pool, n, 8000 + n) if n > 1 else [0]
    bad = next(i for i, row in enumerate(pool) if row[2] == pr.NOT_ON_CURVE)
    for lane in (0, 63, 64, n - 1):                                  # a failing row in the first and the last lane of a block
        if lane < n and n > 1:
            idx[lane] = bad
    if n == 130:
        idx[2:2 + len(pool)] = range(len(pool))                      # every row of the pool at the largest size
        idx[0] = idx[63] = idx[64] = idx[n - 1] = bad
    rows = [pool[i] for i in idx]
    x = np.stack([x_row(r[0]) for r in rows])
    flags = np.array([r[1] for r in rows], dtype=np.uint8)
    (xy, inf), st = points.decompress_limbs(name, x, flags)
    assert xy.shape == (n, 24 * C.deg) and inf.shape == (n,) and st.shape == (n,)
    wrong = []
    for k, (_, fl, want, P) in enumerate(rows):
        if int(st[k]) != want:
            wrong.append((k, idx[k], int(st[k]), want))
        elif want != pr.OK:
            ok = not xy[k].any() and inf[k] == 0                     # a failed row is zero
        elif P is None:
            ok = inf[k] == 1 and point_of(C, xy[k]) == (C.E.zero(), C.E.one())     # GroupAffine::zero()
        else:
            ok = inf[k] == 0 and point_of(C, xy[k]) == P and pr.is_odd(P[1]) == bool(fl & pr.FLAG_PARITY)
        if int(st[k]) == want and not ok:
            wrong.append((k, idx[k], "value"))
    assert not wrong, wrong


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", CURVES)
def test_compress_round_trip(points, name, n):
    """compress -> decompress of k G at each n, the point at infinity among them; compress equals the restatement's"""
    C = pyref.CURVES[name]
    rng = random.Random(9000 + n)
    base = [C.mul(rng.randrange(1, 1 << 16), C.G) for _ in range(min(n, 6))] + [None, kat_point(name, "even"), kat_point(name, "odd")]
    pts = [base[i % len(base)] for i in range(n)] if n > 1 else [base[0]]
    pts = [C.neg(P) if P is not None and i % 2 else P for i, P in enumerate(pts)]
    x, flags = points.compress_limbs(name, batch(C, pts))
    want = [pr.compress(C, P) for P in pts]
    assert [(x_of(x[k], C.deg), int(flags[k])) for k in range(n)] == want
    (xy, inf), st = points.decompress_limbs(name, x, flags)
    assert not st.any()
    for k, P in enumerate(pts):
        assert (inf[k] == 1 and point_of(C, xy[k]) == (C.E.zero(), C.E.one())) if P is None else (inf[k] == 0 and point_of(C, xy[k]) == P), k
    # the same through the reference's Vec<bool> layout
    bits = points.compress(name, batch(C, pts[:3]))
    assert [b.tolist() for b in bits] == [pr.to_bits(*w) for w in want[:3]]
    (xy2, inf2), st2 = points.decompress(name, bits)
    assert not st2.any() and (xy2 == xy[:3]).all() and (inf2 == inf[:3]).all()


# ---------------------------------------------------------------------------------------------------- validated verification
@pytest.fixture(scope="module", params=["mnt4753", "mnt6753"])
def validated(request, gpu):
    """per engine: the key known in the exponent (tests/groth16_exp_key.py) with the inputs s and the proofs drawn after it,
    and rows (A, B, C, expected status, expected point status) for the checked entry point: two valid proofs, C + G (a false proof of valid points), B on the twist outside the subgroup, B = T + B (the same, in another
    position), A off its curve, C off its curve, A at infinity"""
    engine = request.param
    ref = pairing_ref.engine(engine)
    pairing = importlib.import_module("ginger_lib_amd.pairing")
    K = ExpKey(ref, 1500 + len(engine))
    C1, C2, rng = ref.C1, ref.C2, K.rng
    s = [rng.randrange(1, ref.r), rng.randrange(1, ref.r)]

    def proof():
        a, b = rng.randrange(1, ref.r), rng.randrange(1, 1 << 20)
        return K.g1(a), C2.mul(b, C2.G), K.g1(K.c_of(a, b, s))
    A, B, C = proof()
    A2, B2, Cc2 = proof()
    T = outside_point(C2)
    off = (A[0], C1.E.add(A[1], C1.E.one()))
    assert not C1.on_curve(off) and C2.on_curve(T)
    rows = [(A, B, C, 1, [0, 0, 0]), (A2, B2, Cc2, 1, [0, 0, 0]), (A, B, C1.add(C, C1.G), 0, [0, 0, 0]),
            (A, T, C, 3, [0, pr.NOT_PRIME_ORDER, 0]), (A2, C2.add(T, B2), Cc2, 3, [0, pr.NOT_PRIME_ORDER, 0]),
            (off, B, C, 3, [pr.NOT_ON_CURVE, 0, 0]), (A, T, off, 3, [0, pr.NOT_PRIME_ORDER, pr.NOT_ON_CURVE]), (None, B, C, 0, [0, 0, 0])]
    pvk = K.pvk(pairing)
    yield {"engine": engine, "ref": ref, "inputs": lambda n: ref.input_rows([s] * n), "rows": rows, "pvk": pvk, "pairing": pairing}
    pvk.close()


def _abc(ref, rows):
    return batch(ref.C1, [r[0] for r in rows]), batch(ref.C2, [r[1] for r in rows]), batch(ref.C1, [r[2] for r in rows])


@pytest.mark.parametrize("n", [8, 130])
def test_verify_checked(points, validated, n):
    ref, inputs, pvk, pairing = validated["ref"], validated["inputs"], validated["pvk"], validated["pairing"]
    order = list(range(8)) if n == 8 else spread(validated["rows"], n, 1300)
    rows = [validated["rows"][i] for i in order]
    a, b, c = _abc(ref, rows)
    st, pst = pvk.verify_checked(a, b, c, inputs(n))
    assert [int(v) for v in st] == [r[3] for r in rows]
    assert pst.tolist() == [r[4] for r in rows]
    tm, _ = points.last_timing()
    ptm, _ = pairing.last_timing()
    assert tm["validate"] > 0 and tm["upload"] == 0 and all(ptm[ph] > 0 for ph in ("g_ic", "miller", "final_exp"))
    # gh_groth16_verify on the rows of valid points returns what it returned before; on the rows it cannot judge, anything but a fault
    plain = [int(v) for v in pvk.verify(a, b, c, inputs(n))]
    for k, r in enumerate(rows):
        if r[3] != 3:
            assert plain[k] == r[3], k
        elif pr.NOT_ON_CURVE in r[4]:
            assert plain[k] == 2, k
        else:
            assert plain[k] in (0, 1), k


@pytest.mark.parametrize("n", [8, 130])
def test_verify_compressed(points, validated, n):
    """the same proofs in the wire form, compressed by the device; then rows that do not decompress"""
    ref, inputs, pvk = validated["ref"], validated["inputs"], validated["pvk"]
    C1 = ref.C1
    g1, g2 = "%s_g1" % validated["engine"], "%s_g2" % validated["engine"]
    good = [r for r in validated["rows"] if pr.NOT_ON_CURVE not in r[4]]         # an off-curve point has no compressed form
    order = list(range(len(good))) if n == 8 else spread(good, n - 2, 1400)
    rows = [good[i] for i in order]
    a, b, c = _abc(ref, rows)
    ax, af = points.compress_limbs(g1, a)
    bx, bf = points.compress_limbs(g2, b)
    cx, cf = points.compress_limbs(g1, c)
    want = [(r[3], r[4]) for r in rows]
    # two more rows, copies of the first valid proof: A's x has no root; C's x is the modulus and B's flags are illegal
    x = (2,)
    while pr.is_square(C1.E, pr.rhs(C1, x)):
        x = (x[0] + 1,)
    first = next(k for k, r in enumerate(rows) if r[3] == 1)
    ax, af = np.vstack([ax, x_row(x), ax[first]]), np.concatenate([af, [0], [af[first]]]).astype(np.uint8)
    bx, bf = np.vstack([bx, bx[first], bx[first]]), np.concatenate([bf, [bf[first]], [bf[first] | 1]]).astype(np.uint8)
    cx, cf = np.vstack([cx, cx[first], x_row((C1.E.p,))]), np.concatenate([cf, [cf[first]], [cf[first]]]).astype(np.uint8)
    want += [(3, [pr.NOT_ON_CURVE, 0, 0]), (3, [0, pr.INVALID_FLAGS, pr.INVALID_FIELD_ELEMENT])]
    m = len(want)
    st, pst = pvk.verify_compressed((ax, af), (bx, bf), (cx, cf), inputs(m))
    assert [int(v) for v in st] == [w[0] for w in want]
    assert pst.tolist() == [w[1] for w in want]
