"""The Bowe-Hopwood hash, the joint double-scalar multiplication and the field-based EC-VRF on the device
(include/ginger_hip_ecvrf.h), against the Python restatement tests/ecvrf_ref.py and the device's gh_batch_mul."""
import random

import numpy as np
import pytest

import ecvrf_ref
import poseidon_ref
import pyref
from schnorr_ref import BOUND, mul

pytestmark = pytest.mark.gpu
SCHEMES = list(ecvrf_ref.SCHEMES)
NUM_WINDOWS, WINDOW_SIZE = 4, 128          # 512 chunks: messages of up to two field elements


def limbs(vals):
    return np.array([pyref.int_to_limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 12)


def to_int(row):
    return pyref.limbs_to_int([int(v) for v in row])


def pts_abi(V, pts):
    xy = np.zeros((len(pts), 24), dtype=np.uint64)
    inf = np.zeros(len(pts), dtype=np.uint8)
    for i, P in enumerate(pts):
        xy[i], inf[i] = V.pt_abi(P)
    return xy, inf


def proj_to_aff(V, row):
    X, Y, Z = (V.from_fe(row[12 * c:12 * c + 12]) for c in range(3))
    if Z == 0:
        return None
    zi = pow(Z, -1, V.p)
    return ((X * zi % V.p,), (Y * zi % V.p,))


def msg_arr(V, msgs, L):
    return np.array([[V.fe(x) for x in m] for m in msgs], dtype=np.uint64).reshape(len(msgs), L, 12)


def cs_arr(V, proofs):
    return np.array([V.fe(c) + V.fe(s) for _, c, s in proofs], dtype=np.uint64).reshape(-1, 24)


@pytest.fixture(scope="module")
def setups(gpu):
    """per scheme: (restatement, device VRF, device BH); recipe generators from random segment bases"""
    from ginger_lib_amd import ecvrf, poseidon
    out = {}
    for s, (tag, curve) in ecvrf_ref.SCHEMES.items():
        C = pyref.CURVES[curve]
        bh = ecvrf_ref.make_bh(C, random.Random(len(s)), NUM_WINDOWS, WINDOW_SIZE)
        V = ecvrf_ref.EcVrf(s, bh)
        xy, inf = pts_abi(V, bh.flat())
        dbh = ecvrf.BoweHopwoodPedersenCRH(curve, xy, inf, NUM_WINDOWS, WINDOW_SIZE)
        prm = poseidon.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, tag)
        out[s] = (V, ecvrf.FieldBasedEcVrf(prm, dbh, curve), dbh)
    yield out
    for V, D, B in out.values():
        D.close()
        B.close()


# ---------------------------------------------------------------- 1. gh_bh_hash
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bh_hash_matches_restatement(gpu, scheme):
    from ginger_lib_amd import ecvrf
    curve = ecvrf_ref.SCHEMES[scheme][1]
    C = pyref.CURVES[curve]
    rng = random.Random(21 + len(scheme))
    V = ecvrf_ref.EcVrf(scheme, None)
    bh = ecvrf_ref.make_bh(C, rng, 2, 64, recipe=False)         # independent random generators, one at infinity
    bh.gens[0][5] = None
    xy, inf = pts_abi(V, bh.flat())
    D = ecvrf.BoweHopwoodPedersenCRH(curve, xy, inf, 2, 64)
    try:
        cap = bh.capacity_bits() // 8
        for nbytes in (0, 1, 2, 3, 23, 24, cap):
            data = np.array([[rng.randrange(256) for _ in range(nbytes)] for _ in range(6)], dtype=np.uint8).reshape(6, nbytes)
            if nbytes:
                data[0] = 0xFF
                data[1, 0] = 0b00100000                         # chunk 1 = (0, 0, 1) touches no infinity generator
            oxy, oinf = D.evaluate(data)
            for i in range(6):
                assert V.pt_from_abi(oxy[i], oinf[i]) == bh.evaluate(bytes(data[i].tolist())), (nbytes, i)
        with pytest.raises(ecvrf.GingerHipError, match="-1"):
            D.evaluate(np.zeros((1, cap + 1), dtype=np.uint8))
    finally:
        D.close()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_bh_hash_recipe_closed_form_and_2p16(setups, scheme):
    V, _, D = setups[scheme]
    rng = np.random.default_rng(3 + len(scheme))
    for nbytes in (95, 96, 97, 192):
        data = rng.integers(0, 256, size=(4, nbytes), dtype=np.uint8)
        oxy, oinf = D.evaluate(data)
        for i in range(4):
            want = None
            for seg in range(NUM_WINDOWS):
                digits = V.bh.chunks(bytes(data[i].tolist()))[seg * WINDOW_SIZE:(seg + 1) * WINDOW_SIZE]
                k = sum(d * 16 ** j for j, d in enumerate(digits)) % V.r
                want = V.C.add(want, mul(V.C, k, V.bh.gens[seg][0]))
            assert V.pt_from_abi(oxy[i], oinf[i]) == want, (nbytes, i)
    n = 1 << 16
    data = rng.integers(0, 256, size=(n, 96), dtype=np.uint8)
    oxy, oinf = D.evaluate(data)
    for i in rng.choice(n, size=64, replace=False):
        assert V.pt_from_abi(oxy[i], oinf[i]) == V.bh.evaluate(bytes(data[i].tolist())), i


# ---------------------------------------------------------------- 2. gh_batch_double_mul
@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_double_mul_matches_restatement(gpu, scheme):
    from ginger_lib_amd import ecvrf
    curve = ecvrf_ref.SCHEMES[scheme][1]
    V = ecvrf_ref.EcVrf(scheme, None)
    C, r = V.C, V.r
    rng = random.Random(5 + len(scheme))
    top = (1 << 753) - 1
    rows = []                                                   # (P1, k1, P2, k2)
    for k in (0, 1, r - 1, top):
        rows.append((ecvrf_ref.random_point(C, rng), k, ecvrf_ref.random_point(C, rng), rng.randrange(r)))
        rows.append((ecvrf_ref.random_point(C, rng), rng.randrange(r), ecvrf_ref.random_point(C, rng), k))
    P = ecvrf_ref.random_point(C, rng)
    k = rng.randrange(r)
    rows += [(P, k, P, k), (P, k, P, rng.randrange(r)), (P, k, C.neg(P), k), (P, top, C.neg(P), top)]
    rows += [(None, rng.randrange(r), P, k), (P, k, None, rng.randrange(r)), (None, 5, None, 7)]
    rows += [(ecvrf_ref.random_point(C, rng), rng.randrange(1 << 753), ecvrf_ref.random_point(C, rng), rng.randrange(1 << 753))
             for _ in range(20)]
    xy1, inf1 = pts_abi(V, [x[0] for x in rows])
    xy2, inf2 = pts_abi(V, [x[2] for x in rows])
    out = ecvrf.batch_double_mul(curve, xy1, limbs([x[1] for x in rows]), xy2, limbs([x[3] for x in rows]), inf1, inf2)
    for i, (P1, k1, P2, k2) in enumerate(rows):
        assert proj_to_aff(V, out[i]) == C.add(mul(C, k1, P1), mul(C, k2, P2)), i
    assert proj_to_aff(V, out[10]) is None                       # P2 = -P1, k2 = k1
    # without infinity bytes
    out2 = ecvrf.batch_double_mul(curve, xy1[-20:], limbs([x[1] for x in rows[-20:]]), xy2[-20:], limbs([x[3] for x in rows[-20:]]))
    assert np.array_equal(out2, out[-20:])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_double_mul_matches_batch_mul_at_2p16(gpu, scheme):
    """k1 P + k2 (7 P) == (k1 + 7 k2) P through gh_batch_mul, every row"""
    from ginger_lib_amd import ecvrf, schnorr
    curve = ecvrf_ref.SCHEMES[scheme][1]
    V = ecvrf_ref.EcVrf(scheme, None)
    rng = random.Random(9)
    n = 1 << 16
    bases = [ecvrf_ref.random_point(V.C, rng) for _ in range(8)]
    P1 = [bases[i % 8] for i in range(n)]
    xy1, _ = pts_abi(V, bases)
    xy2, _ = pts_abi(V, [mul(V.C, 7, B) for B in bases])
    xy1, xy2 = np.tile(xy1, (n // 8, 1)), np.tile(xy2, (n // 8, 1))
    rs = np.random.default_rng(11)
    k1 = rs.integers(0, 1 << 63, size=(n, 12), dtype=np.uint64)
    k2 = rs.integers(0, 1 << 63, size=(n, 12), dtype=np.uint64)
    k1[:, 11] &= np.uint64((1 << 45) - 1)                        # below 2^749: k1 + 7 k2 < 2^753
    k2[:, 11] &= np.uint64((1 << 45) - 1)
    k1[0] = 0
    k2[1] = 0
    ks = [to_int(k1[i]) + 7 * to_int(k2[i]) for i in range(n)]
    want = schnorr.batch_mul(curve, xy1, limbs(ks))
    got = ecvrf.batch_double_mul(curve, xy1, k1, xy2, k2)
    p = V.p
    bad = []
    for i in range(n):
        a, b = got[i], want[i]
        X1, Y1, Z1 = to_int(a[:12]), to_int(a[12:24]), to_int(a[24:])
        X2, Y2, Z2 = to_int(b[:12]), to_int(b[12:24]), to_int(b[24:])
        if (Z1 == 0 or Z2 == 0) and Z1 != Z2 or (X1 * Z2 - X2 * Z1) % p or (Y1 * Z2 - Y2 * Z1) % p:
            bad.append(i)
    assert not bad, bad[:8]
    assert proj_to_aff(V, got[5]) == mul(V.C, ks[5], P1[5])


# ---------------------------------------------------------------- 3. / 4. prove and proof_to_hash against the restatement
def _rows(V, rng, n, L):
    out = []
    for _ in range(n):
        sk = rng.randrange(V.r)
        out.append((sk, V.pk(sk), [rng.randrange(V.p) for _ in range(L)]))
    return out


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("L", [0, 1, 2])
def test_prove_and_proof_to_hash_against_restatement(setups, scheme, L):
    V, D, _ = setups[scheme]
    rng = random.Random(100 * L + len(scheme))
    n = 10
    rows = _rows(V, rng, n, L)
    sks, pks, msgs = [x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows]
    xy, inf = D.get_public_key(limbs([V.R.to_mont(sk) for sk in sks]))
    exy, einf = pts_abi(V, pks)
    assert np.array_equal(xy, exy) and np.array_equal(inf, einf)
    assert D.keyverify((xy, inf)).all()
    ma = msg_arr(V, msgs, L)
    # prove with the restatement's nonces: identical words, status 0 exactly where the restatement rejects
    nonces = [rng.randrange(V.r) for _ in range(n)]
    nonces[0] = 0
    want = [V.prove_with(sk, pk, m, k) for sk, pk, m, k in zip(sks, pks, msgs, nonces)]
    (gxy, ginf), cs, st = D.prove(limbs([V.R.to_mont(x) for x in sks]), (xy, inf), ma, limbs([V.R.to_mont(k) for k in nonces]))
    assert [int(x) for x in st] == [0 if w is None else 1 for w in want]
    for i, w in enumerate(want):
        assert V.pt_from_abi(gxy[i], ginf[i]) == V.gamma_of(sks[i], msgs[i]), i
        if w is None:
            assert not cs[i].any()
        else:
            assert (V.from_fe(cs[i][:12]), V.from_fe(cs[i][12:])) == w[1:], i
    # proof_to_hash of the restatement's valid proofs: 1 and the restatement's output
    good = [V.prove(sk, pk, m, rng) for sk, pk, m in rows]
    gm = pts_abi(V, [pr[0] for pr in good])
    out, st = D.proof_to_hash((xy, inf), ma, gm, cs_arr(V, good))
    assert list(st) == [1] * n
    for i in range(n):
        code, o = V.proof_to_hash(pks[i], msgs[i], good[i])
        assert code == ecvrf_ref.OK and V.from_fe(out[i]) == o, i
    # tampering: c +- 1, s +- 1, another gamma on the curve -> 0; c or s >= 2^752 -> 2; gamma off the curve -> 3
    bad, expect = list(good), []
    other = ecvrf_ref.random_point(V.C, rng)
    for i in range(n):
        g_, c, s = good[i]
        kind = i % 9
        bad[i] = [(g_, c, s), (g_, (c + 1) % BOUND, s), (g_, (c - 1) % BOUND, s), (g_, c, (s + 1) % BOUND), (g_, c, (s - 1) % BOUND),
                  (other, c, s), (g_, BOUND + c % (V.p - BOUND), s), (g_, c, BOUND + s % (V.p - BOUND)), (g_, c, s)][kind]
        expect.append([1, 0, 0, 0, 0, 0, 2, 2, 3][kind])
    gxy_b, ginf_b = pts_abi(V, [pr[0] for pr in bad])
    for i in range(n):
        if i % 9 == 8:                                          # off the curve: y + 1
            gxy_b[i, 12:] = V.fe(bad[i][0][1][0] + 1) if bad[i][0] else V.fe(2)
            ginf_b[i] = 0
    out, st = D.proof_to_hash((xy, inf), ma, (gxy_b, ginf_b), cs_arr(V, bad))
    assert [int(x) for x in st] == expect
    assert not out[np.array(expect) != 1].any()
    for i in range(min(n, 9)):
        P = V.pt_from_abi(gxy_b[i], ginf_b[i])
        assert V.proof_to_hash(pks[i], msgs[i], (P,) + tuple(bad[i][1:]))[0] == expect[i], i
    # another message, another key -> 0
    if L:
        msgs2 = [list(m) for m in msgs]
        for m in msgs2:
            m[-1] = (m[-1] + 1) % V.p
        assert list(D.proof_to_hash((xy, inf), msg_arr(V, msgs2, L), gm, cs_arr(V, good))[1]) == [0] * n
    rot = np.roll(np.arange(n), 1)
    assert list(D.proof_to_hash((xy[rot], inf[rot]), ma, gm, cs_arr(V, good))[1]) == [0] * n


# ---------------------------------------------------------------- 5. edge cases
@pytest.mark.parametrize("scheme", SCHEMES)
def test_edge_cases(setups, scheme):
    V, D, _ = setups[scheme]
    rng = random.Random(77 + len(scheme))
    # pk = infinity (sk = 0): proves and verifies
    xy0, inf0 = D.get_public_key(limbs([0]))
    assert inf0[0] == 1 and D.keyverify((xy0, inf0))[0]
    m0 = [rng.randrange(V.p)]
    while True:
        k = rng.randrange(1, V.r)
        w = V.prove_with(0, None, m0, k)
        if w:
            break
    (gxy, ginf), cs, st = D.prove(limbs([0]), (xy0, inf0), msg_arr(V, [m0], 1), limbs([V.R.to_mont(k)]))
    assert st[0] == 1 and ginf[0] == 1 and (V.from_fe(cs[0][:12]), V.from_fe(cs[0][12:])) == w[1:]
    out, st = D.proof_to_hash((xy0, inf0), msg_arr(V, [m0], 1), (gxy, ginf), cs)
    assert st[0] == 1 and V.from_fe(out[0]) == V.proof_to_hash(None, m0, w)[1]
    # L = 0: mh = gamma = v = infinity
    sk = rng.randrange(V.r)
    pk = V.pk(sk)
    xy, inf = pts_abi(V, [pk])
    w = V.prove(sk, pk, [], rng)
    assert w[0] is None
    gm = pts_abi(V, [w[0]])
    out, st = D.proof_to_hash((xy, inf), np.zeros((1, 0, 12), dtype=np.uint64), gm, cs_arr(V, [w]))
    assert st[0] == 1 and V.from_fe(out[0]) == V.proof_to_hash(pk, [], w)[1]
    # gamma = infinity supplied for a message with mh != infinity: a well-formed point, so the verdict is the hash's
    m = [rng.randrange(V.p)]
    w = V.prove(sk, pk, m, rng)
    forged = (None, w[1], w[2])
    out, st = D.proof_to_hash((xy, inf), msg_arr(V, [m], 1), pts_abi(V, [None]), cs_arr(V, [forged]))
    code, _ = V.proof_to_hash(pk, m, forged)
    assert int(st[0]) == code == ecvrf_ref.FAILED
    # an off-curve key
    bad = xy.copy()
    bad[0, 12:] = V.fe(pk[1][0] + 1)
    assert not D.keyverify((bad, np.zeros(1, dtype=np.uint8)))[0]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_non_canonical_input_is_rejected(setups, scheme):
    from ginger_lib_amd import ecvrf
    V, D, _ = setups[scheme]
    xy, inf = pts_abi(V, [V.G])
    cs = np.zeros((1, 24), dtype=np.uint64)
    msg = np.zeros((1, 1, 12), dtype=np.uint64)
    msg[0, 0] = pyref.int_to_limbs(V.p)
    with pytest.raises(ecvrf.GingerHipError, match="-1"):
        D.proof_to_hash((xy, inf), msg, (xy, inf), cs)
    cs[0, 12:] = pyref.int_to_limbs(V.p)
    with pytest.raises(ecvrf.GingerHipError, match="-1"):
        D.proof_to_hash((xy, inf), np.zeros((1, 1, 12), dtype=np.uint64), (xy, inf), cs)
    with pytest.raises(ecvrf.GingerHipError, match="-1"):
        D.get_public_key(limbs([V.r]))
    with pytest.raises(ecvrf.GingerHipError, match="-1"):               # 3 elements: more than 512 chunks
        D.proof_to_hash((xy, inf), np.zeros((1, 3, 12), dtype=np.uint64), (xy, inf), np.zeros((1, 24), dtype=np.uint64))


# ---------------------------------------------------------------- 6. 2^18 rows, device only
def _random_elems(rs, n, p):
    a = rs.integers(0, 1 << 63, size=(n, 12), dtype=np.uint64) * 2 + rs.integers(0, 2, size=(n, 12), dtype=np.uint64)
    a[:, 11] = a[:, 11] % np.uint64(p >> (64 * 11))
    return a


@pytest.mark.parametrize("scheme", SCHEMES)
def test_device_round_trip_2p18(setups, scheme):
    V, D, _ = setups[scheme]
    n = 1 << 18
    rs = np.random.default_rng(18 + len(scheme))
    sk = _random_elems(rs, n, V.r)
    msg = _random_elems(rs, n, V.p).reshape(n, 1, 12)
    xy, inf = D.get_public_key(sk)
    gxy = np.zeros((n, 24), dtype=np.uint64)
    ginf = np.zeros(n, dtype=np.uint8)
    cs = np.zeros((n, 24), dtype=np.uint64)
    todo = np.arange(n)
    for rnd in range(64):                      # about 32 % of the nonces pass both range checks: 0.68^64 * 2^18 < 1e-5
        nonce = _random_elems(rs, len(todo), V.r)
        (g_, gi_), c_, st = D.prove(sk[todo], (xy[todo], inf[todo]), msg[todo], nonce)
        if rnd == 0:                           # rejections are the restatement's
            for j in np.nonzero(st != 1)[0][:4]:
                i = todo[j]
                pk = V.pt_from_abi(xy[i], inf[i])
                assert V.prove_with(V.R.from_mont(to_int(sk[i])), pk, [V.from_fe(msg[i, 0])], V.R.from_mont(to_int(nonce[j]))) is None
        ok = todo[st == 1]
        gxy[ok], ginf[ok], cs[ok] = g_[st == 1], gi_[st == 1], c_[st == 1]
        todo = todo[st != 1]
        if not len(todo):
            break
    assert not len(todo)
    out, st = D.proof_to_hash((xy, inf), msg, (gxy, ginf), cs)
    assert (st == 1).all()
    # flip one bit in 1 % of the rows (message or c, s words, kept below the modulus)
    flip = rs.choice(n, size=n // 100, replace=False)
    msg2, cs2 = msg.copy(), cs.copy()
    for j, i in enumerate(flip):
        tgt = (msg2[i, 0], cs2[i, :12], cs2[i, 12:])[j % 3]
        tgt[j % 11] ^= np.uint64(1 << (j % 64))
        assert to_int(tgt) < V.p
    out2, st2 = D.proof_to_hash((xy, inf), msg2, (gxy, ginf), cs2)
    assert set(np.nonzero(st2 != 1)[0].tolist()) == set(flip.tolist())
    keep = np.ones(n, dtype=bool)
    keep[flip] = False
    assert np.array_equal(out2[keep], out[keep])
    # 16 sampled rows agree with the restatement
    for i in rs.choice(n, size=16, replace=False):
        pk = V.pt_from_abi(xy[i], inf[i])
        assert pk == V.pk(V.R.from_mont(to_int(sk[i])))
        m = [V.from_fe(msg2[i, 0])]
        proof = (V.pt_from_abi(gxy[i], ginf[i]), V.from_fe(cs2[i][:12]), V.from_fe(cs2[i][12:]))
        code, o = V.proof_to_hash(pk, m, proof)
        assert int(st2[i]) == code, i
        if code == ecvrf_ref.OK:
            assert V.from_fe(out2[i]) == o, i


# ---------------------------------------------------------------- 7. the chunks after the first (tests/slab_chunks.py)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_double_mul_in_three_slab_chunks(gpu, scheme, monkeypatch, capfd):
    """gh_batch_double_mul of 261 rows in chunks of 128, 128 and 5 rows: the chunk line of the joint launch, the same bits as
    in one chunk, and the restatement's points at both sides of every chunk edge and in the special rows (later chunks only)"""
    from ginger_lib_amd import ecvrf
    import slab_chunks as K
    curve = ecvrf_ref.SCHEMES[scheme][1]
    V = ecvrf_ref.EcVrf(scheme, None)
    C = V.C
    rng = random.Random(261 + len(scheme))
    P1, P2, H = ecvrf_ref.random_point(C, rng), ecvrf_ref.random_point(C, rng), mul(C, 3, V.G)
    p1, p2 = [], []
    for _ in range(K.N):                                        # P1 + i G and P2 + 3 i G: bases of its own in every row
        p1.append(P1)
        p2.append(P2)
        P1, P2 = C.add(P1, V.G), C.add(P2, H)
    k1 = [rng.getrandbits(753) for _ in range(K.N)]
    k2 = [rng.getrandbits(753) for _ in range(K.N)]
    K.assert_rows_differ(p1, p2, k1, k2)
    top = (1 << 753) - 1
    p1[131], p2[257] = None, None                               # rows 3 and 259 (1 and 129) are ordinary rows
    k1[140], k2[150], k1[160], k2[258] = 0, 0, top, top
    p2[170], k2[170] = C.neg(p1[170]), k1[170]                  # the two halves cancel
    xy1, inf1 = pts_abi(V, p1)
    xy2, inf2 = pts_abi(V, p2)
    a1, a2 = limbs(k1), limbs(k2)
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: ecvrf.batch_double_mul(curve, xy1, a1, xy2, a2, inf1, inf2))
    assert K.chunk_lines(err, "vb_joint") == K.THREE, err
    assert K.identical(plain, cut)
    for i in K.SAMPLE + (131, 140, 150, 160, 170, 257, 258):
        assert proj_to_aff(V, cut[i]) == C.add(mul(C, k1[i], p1[i]), mul(C, k2[i], p2[i])), i
    assert proj_to_aff(V, cut[170]) is None


_CHUNK_ROWS = {}


def _chunk_rows(V, D, scheme):
    """261 rows of (sk, pk, one message element), shared by the two tests below; sk = 0 (pk, gamma at infinity) in row 131"""
    import slab_chunks as K
    if scheme not in _CHUNK_ROWS:
        rng = random.Random(522 + len(scheme))
        sks = [rng.randrange(1, V.r) for _ in range(K.N)]
        sks[131] = 0
        msgs = [[rng.randrange(V.p)] for _ in range(K.N)]
        K.assert_rows_differ(sks, [m[0] for m in msgs])
        sk = limbs([V.R.to_mont(x) for x in sks])
        pk = D.get_public_key(sk)
        for i in (0, 131, 260):
            assert V.pt_from_abi(pk[0][i], pk[1][i]) == V.pk(sks[i]), i
        _CHUNK_ROWS[scheme] = (sks, sk, pk, msgs, msg_arr(V, msgs, 1))
    return _CHUNK_ROWS[scheme]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_prove_in_three_slab_chunks(setups, scheme, monkeypatch, capfd):
    """EC-VRF prove of 261 rows at L = 1: its one table per row serves two scalar vectors (gamma = sk mh, b = k mh) in every chunk"""
    import slab_chunks as K
    V, D, _ = setups[scheme]
    sks, sk, pk, msgs, ma = _chunk_rows(V, D, scheme)
    rng = random.Random(7 + len(scheme))
    nonces = [rng.randrange(1, V.r) for _ in range(K.N)]
    K.assert_rows_differ(nonces)
    nonces[140] = 0                                             # rejected, in the second chunk only
    ka = limbs([V.R.to_mont(k) for k in nonces])
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: D.prove(sk, pk, ma, ka))
    assert K.chunk_lines(err, "vb_single") == K.THREE, err
    assert K.identical(plain, cut)
    (gxy, ginf), cs, st = cut
    assert 0 < int(st.sum()) < K.N and st[140] == 0             # both verdicts occur
    for i in K.SAMPLE + (131, 140):
        want = V.prove_with(sks[i], V.pt_from_abi(pk[0][i], pk[1][i]), msgs[i], nonces[i])
        assert V.pt_from_abi(gxy[i], ginf[i]) == (want[0] if want else V.gamma_of(sks[i], msgs[i])), i
        assert int(st[i]) == (want is not None), i
        if want is None:
            assert not cs[i].any(), i
        else:
            assert (V.from_fe(cs[i][:12]), V.from_fe(cs[i][12:])) == want[1:], i
    assert ginf[131] == 1


@pytest.mark.parametrize("scheme", SCHEMES)
def test_proof_to_hash_in_three_slab_chunks(setups, scheme, monkeypatch, capfd):
    """EC-VRF proof_to_hash of 261 proofs of the device's prove, one spoilt row in each chunk: c (-pk) by the single launch
    and s mh + c (-gamma) by the joint launch, both in three chunks"""
    import slab_chunks as K
    V, D, _ = setups[scheme]
    sks, sk, pk, msgs, ma = _chunk_rows(V, D, scheme)
    rs = np.random.default_rng(261 + len(scheme))
    gxy, ginf, cs = np.zeros((K.N, 24), dtype=np.uint64), np.zeros(K.N, dtype=np.uint8), np.zeros((K.N, 24), dtype=np.uint64)
    todo = np.arange(K.N)
    for _ in range(64):                                         # about 32 % of the nonces pass both range checks
        (g_, gi_), c_, st = D.prove(sk[todo], (pk[0][todo], pk[1][todo]), ma[todo], _random_elems(rs, len(todo), V.r))
        ok = todo[st == 1]
        gxy[ok], ginf[ok], cs[ok] = g_[st == 1], gi_[st == 1], c_[st == 1]
        todo = todo[st != 1]
        if not len(todo):
            break
    assert not len(todo)
    K.assert_rows_differ([r.tobytes() for r in cs[:, :12]], [r.tobytes() for r in cs[:, 12:]], [r.tobytes() for r in gxy])
    expect = [1] * K.N
    cs[5, 12:] = V.fe((V.from_fe(cs[5, 12:]) + 1) % BOUND)      # s + 1
    ma2 = ma.copy()
    ma2[140, 0] = V.fe(msgs[140][0] + 1)                         # another message
    cs[258, :12] = V.fe((V.from_fe(cs[258, :12]) + 1) % BOUND)  # c + 1
    expect[5] = expect[140] = expect[258] = 0
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: D.proof_to_hash(pk, ma2, (gxy, ginf), cs))
    assert K.chunk_lines(err, "vb_single") == K.THREE and K.chunk_lines(err, "vb_joint") == K.THREE, err
    assert K.identical(plain, cut)
    out, st = cut
    assert [int(x) for x in st] == expect
    assert not out[[5, 140, 258]].any()
    for i in K.SAMPLE + (5, 131, 140, 258):
        proof = (V.pt_from_abi(gxy[i], ginf[i]), V.from_fe(cs[i][:12]), V.from_fe(cs[i][12:]))
        code, o = V.proof_to_hash(V.pt_from_abi(pk[0][i], pk[1][i]), [V.from_fe(ma2[i, 0])], proof)
        assert int(st[i]) == code, i
        if code == ecvrf_ref.OK:
            assert V.from_fe(out[i]) == o, i
