"""Field-based Schnorr and the batched variable-base scalar multiplication on the device (include/ginger_hip_schnorr.h),
against the host's gh_proj_mul, the device's fixed-base path and the Python restatement tests/schnorr_ref.py."""
import random

import numpy as np
import pytest

import poseidon_ref
import pyref
import schnorr_ref

pytestmark = pytest.mark.gpu
SCHEMES = list(schnorr_ref.SCHEMES)
BOUND = schnorr_ref.BOUND


@pytest.fixture(scope="module")
def refs():
    return {s: schnorr_ref.Schnorr(s) for s in SCHEMES}


@pytest.fixture(scope="module")
def schemes(gpu):
    from ginger_lib_amd import poseidon, schnorr
    out = {}
    for s, (tag, curve) in schnorr_ref.SCHEMES.items():
        prm = poseidon.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, tag)
        out[s] = schnorr.FieldBasedSchnorrSignatureScheme(prm, curve)
    yield out
    for v in out.values():
        v.close()


def limbs(vals):
    return np.array([pyref.int_to_limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 12)


def to_int(row):
    return pyref.limbs_to_int([int(v) for v in row])


def proj_eq(p, a, b):
    """projective ABI rows a, b (36 limbs) are the same point: cross products hold in the Montgomery form as well"""
    X1, Y1, Z1 = to_int(a[:12]), to_int(a[12:24]), to_int(a[24:36])
    X2, Y2, Z2 = to_int(b[:12]), to_int(b[12:24]), to_int(b[24:36])
    if Z1 == 0 or Z2 == 0:
        return Z1 == Z2
    return (X1 * Z2 - X2 * Z1) % p == 0 and (Y1 * Z2 - Y2 * Z1) % p == 0


def aff_row(S, P):
    xy, inf = S.pk_abi(P)
    return xy, inf


# ---------------------------------------------------------------- 1. gh_batch_mul
@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_mul_matches_host_and_restatement(gpu, refs, scheme):
    from ginger_lib_amd import schnorr
    S = refs[scheme]
    C, curve = S.C, schnorr_ref.SCHEMES[scheme][1]
    p, r = S.p, S.r
    rng = random.Random(11 + len(scheme))
    one = pyref.int_to_limbs(S.F.to_mont(1))
    base_pts = [S.G] + [schnorr_ref.mul(C, rng.randrange(1, r), S.G) for _ in range(7)]
    n = 512
    pts = [base_pts[i % len(base_pts)] for i in range(n)]
    ks = [rng.randrange(r) for _ in range(n)]
    ks[:6] = [0, 1, 2, r - 1, 3, rng.getrandbits(753) % r]
    infs = [0] * n
    infs[5] = 1                                               # a base at infinity
    xy = np.zeros((n, 24), dtype=np.uint64)
    for i, P in enumerate(pts):
        xy[i], _ = aff_row(S, P)
    out = schnorr.batch_mul(curve, xy, limbs(ks), np.array(infs, dtype=np.uint8))
    for i in range(n):
        xyz = np.concatenate([xy[i], np.array(one, dtype=np.uint64)])
        want = gpu.proj_mul(curve, xyz, limbs([ks[i]])[0])
        if infs[i]:
            assert to_int(out[i][24:]) == 0, i
            continue
        assert proj_eq(p, out[i], want), i
    # scalars r <= k < 2^753, which gh_proj_mul does not take: against the restatement
    big = [r, r + 1, (1 << 753) - 1, (1 << 753) - 2, r + rng.randrange(1 << 752)]
    big = [k for k in big if k < (1 << 753)]
    xy2 = np.array([aff_row(S, base_pts[j % 8])[0] for j in range(len(big))], dtype=np.uint64)
    out2 = schnorr.batch_mul(curve, xy2, limbs(big))
    for j, k in enumerate(big):
        P = schnorr_ref.mul(C, k, base_pts[j % 8])
        X, Y, Z = (S.from_fe(out2[j][12 * c:12 * c + 12]) for c in range(3))
        if P is None:
            assert Z == 0, k
        else:
            zi = pow(Z, -1, p)
            assert (X * zi % p, Y * zi % p) == (P[0][0], P[1][0]), k


@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_mul_matches_fixed_base_at_2p16(gpu, refs, scheme):
    from ginger_lib_amd import schnorr
    S = refs[scheme]
    curve = schnorr_ref.SCHEMES[scheme][1]
    n = 1 << 16
    rs = np.random.default_rng(5)
    k = rs.integers(0, 1 << 63, size=(n, 12), dtype=np.uint64) * 2 + rs.integers(0, 2, size=(n, 12), dtype=np.uint64)
    k[:, 11] &= (1 << 48) - 1                                 # below 2^752 < r
    k[0] = 0
    k[1] = 0
    k[1, 0] = 1
    P = schnorr_ref.mul(S.C, 12345, S.G)
    xy = np.tile(np.array(aff_row(S, P)[0], dtype=np.uint64), (n, 1))
    one = np.array(pyref.int_to_limbs(S.F.to_mont(1)), dtype=np.uint64)
    fb = gpu.FixedBaseMSM(curve, np.concatenate([xy[0], one]), scalar_size=753, window=12)
    try:
        want = fb.multi_scalar_mul(k)
    finally:
        fb.free()
    got = schnorr.batch_mul(curve, xy, k)
    bad = [i for i in range(n) if not proj_eq(S.p, got[i], want[i])]
    assert not bad, bad[:8]


# ---------------------------------------------------------------- 2. / 3. the scheme against the restatement
def _rows(S, rng, n_rows, L):
    out = []
    for i in range(n_rows):
        sk = rng.randrange(S.r)
        out.append((sk, S.pk(sk), [rng.randrange(S.p) for _ in range(L)]))
    return out


def _pk_arrays(S, pks):
    xy = np.zeros((len(pks), 24), dtype=np.uint64)
    inf = np.zeros(len(pks), dtype=np.uint8)
    for i, P in enumerate(pks):
        xy[i], inf[i] = S.pk_abi(P)
    return xy, inf


def _msg_arr(S, msgs, L):
    return np.array([[S.fe(x) for x in m] for m in msgs], dtype=np.uint64).reshape(len(msgs), L, 12)


def _sig_arr(S, sigs):
    return np.array([S.fe(e) + S.fe(s) for e, s in sigs], dtype=np.uint64).reshape(-1, 24)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("L", [0, 1, 2, 5])
def test_scheme_against_restatement(schemes, refs, scheme, L):
    S, D = refs[scheme], schemes[scheme]
    rng = random.Random(100 * L + len(scheme))
    n = 12
    rows = _rows(S, rng, n, L)
    sks = [sk for sk, _, _ in rows]
    pks = [pk for _, pk, _ in rows]
    msgs = [m for _, _, m in rows]
    # public keys
    xy, inf = D.get_public_key(limbs([S.R.to_mont(sk) for sk in sks]))
    exy, einf = _pk_arrays(S, pks)
    assert np.array_equal(xy, exy) and np.array_equal(inf, einf)
    assert D.keyverify((xy, inf)).all()
    # signing with the restatement's nonces: identical words, and status 0 exactly where the restatement rejects
    nonces = [rng.randrange(S.r) for _ in range(n)]
    nonces[0] = 0
    want = [S.sign_with(sk, pk, m, k) for sk, pk, m, k in zip(sks, pks, msgs, nonces)]
    sig, st = D.sign(limbs([S.R.to_mont(x) for x in sks]), (xy, inf), _msg_arr(S, msgs, L), limbs([S.R.to_mont(k) for k in nonces]))
    assert [int(x) for x in st] == [0 if w is None else 1 for w in want]
    for i, w in enumerate(want):
        if w is None:
            assert not sig[i].any()
        else:
            assert [S.from_fe(sig[i][:12]), S.from_fe(sig[i][12:])] == list(w), i
    # verification: the restatement's valid signatures
    good = [S.sign(sk, pk, m, rng) for sk, pk, m in rows]
    sg = _sig_arr(S, good)
    ma = _msg_arr(S, msgs, L)
    assert list(D.verify((xy, inf), ma, sg)) == [1] * n
    # another message, changed e or s, another key -> 0; e or s >= 2^752 -> 2
    bad_sigs = list(good)
    expect = [1] * n
    for i in range(n):
        e, s = good[i]
        kind = i % 5
        if kind == 1:
            bad_sigs[i] = ((e + 1) % BOUND, s)
        elif kind == 2:
            bad_sigs[i] = (e, (s + 1) % BOUND)
        elif kind == 3:
            bad_sigs[i] = (BOUND + e % (S.p - BOUND), s)         # in [2^752, p): a field element the reference rejects
        elif kind == 4:
            bad_sigs[i] = (e, BOUND + s % (S.p - BOUND))
        expect[i] = [1, 0, 0, 2, 2][kind]
    st = D.verify((xy, inf), ma, _sig_arr(S, bad_sigs))
    assert [int(x) for x in st] == expect
    assert [S.verify(pk, m, sg_) for pk, m, sg_ in zip(pks[:5], msgs[:5], bad_sigs[:5])] == [True, False, False, None, None]
    if L:
        msgs2 = [list(m) for m in msgs]
        for m in msgs2:
            m[-1] = (m[-1] + 1) % S.p
        assert list(D.verify((xy, inf), _msg_arr(S, msgs2, L), sg)) == [0] * n
    rot = np.roll(np.arange(n), 1)
    assert list(D.verify((xy[rot], inf[rot]), ma, sg)) == [0] * n


@pytest.mark.parametrize("scheme", SCHEMES)
def test_edge_cases(schemes, refs, scheme):
    S, D = refs[scheme], schemes[scheme]
    rng = random.Random(77 + len(scheme))
    L = 1
    # R' = infinity: e = H(m || 0 || 1 || pk.x), s = e sk mod r
    sk = rng.randrange(S.r)
    pk = S.pk(sk)
    while True:
        m = [rng.randrange(S.p)]
        e = S.H.evaluate(m + [0, 1, pk[0][0]])
        s = e * sk % S.r
        if e < BOUND and s < BOUND:
            break
    assert S.verify(pk, m, (e, s)) is True
    # PK = infinity (sk = 0): signs and verifies, keyverify 1
    xy0, inf0 = D.get_public_key(limbs([0]))
    assert inf0[0] == 1 and D.keyverify((xy0, inf0))[0]
    m0 = [rng.randrange(S.p)]
    while True:
        k = rng.randrange(1, S.r)
        w = S.sign_with(0, None, m0, k)
        if w:
            break
    sig0, st0 = D.sign(limbs([0]), (xy0, inf0), _msg_arr(S, [m0], 1), limbs([S.R.to_mont(k)]))
    assert st0[0] == 1 and [S.from_fe(sig0[0][:12]), S.from_fe(sig0[0][12:])] == list(w)
    assert S.verify(None, m0, w) is True
    xy, inf = _pk_arrays(S, [pk, None])
    st = D.verify((xy, inf), _msg_arr(S, [m, m0], L), _sig_arr(S, [(e, s), w]))
    assert list(st) == [1, 1]
    # an off-curve key
    bad = xy.copy()
    bad[0, 12:] = S.fe(pk[1][0] + 1)
    assert list(D.keyverify((bad, np.zeros(2, dtype=np.uint8)))) == [False, False]     # row 1: (0, 0) without the flag


@pytest.mark.parametrize("scheme", SCHEMES)
def test_non_canonical_input_is_rejected(schemes, refs, scheme):
    from ginger_lib_amd import schnorr
    S, D = refs[scheme], schemes[scheme]
    xy, inf = _pk_arrays(S, [S.G])
    sig = np.zeros((1, 24), dtype=np.uint64)
    msg = np.zeros((1, 1, 12), dtype=np.uint64)
    msg[0, 0] = pyref.int_to_limbs(S.p)
    with pytest.raises(schnorr.GingerHipError, match="-1"):
        D.verify((xy, inf), msg, sig)
    sig[0, 12:] = pyref.int_to_limbs(S.p)
    with pytest.raises(schnorr.GingerHipError, match="-1"):
        D.verify((xy, inf), np.zeros((1, 1, 12), dtype=np.uint64), sig)
    with pytest.raises(schnorr.GingerHipError, match="-1"):
        D.get_public_key(limbs([S.r]))


# ---------------------------------------------------------------- 4. 2^18 rows, device only
def _random_elems(rs, n, p):
    a = rs.integers(0, 1 << 63, size=(n, 12), dtype=np.uint64) * 2 + rs.integers(0, 2, size=(n, 12), dtype=np.uint64)
    a[:, 11] = a[:, 11] % np.uint64(p >> (64 * 11))           # below p's top limb: below p
    return a


@pytest.mark.parametrize("scheme", SCHEMES)
def test_device_round_trip_2p18(schemes, refs, scheme):
    S, D = refs[scheme], schemes[scheme]
    n = 1 << 18
    rs = np.random.default_rng(18 + len(scheme))
    sk = _random_elems(rs, n, S.r)
    msg = _random_elems(rs, n, S.p).reshape(n, 1, 12)
    xy, inf = D.get_public_key(sk)
    assert D.keyverify((xy, inf)).all()
    sig = np.zeros((n, 24), dtype=np.uint64)
    todo = np.arange(n)
    for _ in range(40):
        s_, st = D.sign(sk[todo], (xy[todo], inf[todo]), msg[todo], _random_elems(rs, len(todo), S.r))
        sig[todo[st == 1]] = s_[st == 1]
        todo = todo[st != 1]
        if not len(todo):
            break
    assert not len(todo)
    assert (D.verify((xy, inf), msg, sig) == 1).all()
    # flip one bit in 1 % of the rows (message or signature words, kept below the modulus)
    flip = rs.choice(n, size=n // 100, replace=False)
    msg2, sig2 = msg.copy(), sig.copy()
    for j, i in enumerate(flip):
        tgt = (msg2[i, 0], sig2[i, :12], sig2[i, 12:])[j % 3]
        tgt[j % 11] ^= np.uint64(1 << (j % 64))
        assert to_int(tgt) < S.p
    st = D.verify((xy, inf), msg2, sig2)
    assert set(np.nonzero(st != 1)[0].tolist()) == set(flip.tolist())
    # 16 sampled rows agree with the restatement
    for i in rs.choice(n, size=16, replace=False):
        pk = None if inf[i] else ((S.from_fe(xy[i][:12]),), (S.from_fe(xy[i][12:]),))
        assert pk == S.pk(S.R.from_mont(to_int(sk[i])))
        m = [S.from_fe(msg2[i, 0])]
        sg = (S.from_fe(sig2[i][:12]), S.from_fe(sig2[i][12:]))
        want = S.verify(pk, m, sg)
        assert int(st[i]) == {True: 1, False: 0, None: 2}[want], i


# ---------------------------------------------------------------- the windows of GH_SCHNORR_WINDOW, the generator table's rebuild
_WINDOW_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from __graft_entry__ import _load_pkg
gl = _load_pkg(); gl.init()
from ginger_lib_amd import schnorr
import pyref, schnorr_ref
rng = np.random.default_rng(int(sys.argv[2]))
bad = 0
for scheme, (tag, curve) in schnorr_ref.SCHEMES.items():
    S = schnorr_ref.Schnorr(scheme)
    P = schnorr_ref.mul(S.C, 777, S.G)
    xy = np.tile(np.array(S.pk_abi(P)[0], dtype=np.uint64), (64, 1))
    ks = [int(rng.integers(0, 1 << 62)) << 690 | int(rng.integers(0, 1 << 62)) for _ in range(62)] + [0, (1 << 753) - 1]
    out = schnorr.batch_mul(curve, xy, np.array([pyref.int_to_limbs(k) for k in ks], dtype=np.uint64))
    for row, k in zip(out, ks):
        X, Y, Z = (S.from_fe(row[12 * c:12 * c + 12]) for c in range(3))
        Q = schnorr_ref.mul(S.C, k, P)
        if Q is None:
            bad += Z != 0
        else:
            zi = pow(Z, -1, S.p)
            bad += (X * zi % S.p, Y * zi % S.p) != (Q[0][0], Q[1][0])
print("BAD", bad)
'''


@pytest.mark.parametrize("w", ["4", "5", "6"])
def test_every_window_of_the_knob_is_correct(gpu, w):
    """GH_SCHNORR_WINDOW = 4, 5, 6 each run their own kernels (the knob is read once per process: a child per window)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _WINDOW_CHILD, root, w], env=dict(os.environ, GH_SCHNORR_WINDOW=w),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "BAD 0" in p.stdout, p.stdout[-2000:]


def test_generator_table_follows_the_batch_size(gpu, refs):
    """a handle first used on one row (a small fixed-base window) still computes larger batches right after its rebuild"""
    from ginger_lib_amd import poseidon, schnorr
    S = refs["SchnorrMNT6"]
    prm = poseidon.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, "mnt6753")
    D = schnorr.FieldBasedSchnorrSignatureScheme(prm, "mnt4753_g1")
    try:
        rng = random.Random(4)
        sks = [rng.randrange(S.r) for _ in range(3000)]
        xy1, inf1 = D.get_public_key(limbs([S.R.to_mont(sks[0])]))
        xy, inf = D.get_public_key(limbs([S.R.to_mont(k) for k in sks]))
        assert np.array_equal(xy[0], xy1[0]) and not inf.any()
        for i in (0, 1, 1234, 2999):
            assert (S.from_fe(xy[i][:12]), S.from_fe(xy[i][12:])) == (S.pk(sks[i])[0][0], S.pk(sks[i])[1][0])
        assert D.keyverify((xy, inf)).all()
    finally:
        D.close()
        prm.close()


# ---------------------------------------------------------------- the chunks after the first (tests/slab_chunks.py)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_mul_in_three_slab_chunks(gpu, refs, scheme, monkeypatch, capfd):
    """gh_batch_mul of 261 rows in chunks of 128, 128 and 5 rows: the chunk line, the same bits as in one chunk, and the
    restatement's points at both sides of every chunk edge and in the special rows, which sit in the later chunks only"""
    from ginger_lib_amd import schnorr
    import slab_chunks as K
    S = refs[scheme]
    C, curve = S.C, schnorr_ref.SCHEMES[scheme][1]
    rng = random.Random(261 + len(scheme))
    P = schnorr_ref.mul(C, rng.randrange(1, S.r), S.G)
    pts = []
    for _ in range(K.N):                                      # P + i G: a base of its own in every row
        pts.append(P)
        P = C.add(P, S.G)
    ks = [rng.getrandbits(753) for _ in range(K.N)]
    K.assert_rows_differ(pts, ks)
    top = (1 << 753) - 1
    pts[131] = None                                           # rows 3 and 259, 12 and 268, ... are ordinary rows
    ks[140], ks[150], ks[258] = 0, top, 0
    xy, inf = _pk_arrays(S, pts)
    k = limbs(ks)
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: schnorr.batch_mul(curve, xy, k, inf))
    assert K.chunk_lines(err, "vb_single") == K.THREE, err
    assert K.identical(plain, cut)
    for i in K.SAMPLE + (131, 140, 150, 258):
        want = schnorr_ref.mul(C, ks[i], pts[i])
        X, Y, Z = (S.from_fe(cut[i][12 * c:12 * c + 12]) for c in range(3))
        if want is None:
            assert Z == 0 and i in (131, 140, 258), i
        else:
            zi = pow(Z, -1, S.p)
            assert (X * zi % S.p, Y * zi % S.p) == (want[0][0], want[1][0]), i


@pytest.mark.parametrize("scheme", SCHEMES)
def test_verify_in_three_slab_chunks(schemes, refs, scheme, monkeypatch, capfd):
    """Schnorr verify of the restatement's 261 signatures (tests/golden/schnorr_chunk_rows.json, written by
    tests/golden/gen_schnorr_chunk_rows.py) with one spoilt row in each chunk"""
    import json
    import os
    import slab_chunks as K
    S, D = refs[scheme], schemes[scheme]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schnorr_chunk_rows.json")) as f:
        rows = json.load(f)[scheme]
    sk0, m0, m_step = (int(rows[x], 16) for x in ("sk0", "m0", "m_step"))
    sigs = [(int(e, 16), int(s, 16)) for e, s in rows["sigs"]]
    nonces = [int(x, 16) for x in rows["nonces"]]
    msgs = [[(m0 + i * m_step) % S.p] for i in range(K.N)]
    pk, pks = S.pk(sk0), []
    for _ in range(K.N):
        pks.append(pk)
        pk = S.C.add(pk, S.G)
    assert pks[260] == S.pk(sk0 + 260)
    K.assert_rows_differ(pks, [m[0] for m in msgs], [e for e, _ in sigs], [s for _, s in sigs], nonces)
    for i in (0, 260):                                        # the file holds what the restatement signs
        assert S.sign_with(sk0 + i, pks[i], msgs[i], nonces[i]) == sigs[i], i
    expect = [1] * K.N
    e, s = sigs[5]
    sigs[5] = (e, (s + 1) % BOUND)
    msgs[140] = [(msgs[140][0] + 1) % S.p]
    e, s = sigs[258]
    sigs[258] = ((e + 1) % BOUND, s)
    expect[5] = expect[140] = expect[258] = 0
    pka, ma, sg = _pk_arrays(S, pks), _msg_arr(S, msgs, 1), _sig_arr(S, sigs)
    plain, cut, err = K.plain_and_cut(monkeypatch, capfd, lambda: D.verify(pka, ma, sg))
    assert K.chunk_lines(err, "vb_single") == K.THREE, err
    assert K.identical(plain, cut)
    assert [int(x) for x in cut] == expect
    for i in K.SAMPLE + (5, 140, 258):
        assert {True: 1, False: 0, None: 2}[S.verify(pks[i], msgs[i], sigs[i])] == int(cut[i]), i
