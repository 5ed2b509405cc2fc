"""The Pedersen hash and the Pedersen commitment on the device (include/ginger_hip_pedersen.h), against the Python
restatement tests/pedersen_ref.py, the device's gh_batch_mul and the literal bit loop on the device (table_bits 1)."""
import random

import numpy as np
import pytest

import pedersen_ref
import pyref
from schnorr_ref import mul

pytestmark = pytest.mark.gpu
CURVES = pedersen_ref.CURVES
TABLE_BITS = (1, 2, 4, 8)


def pts_abi(P, pts):
    xy = np.zeros((len(pts), 24), dtype=np.uint64)
    inf = np.zeros(len(pts), dtype=np.uint8)
    for i, Q in enumerate(pts):
        xy[i], inf[i] = P.pt_abi(Q)
    return xy, inf


def limbs(vals):
    return np.array([pyref.int_to_limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 12)


def points(P, xy, inf):
    return [P.pt_from_abi(xy[i], inf[i]) for i in range(len(inf))]


def proj_to_aff(P, row):
    X, Y, Z = (P.from_fe(row[12 * c:12 * c + 12]) for c in range(3))
    if Z == 0:
        return None
    zi = pow(Z, -1, P.p)
    return ((X * zi % P.p,), (Y * zi % P.p,))


def crh(P, table_bits):
    from ginger_lib_amd import pedersen
    xy, inf = pts_abi(P, P.flat())
    return pedersen.PedersenCRH(P.cname, xy, inf, P.num_windows, P.window_size, table_bits)


def commitment(P, table_bits):
    from ginger_lib_amd import pedersen
    xy, inf = pts_abi(P, P.flat())
    rxy, rinf = pts_abi(P, P.rand)
    return pedersen.PedersenCommitment(P.cname, xy, inf, P.num_windows, P.window_size, rxy, rinf, table_bits)


def rows_for(rs, n, nbytes):
    """random rows; from two rows on an all-zero and an all-ones row, then one row per single bit as far as n goes"""
    data = rs.integers(0, 256, size=(n, nbytes), dtype=np.uint8)
    if n >= 2 and nbytes:
        data[0], data[1] = 0, 0xFF
        for i in range(2, min(n, 2 + 8 * nbytes)):
            data[i] = 0
            data[i, (i - 2) // 8] = 1 << ((i - 2) % 8)
    return data


# ---------------------------------------------------------------- a. parity with the restatement
@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("wn", [(4, 5), (3, 7), (8, 4)])
def test_hash_matches_restatement(gpu, cname, wn):
    """G = 20 and 21: partial last groups at t = 8 and at t = 2, 4, 8; n = 1 (one lane), 17 (one more than a normalisation
    run), 300 (more than a block); every input length"""
    from ginger_lib_amd import pedersen
    W, N = wn
    P = pedersen_ref.make(cname, random.Random(10 * W + N + len(cname)), W, N, recipe=(W == 4))
    G = W * N
    rs = np.random.default_rng(W + N)
    cases = []
    for n in (1, 17, 300):
        for nbytes in (0, 1, G // 8):
            data = rows_for(rs, n, nbytes)
            cases.append((data, [P.evaluate(bytes(r.tolist())) for r in data]))
    for t in TABLE_BITS:
        D = crh(P, t)
        try:
            assert D.input_size_bits == G
            for data, want in cases:
                oxy, oinf = D.evaluate(data)
                got = points(P, oxy, oinf)
                assert got == want, (t, data.shape, [i for i in range(len(want)) if got[i] != want[i]][:8])
                if data.shape[1] == 0 or data.shape[0] >= 2:
                    assert oinf[0] == 1 and not oxy[0, :12].any()                # infinity as gh_bh_hash reports it: (0, 1)
                    assert P.from_fe(oxy[0, 12:]) == 1
            with pytest.raises(pedersen.GingerHipError, match="-1"):
                D.evaluate(np.zeros((1, G // 8 + 1), dtype=np.uint8))
        finally:
            D.close()


# ---------------------------------------------------------------- b. hostile generators
@pytest.mark.parametrize("cname", CURVES)
def test_hostile_generators_all_inputs(gpu, cname):
    """flat generators A A -A inf B -B A C.  At t = 2 the groups are {A, A} (equal inside a group), {-A, inf} (a generator at
    infinity; -A opposite to group 0 across groups: the accumulator passes through infinity and goes on), {B, -B} (an entry
    at infinity), {A, C} (equal across groups); at t = 4 {A, A, -A, inf} and {B, -B, A, C} hold every case inside a group
    and A / -A across; at t = 8 all are inside one group, at t = 1 all across (the accumulator doubles and cancels inside
    proj_madd).  All 256 inputs, every table_bits the same rows."""
    C = pyref.CURVES[cname]
    rng = random.Random(8 + len(cname))
    A, B, Cp = (pedersen_ref.random_point(C, rng) for _ in range(3))
    flat = [A, A, C.neg(A), None, B, C.neg(B), A, Cp]
    P = pedersen_ref.Pedersen(cname, [flat[:4], flat[4:]])
    data = np.arange(256, dtype=np.uint8).reshape(256, 1)
    want = [P.evaluate(bytes([v])) for v in range(256)]
    assert want[0b101] is None and want[0b110000] is None and want[0b1000101] == A and want[0b11] == C.add(A, A)
    first = None
    for t in TABLE_BITS:
        D = crh(P, t)
        try:
            oxy, oinf = D.evaluate(data)
        finally:
            D.close()
        got = points(P, oxy, oinf)
        assert got == want, (t, [i for i in range(256) if got[i] != want[i]][:8])
        if first is None:
            first = (oxy, oinf)
        assert np.array_equal(oxy, first[0]) and np.array_equal(oinf, first[1]), t


# ---------------------------------------------------------------- c. the commitment
@pytest.mark.parametrize("cname", CURVES)
def test_commit_is_evaluate_plus_r_h(gpu, cname):
    """recipe randomness generators h_k = 2^k H: commit == evaluate + r H, with r H by gh_batch_mul on every row and by the
    restatement's scalar multiplication on 8 rows"""
    from ginger_lib_amd import schnorr
    P = pedersen_ref.make(cname, random.Random(30 + len(cname)), 3, 7, recipe=True, commitment=True)
    C, H = P.C, P.rand[0]
    rng = random.Random(31 + len(cname))
    rs = [0, 1, 1 << 752, P.r - 1] + [rng.randrange(P.r) for _ in range(64)]
    n = len(rs)
    data = rows_for(np.random.default_rng(5), n, 2)
    rmont = limbs([P.R.to_mont(r) for r in rs])
    hxy, _ = pts_abi(P, [H])
    rH = [proj_to_aff(P, row) for row in schnorr.batch_mul(cname, np.repeat(hxy, n, axis=0), limbs(rs))]
    assert rH[0] is None and rH[1] == H
    first = None
    for t in TABLE_BITS:
        D = commitment(P, t)
        try:
            exy, einf = D.evaluate(data)
            cxy, cinf = D.commit(data, rmont)
        finally:
            D.close()
        ev, cm = points(P, exy, einf), points(P, cxy, cinf)
        for i in range(n):
            assert cm[i] == C.add(ev[i], rH[i]), (t, i)
        for i in list(range(4)) + [10, 20, 40, 67]:
            assert ev[i] == P.evaluate(bytes(data[i].tolist())), (t, i)
            assert cm[i] == C.add(ev[i], mul(C, rs[i], H)), (t, i)
        assert cm[0] == ev[0] and cinf[0] == einf[0] == 1                        # the zero row with r = 0
        if first is None:
            first = (cxy, cinf)
        assert np.array_equal(cxy, first[0]) and np.array_equal(cinf, first[1]), t


@pytest.mark.parametrize("cname", CURVES)
def test_commit_with_generators_of_no_recipe(gpu, cname):
    """randomness generators that are not each other's doubles, one of them at infinity: the literal loop"""
    from ginger_lib_amd import pedersen
    P = pedersen_ref.make(cname, random.Random(40 + len(cname)), 4, 5, recipe=False, commitment=True)
    P.rand[6] = None
    P.rand[752] = P.C.neg(P.rand[0])                                             # bits 0 and 752 cancel
    rng = random.Random(41 + len(cname))
    rs = [0, 1, (1 << 752) | 1, 1 << 6, P.r - 1] + [rng.randrange(P.r) for _ in range(7)]
    data = rows_for(np.random.default_rng(6), len(rs), 2)
    data[1], data[2], data[3] = 0, 0, 0
    want =[P.commit(bytes(d.tolist()), r) for d, r in zip(data, rs)]
    assert want[0] is None and want[2] is None and want[3] is None and want[1] == P.rand[0]
    rmont = limbs([P.R.to_mont(r) for r in rs])
    for t in TABLE_BITS:
        D = commitment(P, t)
        try:
            cxy, cinf = D.commit(data, rmont)
            assert points(P, cxy, cinf) == want, t
            bad = rmont.copy()
            bad[3] = pyref.int_to_limbs(P.r)
            with pytest.raises(pedersen.GingerHipError, match="-1"):
                D.commit(data, bad)
        finally:
            D.close()
    H = crh(P, 0)
    try:
        out = np.zeros((len(rs), 24), dtype=np.uint64), np.zeros(len(rs), dtype=np.uint8)
        rc = H._fn("commit")(H.handle, data.ctypes.data, len(rs), 2, rmont.ctypes.data, out[0].ctypes.data, out[1].ctypes.data)
        assert rc == -1                                                          # made without randomness generators
    finally:
        H.close()


@pytest.mark.parametrize("cname", CURVES)
def test_setup_recipe_through_batch_mul(gpu, cname):
    """generator_powers / create_generators: the reference's setup with the drawn bases as arguments"""
    from ginger_lib_amd import pedersen
    C = pyref.CURVES[cname]
    rng = random.Random(45 + len(cname))
    bases = [pedersen_ref.random_point(C, rng) for _ in range(3)]
    P = pedersen_ref.Pedersen(cname, pedersen_ref.recipe_generators(C, bases, 7))
    bxy, _ = pts_abi(P, bases)
    gxy, ginf = pedersen.create_generators(cname, bxy, 7)
    assert points(P, gxy, ginf) == P.flat()
    rxy, rinf = pedersen.generator_powers(cname, bxy[0], 753)
    got = points(P, rxy, rinf)
    assert got[:7] == P.gens[0] and got[752] == mul(C, 1 << 752, bases[0])


# ---------------------------------------------------------------- d. a working size
@pytest.mark.parametrize("cname", CURVES)
def test_one_field_element_1024_rows(gpu, cname):
    """(W, N) = (128, 6): one serialised field element of 96 bytes.  table_bits 8 and 4 equal table_bits 1, the literal loop
    on the device, on every row; 16 rows equal the restatement"""
    P = pedersen_ref.make(cname, random.Random(50 + len(cname)), 128, 6, recipe=False)
    n = 1024
    rs = np.random.default_rng(7 + len(cname))
    data = rs.integers(0, 256, size=(n, 96), dtype=np.uint8)
    data[0], data[1] = 0, 0xFF
    out = {}
    for t in (1, 4, 8):
        D = crh(P, t)
        try:
            out[t] = D.evaluate(data)
        finally:
            D.close()
    for t in (4, 8):
        assert np.array_equal(out[t][0], out[1][0]) and np.array_equal(out[t][1], out[1][1]), t
    oxy, oinf = out[8]
    for i in [0, 1, 2, 63, 64, 1023] + [int(x) for x in rs.choice(n, size=10, replace=False)]:
        assert P.pt_from_abi(oxy[i], oinf[i]) == P.evaluate(bytes(data[i].tolist())), i


# ---------------------------------------------------------------- e. the device-pointer entry points
@pytest.mark.parametrize("cname", CURVES)
def test_dev_entry_points_give_the_same_bytes(gpu, cname):
    from ginger_lib_amd import pedersen
    P = pedersen_ref.make(cname, random.Random(60 + len(cname)), 3, 7, recipe=False, commitment=True)
    n, nbytes = 70, 2
    data = rows_for(np.random.default_rng(8), n, nbytes)
    rng = random.Random(61)
    rmont = limbs([P.R.to_mont(rng.randrange(P.r)) for _ in range(n)])
    D = commitment(P, 0)
    bufs = [gpu.DeviceBuffer(n * nbytes).upload(data), gpu.DeviceBuffer(n * 96).upload(rmont), gpu.DeviceBuffer(n * 192), gpu.DeviceBuffer(n)]
    d_in, d_r, d_xy, d_inf = bufs
    try:
        exy, einf = D.evaluate(data)
        D.evaluate_dev(d_in, n, nbytes, d_xy, d_inf)
        assert np.array_equal(d_xy.download().reshape(n, 24), exy) and np.array_equal(d_inf.download(np.uint8), einf)
        assert points(P, exy[:3], einf[:3]) == [P.evaluate(bytes(r.tolist())) for r in data[:3]]
        cxy, cinf = D.commit(data, rmont)
        D.commit_dev(d_in, n, nbytes, d_r, d_xy, d_inf)
        assert np.array_equal(d_xy.download().reshape(n, 24), cxy) and np.array_equal(d_inf.download(np.uint8), cinf)
        assert not np.array_equal(cxy, exy)
        ms, total = pedersen.last_timing()
        assert set(ms) == set(pedersen.PHASES) and ms["hash"] > 0 and total > 0
    finally:
        for b in bufs:
            b.free()
        D.close()
