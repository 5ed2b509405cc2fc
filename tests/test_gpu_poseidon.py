"""Device Poseidon (include/ginger_hip_poseidon.h) against the Python restatement (tests/poseidon_ref.py)."""
import random

import numpy as np
import pytest

import poseidon_ref

pytestmark = pytest.mark.gpu
TAGS = ["mnt4753", "mnt6753"]


@pytest.fixture(scope="module")
def pos(gpu):
    from ginger_lib_amd import poseidon
    yield poseidon
    poseidon.set_tuning(0, None)


@pytest.fixture(scope="module")
def sets(pos):
    return {t: (poseidon_ref.Poseidon(t), pos.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, t)) for t in TAGS}


def rows(R, vals):
    return np.array([R.to_abi(v) for v in vals], dtype=np.uint64).reshape(-1, 12)


def ints(R, arr):
    return [R.from_abi(r) for r in np.asarray(arr).reshape(-1, 12)]


@pytest.mark.parametrize("tag", TAGS)
def test_permute_zero_is_after_zero_perm(pos, sets, tag):
    R, prm = sets[tag]
    out = prm.permute(np.zeros((1, 3, 12), dtype=np.uint64))
    assert np.array_equal(out.reshape(3, 12), prm.after_zero_perm)
    assert ints(R, out) == R.azp


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_evaluate_many_every_k(pos, sets, tag, k):
    R, prm = sets[tag]
    H = pos.PoseidonHash(prm)
    rng = random.Random(k * 7 + len(tag))
    pos.set_tuning(k, None)
    try:
        for ln in (0, 1, 2, 3, 4, 7):
            for n in (1, 63, 64, 65, 3001):
                if ln >= 4 and n == 3001:
                    n = 700                  # the restatement is the slow side
                vals = [[rng.randrange(R.p) for _ in range(ln)] for _ in range(n)]
                out = ints(R, H.evaluate_many(rows(R, [x for v in vals for x in v]).reshape(n, ln, 12)))
                idx = range(n) if n <= 65 else rng.sample(range(n), 40) + [0, n - 1]
                for i in idx:
                    assert out[i] == R.evaluate(vals[i]), (ln, n, i)
    finally:
        pos.set_tuning(0, None)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_evaluate_many_reproduces_the_reference_phantom_merkle_root(pos, sets, k):
    """the one hash answer the reference ships (MNT4753_PHANTOM_MERKLE_ROOT: the hash of ONE element), word for word, with the
    element in rows 0, 63 and 64 of a batch of 65 single-element inputs"""
    tag, x, words = poseidon_ref.phantom_root_kat()
    R, prm = sets[tag]
    rng = random.Random(5 + k)
    vals = [rng.randrange(R.p) for _ in range(65)]
    at = (0, 63, 64)
    for i in at:
        vals[i] = x
    pos.set_tuning(k, None)
    try:
        out = pos.PoseidonHash(prm).evaluate_many(rows(R, vals).reshape(65, 1, 12)).reshape(65, 12)
    finally:
        pos.set_tuning(0, None)
    for i in at:
        assert [int(w) for w in out[i]] == words, (k, i)
    for i in (1, 62):
        assert R.from_abi(out[i]) == R.evaluate([vals[i]]), (k, i)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_zero_sbox_inputs_inside_a_batch_and_last(pos, sets, tag, k):
    """states whose first-round S-box inputs are zero (one, two, all three elements) among random ones and as the last"""
    R, prm = sets[tag]
    p = R.p
    rng = random.Random(99 + k)
    neg = [(-R.rc[e]) % p for e in range(3)]
    r = lambda: rng.randrange(p)
    crafted = [[neg[0], r(), r()], [r(), neg[1], r()], [r(), r(), neg[2]], [neg[0], neg[1], r()], neg[:], [0, 0, 0], [p - 1, 1, 0]]
    n = 300
    states = [[r(), r(), r()] for _ in range(n)]
    for j, c in enumerate(crafted):
        states[17 + 37 * j] = c
    states[-1] = neg[:]
    pos.set_tuning(k, None)
    try:
        out = prm.permute(rows(R, [x for s in states for x in s]).reshape(n, 3, 12))
    finally:
        pos.set_tuning(0, None)
    got = ints(R, out)
    for i in [17 + 37 * j for j in range(len(crafted))] + [n - 1, 0, 1, n - 2]:
        assert got[3 * i:3 * i + 3] == R.perm(states[i]), i
    # a pair input that makes the first-round S-box inputs of the capacity element zero: the hash path through absorb()
    H = pos.PoseidonHash(prm)
    a, b = (neg[0] - R.azp[0]) % p, (neg[1] - R.azp[1]) % p
    vals = [[r(), r()] for _ in range(130)]
    vals[64], vals[-1] = [a, b], [a, r()]
    out = ints(R, H.evaluate_many(rows(R, [x for v in vals for x in v]).reshape(130, 2, 12)))
    for i in (63, 64, 65, 129):
        assert out[i] == R.evaluate(vals[i])


@pytest.mark.parametrize("tag", TAGS)
def test_multi_pass_batch_at_k1(pos, sets, tag):
    """n above K x (lanes of one pass = CUs x 512) at K = 1: the kernel walks the batch in several passes"""
    R, prm = sets[tag]
    n = 300_000                                     # > 256 CUs x 512 = 131 072 lanes: three passes at K = 1
    rng = np.random.default_rng(17)
    pairs = rng.integers(0, 1 << 63, size=(n, 2, 12), dtype=np.uint64)
    pairs[:, :, 11] &= (1 << 40) - 1
    H = pos.PoseidonHash(prm)
    pos.set_tuning(1, None)
    try:
        k1 = H.evaluate_many(pairs)
    finally:
        pos.set_tuning(0, None)
    pos.set_tuning(8, None)
    try:
        k8 = H.evaluate_many(pairs)
    finally:
        pos.set_tuning(0, None)
    assert np.array_equal(k1, k8)
    for i in [0, 131_071, 131_072, 131_073, 262_143, 262_144, n - 1] + random.Random(2).sample(range(n), 24):
        assert R.from_abi(k1[i]) == R.evaluate([R.from_abi(pairs[i, 0]), R.from_abi(pairs[i, 1])]), i


@pytest.mark.parametrize("tag", TAGS)
def test_batch_evaluate_2_1(pos, sets, tag):
    R, prm = sets[tag]
    rng = np.random.default_rng(5)
    n = 1 << 16
    vals = [int(x) % R.p for x in rng.integers(0, 1 << 62, size=2 * n)]
    vals = [(v * 0x9E3779B97F4A7C15 ** 11) % R.p for v in vals]
    arr = rows(R, vals)
    pairs = arr.reshape(n, 2, 12).copy()
    pos.PoseidonBatchHash(prm).batch_evaluate_2_1(arr)
    assert np.array_equal(arr[:n], pos.PoseidonHash(prm).evaluate_many(pairs))
    assert np.array_equal(arr[n:], rows(R, vals[n:]))          # the second half is left as it was
    for i in list(range(0, n, 4099)) + [n - 1]:
        assert R.from_abi(arr[i]) == R.evaluate([vals[2 * i], vals[2 * i + 1]])


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("tail", [0, 1 << 40])
def test_trees_against_restatement(pos, sets, tag, tail):
    R, prm = sets[tag]
    rng = random.Random(3 + tail % 7)
    pos.set_tuning(0, tail)
    try:
        for n in (0, 1, 2, 3, 5, 16, 17, 32, 1000):
            leaves = [rng.randrange(R.p) for _ in range(n)]
            L = 1
            while L < n:
                L *= 2
            th = L.bit_length()
            for height in sorted({th, th + 1, 12} if th <= 12 else {th}):
                t = pos.FieldBasedMerkleHashTree(prm, height, rows(R, leaves))
                want_tree, want_pad, want_root = R.tree(leaves, height)
                assert ints(R, t.tree) == want_tree, (n, height)
                assert ints(R, t.padding) == want_pad, (n, height)
                assert R.from_abi(t.root()) == want_root
                assert np.array_equal(t.leaves()[:n], rows(R, leaves))
                if height < 2:
                    continue
                root = t.root()
                paths = [t.generate_proof(i, t.leaves()[i]) for i in range(max(n, 1))]
                lv = t.leaves()[:max(n, 1)]
                assert pos.verify_paths(prm, lv, paths, root).all()
                bad_root = root.copy()
                bad_root[0] ^= 1
                assert not pos.verify_paths(prm, lv, paths, bad_root).any()
                flipped = pos.FieldBasedMerkleTreePath(paths[0].siblings.copy(), paths[0].directions)
                flipped.siblings[0, 0] ^= 2
                assert not flipped.verify(prm, root, lv[0])
            if th > 1:
                with pytest.raises(Exception):
                    pos.FieldBasedMerkleHashTree(prm, th - 1, rows(R, leaves))
    finally:
        pos.set_tuning(0, None)


def test_tree_too_short_is_bad_arg(pos, sets):
    import ctypes
    R, prm = sets["mnt4753"]
    lib = pos._lib()
    x = np.zeros((5, 12), dtype=np.uint64)
    root = np.zeros(12, dtype=np.uint64)
    assert lib.gh_poseidon_merkle_tree(prm.handle, x.ctypes.data_as(ctypes.c_void_p), 5, 3, None, None,
                                       root.ctypes.data_as(ctypes.c_void_p)) == -1


@pytest.mark.parametrize("tag", ["mnt4753"])
def test_tree_2p20(pos, sets, tag):
    R, prm = sets[tag]
    n = 1 << 20
    rng = np.random.default_rng(11)
    leaves = rng.integers(0, 1 << 63, size=(n, 12), dtype=np.uint64)
    leaves[:, 11] &= (1 << 40) - 1                        # below p, so every row is a valid Montgomery word
    height = 22
    t = pos.FieldBasedMerkleHashTree(prm, height, leaves)
    H = pos.PoseidonHash(prm)
    # the root rebuilt level by level through gh_poseidon_hash
    lvl = leaves
    while lvl.shape[0] > 1:
        lvl = H.evaluate_many(lvl.reshape(-1, 2, 12))
    cur = lvl[0]
    empty = R.to_abi(R.empty())
    for _ in range(height - 21):
        cur = H.evaluate_many(np.stack([cur, np.array(empty, dtype=np.uint64)]).reshape(1, 2, 12))[0]
    assert np.array_equal(cur, t.root())
    # 512 sampled internal nodes and the top 10 levels against the restatement
    tr = t.tree
    rs = random.Random(1)
    for i in rs.sample(range(n - 1), 512) + list(range(0, (1 << 10) - 1)):
        assert R.from_abi(tr[i]) == R.evaluate([R.from_abi(tr[2 * i + 1]), R.from_abi(tr[2 * i + 2])]), i
    # 4096 batched path verifications
    idx = rs.sample(range(n), 4096)
    paths = [t.generate_proof(i, tr[n - 1 + i]) for i in idx]
    assert pos.verify_paths(prm, tr[[n - 1 + i for i in idx]], paths, t.root()).all()
