"""The persistent form of the G1 bucket accumulation kernel (asmgen/g1_xyzz.py build(persistent=True): one wave per workgroup,
tiles of 64 tasks drawn from a counter) in asmgen/sim.py -- no GPU.  Waves run one after another over shared memory, so
the first wave of a grid draws every tile and the others find the counter spent: exactly the case "a wave that starts late".

Per prime one task table of 7 tiles (6 x 64 + 17 tasks) whose first tile holds the cases the group law branches on (empty list,
P - P, P + P through either salt, a sum that returns to infinity and restarts); every bucket is checked against the textbook law
(tests/pyref.py) and, word for word, against the block kernel's output on the same table.
"""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ginger-lib_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyref                                                      # noqa: E402
from asmgen import g1_xyzz                                        # noqa: E402
from asmgen.field import limbs, unlimbs                           # noqa: E402
from asmgen.isa import hazard_scan                                # noqa: E402
from asmgen.sim import Memory, Wave                               # noqa: E402

R = 1 << 754
CURVES = ["mnt4753_g1", "mnt6753_g1"]
N_FULL = 6 * 64 + 17            # 7 tiles, the last with 17 live tasks
N_SMALL = 64 + 17               # 2 tiles
SPECIAL = [
    [],                                              # cnt = 0 -> infinity
    [(5, 0)],
    [(5, 0), (5, 0)],                                # P + P: the detour through a salt point
    [(5, 0), (5, 1)],                                # P - P -> infinity
    [(5, 0), (5, 1), (7, 0)],                        # ... and a restart from infinity
    [(0, 0), (0, 0)],                                # G + G: the salt must be 2G
    [(1, 0), (1, 0), (3, 1)],                        # 2G + 2G: the salt must be G
    [(6, 0), (7, 0), (6, 1), (7, 1), (9, 0)],        # returns to infinity after four entries, then restarts
    [],
]
_CACHE = {}


def _setup(cname):
    """kernels, points, lists, expected sums and the block kernel's output words: computed once per curve, never changed"""
    if cname in _CACHE:
        return _CACHE[cname]
    C = pyref.CURVES[cname]
    p = C.F.p
    rnd = random.Random(23 + len(cname))
    h = C.mul(rnd.randrange(1, 1 << 60), C.G)
    pts = [C.G, C.add(C.G, C.G)]
    pt = C.mul(rnd.randrange(1, 1 << 60), C.G)
    for _ in range(30):
        pts.append(pt)
        pt = C.add(pt, h)
    lists = []
    for t in range(N_FULL):
        if t < len(SPECIAL):
            lists.append(SPECIAL[t])
        else:       # short lists: a tile costs its longest list
            lists.append([(rnd.randrange(len(pts)), rnd.randrange(2)) for _ in range(2 if t % 7 == 0 else 1)])
    lists[N_FULL - 1] = [(8, 0), (8, 0)]             # the last live lane of the ragged tile doubles
    expect = []
    for l in lists:
        e = None
        for (i, s) in l:
            e = C.add(e, C.neg(pts[i]) if s else pts[i])
        expect.append(e)
    st = dict(C=C, p=p, pts=pts, lists=lists, expect=expect,
              pw=g1_xyzz.build("acc_pw_" + cname, p, R % p, persistent=True),
              blk=g1_xyzz.build("acc_" + cname, p, R % p))
    st["block_out"] = _launch_block(st, N_FULL)
    st["block_out"].setflags(write=False)
    _CACHE[cname] = st
    return st


def _memory(st, nt, stamps_at=None, budget=0, mem=None):
    """-> (mem, kernarg address); the first nt tasks; the counter sits 16 bytes behind the task table as on the device.
    stamps_at: kernarg word of the pointer to a side buffer of two stamp records (the diagnostic kernels)"""
    C, p, r = st["C"], st["p"], R % st["p"]

    def enc(pt):
        return limbs(pt[0][0] * r % p) + limbs(pt[1][0] * r % p)
    mem = Memory() if mem is None else mem                           # the card runner passes one at device addresses
    a_bases = mem.add("bases", np.array([enc(pt) for pt in st["pts"]], dtype=np.uint32))
    sorted_l, tasks = [], []
    for l in st["lists"][:nt]:
        tasks.append((len(sorted_l), len(l)))
        sorted_l += [i | (s << 31) for (i, s) in l]
    a_sorted = mem.add("sorted", np.array(sorted_l + [0], dtype=np.uint32))
    a_out = mem.add("out", np.zeros((nt, 78), dtype=np.uint32), writable=True)
    tk = np.zeros((nt + 1, 4), dtype=np.uint32)                      # + the counter's 16 bytes
    for t, (b, c) in enumerate(tasks):
        d = a_out + t * 312
        tk[t] = (b, c, d & 0xFFFFFFFF, d >> 32)
    a_tasks = mem.add("tasks", tk, writable=True)
    a_salts = mem.add("salts", np.array([enc(C.G), enc(C.add(C.G, C.G))], dtype=np.uint32))
    a_ctr = a_tasks + nt * 16
    karg = np.zeros(16, dtype=np.uint32)
    for j, a in enumerate((a_bases, a_sorted, a_tasks, a_salts)):
        karg[2 * j], karg[2 * j + 1] = a & 0xFFFFFFFF, a >> 32
    karg[8], karg[9] = nt, (nt + 63) // 64
    karg[10], karg[11] = a_ctr & 0xFFFFFFFF, a_ctr >> 32
    karg[12] = budget                                                # persistent form: tiles per wave (0 = no limit)
    if stamps_at is not None:
        a_st = mem.add("stamps", np.zeros(2 * 16, dtype=np.uint32), writable=True)
        karg[stamps_at], karg[stamps_at + 1] = a_st & 0xFFFFFFFF, a_st >> 32
    return mem, mem.add("karg", karg)


def _wave(g, mem, a_karg, wg, tid0):
    w = Wave(g, mem, lds_words=g.lds_bytes // 4, strict=True)
    w.S[0], w.S[1], w.S[2] = a_karg & 0xFFFFFFFF, a_karg >> 32, wg
    w.V[0] = np.arange(64, dtype=np.uint32) + tid0
    w.lds[:] = 0xDEADBEEF
    w.run()
    return w


def _launch_block(st, nt):
    mem, a_karg = _memory(st, nt)
    for blk in range((nt + 255) // 256):
        for wv in range(4):
            if blk * 256 + wv * 64 < nt:
                _wave(st["blk"], mem, a_karg, blk, 64 * wv)
    return mem.get("out").reshape(nt, 78).copy()


def _launch_pw(st, mem, a_karg, waves, g=None):
    """-> per wave: the stores it made (the counter's add is one)"""
    stores = []
    for wg in range(waves):
        before = mem.stores
        _wave(g or st["pw"], mem, a_karg, wg, 0)
        stores.append(mem.stores - before)
    return stores


def _counter(mem, nt):
    return int(mem.get("tasks")[nt * 4])


def _check_law(st, out, nt):
    C, p = st["C"], st["p"]
    ri = pow(R % p, -1, p)
    for t in range(nt):
        xyz = [unlimbs(out[t, 26 * k:26 * k + 26]) for k in range(3)]
        assert max(xyz) < p, "unreduced output"
        X, Y, Z = (v * ri % p for v in xyz)
        exp = st["expect"][t]
        assert C.proj_to_affine((X,), (Y,), (Z,)) == exp, (t, st["lists"][t])
        if exp is None:
            assert (X, Y, Z) == (0, 1, 0)


@pytest.mark.parametrize("cname", CURVES)
def test_seven_tiles_for_three_waves_with_a_ragged_last_tile(cname):
    st = _setup(cname)
    _check_law(st, st["block_out"], N_FULL)                          # the reference of the word-for-word comparison is itself right
    mem, a_karg = _memory(st, N_FULL)
    stores = _launch_pw(st, mem, a_karg, 3)
    out = mem.get("out").reshape(N_FULL, 78)
    _check_law(st, out, N_FULL)
    assert np.array_equal(out, st["block_out"])
    # 39 dwordx2 stores per live lane and one draw per tile + the draw that found the counter spent; the late waves: that draw only
    assert stores == [N_FULL * 39 + 8, 1, 1]
    assert _counter(mem, N_FULL) == 7 + 3
    g = st["pw"]
    assert g.max_v == 256 and g.max_s <= 102 and g.max_a < 0 and g.lds_bytes == 19968
    assert hazard_scan(g, False)[0] == []


def test_a_tile_budget_spreads_the_tiles_over_the_waves():
    """budget 2: a wave ends after two tiles; 7 tiles for 4 waves = 2 + 2 + 2 + 1 -- the fourth wave takes the ragged tile, then
    finds the counter spent.  Here the later waves of a grid do work, on tiles another wave did not take."""
    st = _setup("mnt4753_g1")
    mem, a_karg = _memory(st, N_FULL, budget=2)
    stores = _launch_pw(st, mem, a_karg, 5)
    assert stores == [128 * 39 + 2, 128 * 39 + 2, 128 * 39 + 2, 17 * 39 + 2, 1]
    assert np.array_equal(mem.get("out").reshape(N_FULL, 78), st["block_out"])
    assert _counter(mem, N_FULL) == 7 + 2


@pytest.mark.parametrize("cname", CURVES)
def test_grid_beyond_the_tiles_and_the_counter_rearms_only_by_its_reset(cname):
    st = _setup(cname)
    mem, a_karg = _memory(st, N_SMALL)
    out = mem.get("out").reshape(N_SMALL, 78)
    # a grid of 5 waves for 2 tiles: the surplus waves store nothing
    assert _launch_pw(st, mem, a_karg, 5) == [N_SMALL * 39 + 3, 1, 1, 1, 1]
    assert np.array_equal(out, st["block_out"][:N_SMALL])
    # a second launch over the same counter without the task kernel's reset processes nothing ...
    out[:] = 0
    assert _counter(mem, N_SMALL) == 2 + 5
    assert _launch_pw(st, mem, a_karg, 2) == [1, 1]
    assert not out.any()
    # ... and with it (msm_acc_tasks_kernel writes 0) does the work again: the reset is what re-arms the counter
    mem.get("tasks")[N_SMALL * 4] = 0
    assert _launch_pw(st, mem, a_karg, 2) == [N_SMALL * 39 + 3, 1]
    assert np.array_equal(out, st["block_out"][:N_SMALL])
    _check_law(st, out, N_SMALL)


def test_stamped_variants_store_the_same_buckets_and_one_record_per_tile_or_wave():
    """the diagnostic forms (debug=True, never shipped): outputs unchanged, records inside their buffer, indexed by tile / wave"""
    st = _setup("mnt4753_g1")
    p = st["p"]
    nt = 9                                                            # the special cases: one ragged tile, one wave of one block
    for persistent in (True, False):
        g = g1_xyzz.build("dbg", p, R % p, persistent=persistent, debug=True)
        assert g.max_v == 256 and g.max_s <= 102 and hazard_scan(g, False)[0] == []
        mem, a_karg = _memory(st, nt, stamps_at=14 if persistent else 10)      # the stamps are the last argument
        if persistent:
            _launch_pw(st, mem, a_karg, 2, g)
        else:
            _wave(g, mem, a_karg, 0, 0)
        assert np.array_equal(mem.get("out").reshape(nt, 78), st["block_out"][:nt])
        rec = mem.get("stamps").reshape(2, 16)
        clk0, clk1 = int(rec[0, 0]), int(rec[0, 4])
        assert 0 < clk0 < clk1 and rec[0, 10] == 0 and rec[0, 11] == (1 << nt) - 1
        assert not rec[1].any()
