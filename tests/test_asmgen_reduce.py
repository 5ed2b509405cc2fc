"""The generated lean level 1 of the G1 bucket reduction (ginger-lib_amd/asmgen/g1_reduce.py) executed on the CPU by
asmgen/sim.py -- no GPU, no assembler needed.

The whole kernel, both primes, at L = 2 and L = 4 against the textbook group law (tests/pyref.py): every lane's
run = sum x_i and wacc = sum i x_i, compared as points, where x_i is item item0 + lane + 64 i of the lane's window (what mode 2 of
csrc/msm_reduce_kernels.h msm_wave_reduce_kernel stores, which restates the running sum of variable_base.rs:60-66).  Planted:
items at infinity at the top, in the middle and at the bottom of a lane, a lane of infinities only, an item equal to -run (the
lane goes on from infinity), an item equal to run (the program's flag must be 1: the C++ kernel computes it again; its output is
not looked at), lanes beyond `count`, a segment of padding only, and several programs per launch (blk -> window / segment).
Every load and store is checked against the buffers it may touch (sim.Memory raises outside them); the slabs start as garbage
and the flags as 0xFFFFFFFF, so nothing may depend on a memset.
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
from asmgen import g1_reduce                                      # noqa: E402
from asmgen.field import limbs, unlimbs                           # noqa: E402
from asmgen.isa import hazard_scan, module_text                   # noqa: E402
from asmgen.sim import Memory, Wave                               # noqa: E402

R = 1 << 754
_PROGS = {}


def _prog(cname):
    if cname not in _PROGS:
        p = pyref.CURVES[cname].F.p
        _PROGS[cname] = g1_reduce.build("red_" + cname, p, R % p)
    return _PROGS[cname]


def _run(cname, items, RW, count, valid, L, card=None):
    """items: RW * count affine points (None = infinity) -> per program: flag, [(run, wacc) per lane] as affine points
    card: an asm_card.Runner -- the image at device addresses, the same grid in the simulator and on the GPU, word for word"""
    C = pyref.CURVES[cname]
    p = C.F.p
    r = R % p
    ri = pow(r, -1, p)
    rnd = random.Random(3)
    g = _prog(cname)
    segs = (count + 64 * L - 1) // (64 * L)
    nprog = RW * segs

    def enc(n, pt):
        if pt is None:      # infinity is z == 0 whatever x and y are: (0, 1, 0) and a leftover of a cancelled sum both occur
            return limbs(0) + limbs(r) + limbs(0) if n % 2 else limbs(rnd.randrange(p)) + limbs(rnd.randrange(p)) + limbs(0)
        z = rnd.randrange(1, p)
        return limbs(pt[0][0] * z % p * r % p) + limbs(pt[1][0] * z % p * r % p) + limbs(z * r % p)
    mem = Memory() if card is None else card.memory()
    a_items = mem.add("items", np.array([enc(n, pt) for n, pt in enumerate(items)], dtype=np.uint32))
    a_out = mem.add("out", np.full((nprog * 64 * 2, 78), 0xDEADBEEF, dtype=np.uint32), writable=True)
    a_slabs = mem.add("slabs", np.full(nprog * g1_reduce.SLAB_BYTES // 4, 0xDEADBEEF, dtype=np.uint32), writable=True)
    a_flag = mem.add("flag", np.full(nprog, 0xFFFFFFFF, dtype=np.uint32), writable=True)
    karg = np.zeros(14, dtype=np.uint32)
    for j, a in enumerate((a_items, a_out, a_slabs, a_flag)):
        karg[2 * j], karg[2 * j + 1] = a & 0xFFFFFFFF, a >> 32
    karg[8:13] = (count, valid, segs, L, nprog)
    a_karg = mem.add("karg", karg)
    assert g.kernarg_bytes == 56
    if card is not None:
        from asm_card import Launch
        assert card.run(mem, [Launch(g, a_karg, (segs, RW), 64)]) == []
        mem.release()
    for w_ in range(RW if card is None else 0):
        for seg in range(segs):
            w = Wave(g, mem, strict=True)
            w.S[0], w.S[1], w.S[2], w.S[3] = a_karg & 0xFFFFFFFF, a_karg >> 32, seg, w_
            w.V[0] = np.arange(64, dtype=np.uint32)
            w.V[40:256] = 0x1234567                                 # registers start as garbage too
            w.run()
            assert w.hist.get("global_store_dword", 0) + w.hist.get("global_store_dwordx2", 0) > 0
    out = mem.get("out").reshape(nprog, 64, 2, 3, 26)
    flag = mem.get("flag")
    res = []
    for b in range(nprog):
        assert flag[b] in (0, 1), "program %d did not write its flag" % b
        lanes = []
        for l in range(64):
            pair = []
            for s in range(2):
                xyz = [unlimbs(out[b, l, s, k]) for k in range(3)]
                if flag[b] == 0:
                    assert max(xyz) < p and int(out[b, l, s].max()) < (1 << 29), "unreduced output"
                X, Y, Z = (v * ri % p for v in xyz)
                pair.append(C.proj_to_affine((X,), (Y,), (Z,)))
            lanes.append(tuple(pair))
        res.append((int(flag[b]), lanes))
    return g, res


def _points(C, n, seed):
    rnd = random.Random(seed)
    h = C.mul(rnd.randrange(1, 1 << 60), C.G)
    pt = C.mul(rnd.randrange(1, 1 << 60), C.G)
    out = []
    for _ in range(n):
        out.append(pt)
        pt = C.add(pt, h)
    return out


def _expected(C, items, w, count, item0, lane, L):
    run = wacc = None
    for i in range(L):
        k = item0 + lane + 64 * i
        x = items[w * count + k] if k < count else None
        run = C.add(run, x)
        for _ in range(i):
            wacc = C.add(wacc, x)
    return run, wacc


def _check(C, items, res, RW, count, valid, L, flagged):
    segs = (count + 64 * L - 1) // (64 * L)
    for b, (flag, lanes) in enumerate(res):
        w, seg = divmod(b, segs)
        item0 = seg * 64 * L
        assert flag == (1 if b in flagged else 0), (b, flag)
        if flag:
            continue
        for l in range(64):
            if w * count + item0 >= valid:
                exp = (None, None)
            else:
                exp = _expected(C, items, w, count, item0, l, L)
            assert lanes[l] == exp, (b, l)


@pytest.mark.parametrize("cname", ["mnt4753_g1", "mnt6753_g1"])
def test_lean_level_1_at_L4_in_the_simulator(cname):
    """two windows of 200 items, one segment each: lanes 8.. have no item 3 (k = lane + 64 i < 200)"""
    C = pyref.CURVES[cname]
    RW, count, L = 2, 200, 4
    items = _points(C, RW * count, 21)
    it = lambda w, l, i: w * count + l + 64 * i
    # window 0 (program 0): nothing that doubles
    items[it(0, 0, 3)] = None                                       # infinity at the top ...
    items[it(0, 1, 1)] = None                                       # ... in the middle ...
    items[it(0, 2, 0)] = None                                       # ... at the bottom of a lane
    for i in range(4):
        items[it(0, 3, i)] = None                                   # a lane of infinities
    items[it(0, 4, 2)] = C.neg(items[it(0, 4, 3)])                  # item == -run: the lane goes on from infinity
    items[it(0, 5, 1)] = C.neg(C.add(items[it(0, 5, 3)], items[it(0, 5, 2)]))
    items[it(0, 9, 2)] = None                                       # the first item of a lane that has three
    # window 1 (program 1): lane 2 meets item == run
    items[it(1, 2, 2)] = items[it(1, 2, 3)]
    g, res = _run(cname, items, RW, count, RW * count, L)
    _check(C, items, res, RW, count, RW * count, L, flagged={1})
    assert g.max_v == 256 and g.max_s <= 102 and g.max_a < 0 and g.lds_bytes == 0


@pytest.mark.parametrize("cname", ["mnt4753_g1", "mnt6753_g1"])
def test_lean_level_1_at_L2_with_padding_in_the_simulator(cname):
    """two windows of 140 items in two segments of 128 slots; the last segment of the last window is padding only"""
    C = pyref.CURVES[cname]
    RW, count, L = 2, 140, 2
    valid = count + 128                                             # w = 1, seg = 1: 140 + 128 >= valid
    items = _points(C, RW * count, 22)
    for k in range(valid, RW * count):
        items[k] = None                                             # what the buffer holds behind `valid`
    it = lambda w, l, i: w * count + l + 64 * i
    items[it(0, 0, 1)] = None                                       # top
    items[it(0, 1, 0)] = None                                       # bottom
    items[it(0, 2, 0)] = items[it(0, 2, 1)] = None
    items[it(0, 3, 0)] = C.neg(items[it(0, 3, 1)])                  # P + (-P): the formula's Z = 0
    items[it(1, 7, 0)] = items[it(1, 7, 1)]                         # P + P in program 2 (w = 1, seg = 0)
    g, res = _run(cname, items, RW, count, valid, L)
    assert len(res) == 4
    _check(C, items, res, RW, count, valid, L, flagged={2})
    # the segment behind the window's last item (program 1: 12 lanes with item 0 only) and the padding program
    assert all(lane == (None, None) for lane in res[3][1])
    assert sum(1 for lane in res[1][1] if lane[0] is not None) == 12 and all(lane[1] is None for lane in res[1][1])


def test_generated_reducer_is_well_formed():
    g = _prog("mnt4753_g1")
    text, info = module_text([g])
    assert ".amdhsa_private_segment_fixed_size 0" in text and ".amdhsa_group_segment_fixed_size 0" in text
    assert ".amdhsa_system_sgpr_workgroup_id_y 1" in text
    assert info[g.name]["vgprs"] == 256 and g.kernarg_bytes == 56
    assert hazard_scan(g, False)[0] == []
    stores = [i for i in g.ins if i.op.startswith("global_store")]
    assert stores and all(i.op in ("global_store_dword", "global_store_dwordx2") for i in stores)      # vector stores only
    assert not any(i.op.startswith("ds_") for i in g.ins)
    for i in g.ins:
        if i.op.startswith("global_"):
            assert 0 <= int(i.mods.get("offset", 0)) < 4096
    # one addition, emitted once: 10 products, 2 squares, one dual product -- the multiplier instructions fp29.h counts -- and
    # three address computations
    assert g.count(lambda i: i.op == "v_mad_u64_u32") == 10 * 1352 + 2 * 1027 + 2028 + 3
