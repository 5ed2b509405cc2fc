"""The MSM's bucket reduction on the card, program by program: the three written-out copies of the wave program of
ginger-lib_amd/csrc/msm_reduce_kernels.h -- msm_wave_reduce_kernel (G1) in its 512- and 256-register builds on both curves, the
Fq2 build of msm_wave_reduce_split_kernel (the loop written out a second time) and its Fq3 build (wave_reduce_program over a
GroupView) -- and msm_heavy_combine_kernel of msm_kernels.h on all four curves, each launched through
tests/device_shim/msm_reduce.hip with the launch shape of msm_impl.h (reduce_level, launch_accumulate) and read back.

The referee is tests/msm_reduce_ref.py: every item is a known multiple of one base point, the expected sums are written down by
definition in the integers mod r, and each expected point is the summed multiple of the base point (the referee's own
inversion-free group arithmetic, which test_internal_form_round_trip holds against pyref.Curve.mul).  Comparisons are exact:
  * every output buffer starts as 0xFFFFFFFF words and carries a guard row behind it, the slabs a guard row of 64 words; rows no
    program may write (another program's skipped rows, the rows of run_if = 0 programs, everything behind the launch) must still
    hold the fill;
  * a written row must decode: every limb below 2^29, every coefficient below p -- fp29.h keeps a field element "always fully
    reduced into [0, p)", and the reduction's additions end in products and subtractions of that form, so [0, p) is the bound
    of every coordinate the kernels store;
  * the row is then compared AS A POINT with the model's: affine after division by Z, infinity iff Z = 0 (and then Y != 0);
  * an all-padding segment must give proj_zero = (0, one, 0) limb for limb, from slots filled with 0xFFFFFFFF: they are not read.
Items arrive as (X z, Y z, z) with a random z each, so equal points are different projective representatives.

The CPU part (no marker) cross-compiles the shim for gfx950, pins the model to what an MSM means (level 1 -> level 2 -> the
host fold of msm_fold.h gives sum s_i b_i, segment form and lean form, 64, 32 and 16 groups per wave), proves by a replay of the
schedule (msm_schedule.h through the host shim) that every operand set holds the collision it is named for and none it does
not claim, asserts that the sets together reach the detour at each of the five step kinds and every tree offset, and checks
every address each launch will form against the buffers it gets.  The card half launches nothing the host has not validated.

The shim is one shared object per curve (build/libmsm_reduce_<k>.so), compiled side by side.  Measured once (hipcc, gfx950, the
product's flags): as ONE object the shim takes 102 s to compile; as four, side by side, 25 s (mnt4753_g1), 37 s (mnt4753_g2),
37 s (mnt6753_g1) and 44 s (mnt6753_g2), 44 s in all -- hence one per curve.  With a warm build the card half of this file
takes 13 s on an MI355X (86 tests, 1016 launches; the slowest test 0.5 s)."""
import ctypes
import functools
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import asm_card
import msm_reduce_ref as R
import pyref
import shim_build

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
FILL = R.FILL
ITEM, WACC, TREE_WACC, SCAN, TREE_RUN = R.ITEM, R.WACC, R.TREE_WACC, R.SCAN, R.TREE_RUN

# the six builds of the wave program: cid as msm_reduce_ref.CURVE_NAMES, curve / waves as the launchers take them
BUILDS = {
    "g1_p4_w1": dict(cid=0, curve=4, waves=1, tpw=64), "g1_p4_w2": dict(cid=0, curve=4, waves=2, tpw=64),
    "g1_p6_w1": dict(cid=2, curve=6, waves=1, tpw=64), "g1_p6_w2": dict(cid=2, curve=6, waves=2, tpw=64),
    "fq2": dict(cid=1, curve=4, waves=0, tpw=32), "fq3": dict(cid=3, curve=6, waves=0, tpw=16),
}
LS = (1, 2, 3, 4, 5, 16)
BASE_T = 0x5EED5EED5EED5EED5EED5EED7          # the base point of every set but `salts`: P = BASE_T G


def so_path(cid):
    return os.path.join(shim_build.BUILD, "libmsm_reduce_%d.so" % cid)


def counts_of(tpw, L):
    return sorted({1, tpw - 1, tpw, tpw + 1, tpw * L - 1, tpw * L, tpw * L + 1, 2 * tpw * L + tpw + 1} - {0})


# ------------------------------------------------------------------ the host shim (msm_schedule.h, msm_fold.h with g++)
@functools.lru_cache(maxsize=None)
def host_shim():
    lib = shim_build.host_shim("msm_host")
    lib.t_wave_step.argtypes = [u32] + [cint] * 3 + [ctypes.POINTER(cint)]
    lib.t_wave_step_active.argtypes = [cint] * 5
    lib.t_fold.argtypes = [cint, cint, ctypes.POINTER(u64)] + [cint] * 6 + [ctypes.POINTER(u64)]
    return lib


@functools.lru_cache(maxsize=None)
def form(cid):
    return R.Form(cid)


@functools.lru_cache(maxsize=None)
def group(cid, t):
    return R.Group(form(cid), t)


# ------------------------------------------------------------------ cases: a launch and the multiples in its input buffer
class Case:
    """name, the launch, the buffer's slots as multiples of P = t G (UNREAD: a slot no program may load)"""

    def __init__(self, name, launch, mult, t=BASE_T, seed=0):
        self.name, self.launch, self.t, self.seed = name, launch, t, seed
        reads = launch.reads()
        self.mult = [m if j in reads else R.UNREAD for j, m in enumerate(mult)]
        self.max_read = max(reads) if reads else -1

    def validate(self, in_slots, out_rows, slab_programs):
        """every address the kernel forms from (count, stride, offset, W, segs, L) against what the test allocates"""
        la = self.launch
        assert la.L >= 1 and la.segs >= 1 and la.programs() >= 1
        assert self.max_read < in_slots == len(self.mult), (self.name, "input", self.max_read, in_slots)
        assert la.programs() <= slab_programs, (self.name, "slabs")
        top = max(max(la.rows_of(gb)) for gb in range(la.programs()))
        assert top < la.out_rows() <= out_rows, (self.name, "output", top, out_rows)
        for i in la.ins:                     # the indices are 32-bit in the kernel before they are widened
            assert (la.per_input // la.segs + 1) * i.count * i.stride + i.offset < 1 << 31


def single(tpw, L, W, count, mode=0, valid=FILL, run_if=None):
    segs = (count + tpw * L - 1) // (tpw * L)
    return R.Launch([R.In(1, 0, count, mode, valid)], W * segs, segs, L, tpw, run_if)


def strided(tpw, L, W, count, modes):
    """the level-2 forms of launch_reduce: one buffer, stride = number of inputs, offset = which, one program per window and input"""
    assert count <= tpw * L
    n = len(modes)
    return R.Launch([R.In(n, k, count, m) for k, m in enumerate(modes)], W, 1, L, tpw)


def draw(rnd, n, lo=1, hi=1 << 12):
    return [rnd.randrange(lo, hi) for _ in range(n)]


def slots_of(launch):
    return max(max((i.flat(launch.per_input // launch.segs - 1, i.count - 1) for i in launch.ins)) + 1, 1)


@functools.lru_cache(maxsize=None)
def shape_cases(tpw, L):
    """one input in mode 0, every count of the list, W alternating 1 and 3"""
    rnd = random.Random(1000 * tpw + L)
    out = []
    for n, count in enumerate(counts_of(tpw, L)):
        la = single(tpw, L, (1, 3)[n % 2], count)
        out.append(Case("random L %d W %d count %d" % (L, (1, 3)[n % 2], count), la, draw(rnd, slots_of(la)), seed=n))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases(tpw):
    rnd = random.Random(77 + tpw)
    out = []
    for L in (1, 3):
        for count in (tpw * L + 1, 2 * tpw * L + tpw + 1):
            W, last = 3, (count - 1) // (tpw * L) * tpw * L          # item0 of the last segment
            # the last segment of the last window wholly padding (never read: 0xFF..), and a valid inside that segment
            # and valids inside the last segment and inside the one before it (then the last is padding as well)
            forms = [("segment", last), ("before", last - 3)] + ([("inside", last + 5)] if count - last > 5 else [])
            for what, valid in [(a, (W - 1) * count + v) for a, v in forms]:
                la = single(tpw, L, W, count, 0, valid)
                mult = [m if j < valid else 0 for j, m in enumerate(draw(rnd, W * count))]
                out.append(Case("valid %s L %d count %d" % (what, L, count), la, mult))
                if what == "segment":
                    assert out[-1].mult[valid:] == [R.UNREAD] * (W * count - valid) and R.UNREAD not in out[-1].mult[:valid]
    return out


@functools.lru_cache(maxsize=None)
def strided_cases(tpw):
    rnd = random.Random(99 + tpw)
    out = []
    for modes in ((0, 1, 1), (0, 1)):
        for n, L in enumerate((1, 2, 3, 5)):
            for count in sorted({1, min(tpw + 1, tpw * L), tpw * L - 1, tpw * L} - {0}):
                W = (3, 1)[n % 2]
                la = strided(tpw, L, W, count, modes)
                mult = draw(rnd, slots_of(la))
                if count > 2:                                             # some segment sums are infinity, as level 1 delivers them
                    for j in rnd.sample(range(len(mult)), len(mult) // 5):
                        mult[j] = 0
                out.append(Case("stride %d L %d W %d count %d" % (len(modes), L, W, count), la, mult))
    return out


@functools.lru_cache(maxsize=None)
def lean_cases():
    """mode 2 (G1): run_if null, all ones and a mixed pattern; W segs >= 3 programs"""
    rnd = random.Random(4242)
    out = []
    for L, count in ((1, 129), (2, 129), (3, 192), (3, 385), (16, 1025)):
        W = 3
        segs = (count + 64 * L - 1) // (64 * L)
        n = W * segs
        patterns = [("null", None), ("ones", [1] * n), ("mixed", [(g * 5 + 1) % 3 != 0 for g in range(n)])]
        for what, run_if in patterns if L != 16 else patterns[2:]:
            valid = FILL if L != 3 else (W - 1) * count + (segs - 1) * 64 * L       # L = 3: the last program all padding
            la = single(64, L, W, count, 2, valid, None if run_if is None else [int(v) for v in run_if])
            mult = [m if j < valid else 0 for j, m in enumerate(draw(rnd, W * count))]
            for j in rnd.sample(range(len(mult)), len(mult) // 4):
                mult[j] = 0
            out.append(Case("lean L %d count %d run_if %s" % (L, count, what), la, mult))
    assert any(c.launch.run_if and 0 in c.launch.run_if and 1 in c.launch.run_if for c in out)
    return out


# ------------------------------------------------------------------ operand sets: one segment, built for one collision
class OperandSet:
    """name; mode, L; the items of ONE full or ragged segment; t; and what the replay must find:
    exact: {(kind, off or i): groups} -- the detours are exactly these; first: (key, groups) -- no detour before that step and
    exactly these groups there; check(steps): further assertions"""

    def __init__(self, name, mode, L, items, t=BASE_T, exact=None, first=None, check=None):
        self.name, self.mode, self.L, self.items, self.t, self.exact, self.first, self.check = name, mode, L, items, t, exact, first, check

    def steps(self, tpw, r):
        return R.replay(host_shim(), self.mode, self.L, tpw, self.items, r, self.t)[3]

    def holds(self, tpw, r):
        """None, or why the set does not hold what it is named for"""
        steps = self.steps(tpw, r)
        got = R.collisions(steps)
        if self.exact is not None and got != self.exact:
            return "%s: detours %s, named %s" % (self.name, got, self.exact)
        if self.first is not None:
            key, groups = self.first
            order = [(s.kind, s.i if s.kind in (ITEM, WACC) else s.off) for s in steps if s.detour]
            if not order or order[0] != key or got[key] != groups:
                return "%s: first detour %s %s, named %s %s" % (self.name, order[:1], got.get(key), key, groups)
        if self.check is not None:
            return self.check(steps)
        return None


def items_of(x, tpw, L):
    """x[g][i] -> the segment's items j = g + tpw i"""
    return [x[j % tpw][j // tpw] for j in range(tpw * L)]


def tree_before(vals, off, lo=0):
    """the tree's accumulators before its step `off`: acc[g] = sum of vals[h], h = g mod 2 off, h >= lo"""
    return [sum(vals[h] for h in range(g, len(vals), 2 * off) if h >= lo) for g in range(2 * off)]


def tree_set(tpw, kind, mode, off, pairs, rnd):
    """L = 2: wacc_g = x_(g,1), run_g = x_(g,0) + x_(g,1); the groups `pairs` meet equal operands with g + off at the step `off`"""
    wacc, run = draw(rnd, tpw, 1, 400), draw(rnd, tpw, 401, 900)
    if kind == TREE_WACC or (kind == TREE_RUN and mode == 1):
        v = wacc if kind == TREE_WACC else run
        acc = tree_before(v, off)
        for g in pairs:
            v[g + off] += acc[g] - acc[g + off]
    elif kind == SCAN:
        for g in sorted(pairs, reverse=True):
            win = lambda a: sum(run[a:min(a + off, tpw)])
            run[g] += win(g + off) - win(g)
    else:                                    # the last tree of mode 0 runs over the suffix sums S_g, g >= 1
        S = draw(rnd, tpw, 1000, 5000) + [0]
        acc = tree_before(S[:tpw], off, lo=1)
        for g in pairs:
            S[g + off] += acc[g] - acc[g + off]
        run = [S[h] - S[h + 1] for h in range(tpw)]
    return items_of([[run[g] - wacc[g], wacc[g]] for g in range(tpw)], tpw, 2)


def tree_pairs(tpw, kind, mode, off):
    if kind == SCAN:
        return list(range(tpw - off))
    return list(range(1 if (kind == TREE_RUN and mode == 0 and off == tpw // 2) else 0, off))     # S_0 has left the last tree


def find(tpw, r, make, what):
    """the first seed whose items hold exactly the named collision (a chance collision elsewhere: the next seed)"""
    why = None
    for seed in range(64):
        s = make(random.Random(seed * 7919 + tpw))
        why = s.holds(tpw, r)
        if why is None:
            return s
    raise AssertionError("no seed gives %s: %s" % (what, why))


@functools.lru_cache(maxsize=None)
def sets_for(tpw, cid):
    """every operand set for a curve: tree_k / scan_k / treerun_k / tree1_k for every offset, once for exactly one pair and once
    for all pairs, and the serial sets in every mode the build has"""
    r = form(cid).r
    half = tpw // 2
    sets = []
    offs = [half >> s for s in range(tpw.bit_length() - 1)]
    for name, kind, mode in (("tree", TREE_WACC, 0), ("scan", SCAN, 0), ("treerun", TREE_RUN, 0), ("tree1", TREE_RUN, 1)):
        for off in offs:
            allp = tree_pairs(tpw, kind, mode, off)
            one = [allp[len(allp) // 2]]
            sets.append(find(tpw, r, lambda rnd: OperandSet("%s_%d one" % (name, off), mode, 2, tree_set(tpw, kind, mode, off, one, rnd),
                                                            exact={(kind, off): one}), "%s_%d one" % (name, off)))
            sets.append(find(tpw, r, lambda rnd: OperandSet("%s_%d all" % (name, off), mode, 2, tree_set(tpw, kind, mode, off, allp, rnd),
                                                            first=((kind, off), allp)), "%s_%d all" % (name, off)))
    modes = (0, 1, 2) if tpw == 64 else (0, 1)
    for mode in modes:
        sets += serial_sets(tpw, r, mode)
    return sets


def serial_sets(tpw, r, mode):
    L = 3
    half = tpw // 2
    tag = " mode %d" % mode

    def rand_x(rnd):
        return [draw(rnd, L, 3, 400) for _ in range(tpw)]

    def item_dbl(rnd):
        x = rand_x(rnd)
        x[3][1] = x[3][2]                                   # run == item at ITEM i = 1; item 0 follows in the same lane
        return OperandSet("item_dbl" + tag, mode, L, items_of(x, tpw, L), exact={(ITEM, 1): [3]})

    def with_inf(rnd):
        x = rand_x(rnd)
        x[3][1] = x[3][2]
        x[5][2] = 0                                         # lane 5's run is still infinity at the step lane 3 detours in

        def check(steps):
            s = [s for s in steps if s.kind == ITEM and s.i == 1][0]
            return None if sorted(s.detour) == [3] and s.inf.get(5) == "p" else "with_inf: %r" % s
        return OperandSet("with_inf" + tag, mode, L, items_of(x, tpw, L), exact={(ITEM, 1): [3]}, check=check)

    def sparse(rnd):
        Ls = 4
        x = [[rnd.randrange(3, 400) if rnd.randrange(3) == 0 else 0 for _ in range(Ls)] for _ in range(tpw)]
        x[1] = [0, 0, 0, 9]                                 # a first item, then infinities: wacc == run at the next WACC
        x[2] = [11, 0, 0, 0]                                # leading infinities: p infinite when the item arrives
        items = items_of(x, tpw, Ls)[:tpw * Ls - 3]         # ragged: the last three groups have no item 3

        def check(steps):
            if mode != 1 and not any(s.kind == WACC and 1 in s.detour for s in steps):
                return "sparse: no detour in a WACC step"
            ok_p = any(s.kind == ITEM and s.inf.get(2) == "p" for s in steps)
            ok_q = any(s.kind == ITEM and s.inf.get(1) == "q" for s in steps)
            return None if ok_p and ok_q else "sparse: pz %s qz %s" % (ok_p, ok_q)
        return OperandSet("sparse" + tag, mode, Ls, items, check=check)

    def cancel(rnd):
        x = rand_x(rnd)
        x[2] = [17, -x[2][2], x[2][2]]                      # P, -P in one group: run returns to infinity, then takes item 0
        wacc = [sum(i * v for i, v in enumerate(xs)) for xs in x]
        x[1 + half][1] -= wacc[1] + wacc[1 + half]          # wacc of group 1 + half = -wacc of group 1: the first tree step cancels

        def check(steps):
            if R.collisions(steps):
                return "cancel: a detour %s" % R.collisions(steps)
            a = any(s.kind == ITEM and s.i == 0 and s.inf.get(2) == "p" for s in steps)
            b = mode != 0 or any(s.kind == TREE_WACC and s.off == half // 2 and "p" in s.inf.get(1, "") for s in steps)
            return None if a and b else "cancel: the infinite sum is not used again (%s, %s)" % (a, b)
        return OperandSet("cancel" + tag, mode, L, items_of(x, tpw, L), check=check)

    def all_equal(rnd):
        def check(steps):
            for s in steps:
                if s.kind == ITEM and s.i == L - 2 and sorted(s.detour) != list(range(tpw)):   # x + x; item 0 meets 2 x
                    return "all_equal: %r" % s
                if (s.kind == TREE_WACC or (s.kind == TREE_RUN and mode == 1)) and sorted(s.detour) != list(range(s.off)):
                    return "all_equal: %r" % s
                if s.kind == SCAN and s.off == 1 and sorted(s.detour) != list(range(tpw - 1)):
                    return "all_equal: %r" % s
            return None
        return OperandSet("all_equal" + tag, mode, L, [5] * (tpw * L), check=check)

    def all_inf(rnd):
        def check(steps):
            bad = [s for s in steps if s.detour]
            return "all_inf: %r" % bad[0] if bad else None
        return OperandSet("all_inf" + tag, mode, L, [0] * (tpw * L - 1), check=check)

    out = [find(tpw, r, f, f.__name__ + tag) for f in (item_dbl, with_inf, sparse, cancel, all_equal, all_inf)]
    # salts: P = G.  p = G, -G refuse S0 (it has the x of p) and take S1 = 2 G; p = 2 G, -2 G and (r - 1) / 2 G take S0; for the last
    # 2 p = -S0, so that the detour's tmp = 2 p + S0 is infinity and its last step runs through the pz patch (p = -G: G + (-G))
    SALT_M = (1, -1, 2, -2, (r - 1) // 2)
    WANT = (1, 1, 0, 0, 0)
    for n, m in enumerate(SALT_M):
        def one(rnd, m=m, n=n):
            x = rand_x(rnd)
            x[2] = [7, m, m]

            def check(steps):
                s = [s for s in steps if s.kind == ITEM and s.i == 1][0]
                inf_ok = (2 in s.detour_inf) == (m in (-1, (r - 1) // 2))
                return None if s.detour == {2: WANT[n]} and inf_ok else "salts: %r %s %s" % (s, s.detour, s.detour_inf)
            return OperandSet("salts m %d%s" % (n, tag), mode, L, items_of(x, tpw, L), t=1, exact={(ITEM, 1): [2]}, check=check)
        out.append(find(tpw, r, one, "salts"))

    def together(rnd):
        x = rand_x(rnd)
        for n, m in enumerate(SALT_M):
            x[1 + n] = [7 + n, m, m]

        def check(steps):
            s = [s for s in steps if s.kind == ITEM and s.i == 1][0]
            return None if s.detour == {1 + n: w for n, w in enumerate(WANT)} else "salts: %r %s" % (s, s.detour)
        return OperandSet("salts together" + tag, mode, L, items_of(x, tpw, L), t=1, exact={(ITEM, 1): [1, 2, 3, 4, 5]}, check=check)
    out.append(find(tpw, r, together, "salts together"))
    return out


def set_case(s, tpw, rnd):
    """the set as a launch: its segment as window 0 and a random window 1 behind it (a second block)"""
    count = len(s.items)
    la = single(tpw, s.L, 2, count, s.mode)
    return Case(s.name, la, list(s.items) + draw(rnd, count), t=s.t)


# ------------------------------------------------------------------ the shim
def build_shim():
    """build/libmsm_reduce_<k>.so, k = 0 .. 3, from the shipped headers with the product's compiler flags, side by side; rebuilt
    when a source is newer.  -> {curve name: seconds} of what was compiled"""
    with ThreadPoolExecutor(max_workers=4) as ex:
        took = list(ex.map(lambda k: shim_build.device_shim("msm_reduce.hip", so_path(k), ["-DRD_CURVE=%d" % k]), range(4)))
    return {R.CURVE_NAMES[k]: t for k, t in enumerate(took) if t}


LAUNCHERS = {
    "rd_wave_g1": [cint, cint, vp, vp, vp, u32, u32, u32, cint, vp, vp, vp, vp],
    "rd_wave_g2": [cint, vp, vp, vp, u32, u32, u32, cint, vp, vp, vp],
    "rd_heavy_combine": [cint, vp, vp, vp, u32, vp],
}


class Bufs:
    """the device buffers of one check: freed together"""

    def __init__(self, card):
        self.card, self.addrs = card, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for a in self.addrs:
            self.card.free(a)

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes > 0
        a = self.card.malloc(arr.nbytes)
        self.addrs.append(a)
        self.card.upload(a, arr)
        return a

    def filled(self, words):
        return self.put(np.full(words, FILL, dtype=np.uint32))

    def get(self, addr, words):
        out = np.empty(words, dtype=np.uint32)
        self.card.download(addr, out)
        return out


class Reduce:
    def __init__(self):
        self.build_seconds = build_shim()
        self.libs = {}
        self.card = asm_card.Card()
        self.failed = None
        self.launches = 0
        self.rows = {}

    def lib(self, cid):
        if cid not in self.libs:
            lib = ctypes.CDLL(so_path(cid))
            for name, args in LAUNCHERS.items():
                getattr(lib, name).argtypes = args
            lib.rd_sizeof.argtypes = [cint, cint]
            lib.rd_sizeof.restype = u32
            f = form(cid)
            assert lib.rd_sizeof(cid, 0) == 4 * f.aff_words and lib.rd_sizeof(cid, 1) == 4 * f.proj_words
            assert lib.rd_sizeof(cid, 3) == 4 * 3 * R.NL and lib.rd_sizeof(cid, 2) == slab_words(cid)
            self.libs[cid] = lib
        return self.libs[cid]

    def run(self, cid, name, *args):
        """one launcher; after a launch that did not come back clean nothing more is started on the card"""
        if self.failed:
            raise RuntimeError("not launched: %s failed earlier" % self.failed)
        e = getattr(self.lib(cid), name)(*args)
        self.launches += 1
        if e != 0:
            self.failed = "%s (hip error %d)" % (name, e)
            raise RuntimeError(self.failed)

    def close(self):
        self.card.close()
        assert self.card.allocs == []

    def check(self, build, case):
        """launch the case on the build -> failures"""
        b = BUILDS[build]
        cid, la = b["cid"], case.launch
        assert la.tpw == b["tpw"]
        f, G = form(cid), group(cid, case.t)
        pw, sw = f.proj_words, slab_words(cid)
        out_rows, progs = la.out_rows(), la.programs()
        case.validate(len(case.mult), out_rows, progs)
        key = (cid, case.name)                       # the two register builds of a curve take the same rows
        if key not in self.rows:
            self.rows[key] = G.item_rows(case.mult, random.Random(case.seed))
        rows = self.rows[key]
        want = la.expect(case.mult, f.r)
        with Bufs(self.card) as B:
            a_in, a_salts = B.put(rows), B.put(group(cid, 1).salt_rows())
            a_out, a_slabs = B.filled((out_rows + 1) * pw), B.filled(progs * sw + 64)
            a_run = B.put(np.asarray(la.run_if, dtype=np.uint32)) if la.run_if is not None else None
            ins = [np.array(i.words(a_in), dtype=np.uint64) for i in la.ins]
            ins += [np.zeros(6, dtype=np.uint64)] * (3 - len(ins))           # msm_impl.h `none`
            ptr = [i.ctypes.data_as(vp) for i in ins]
            if b["waves"]:
                self.run(cid, "rd_wave_g1", b["curve"], b["waves"], *ptr, la.per_input, la.n_inputs, la.segs, la.L, a_salts, a_out,
                         a_slabs, a_run)
            else:
                assert la.run_if is None and all(i.mode != 2 for i in la.ins)
                self.run(cid, "rd_wave_g2", b["curve"], *ptr, la.per_input, la.n_inputs, la.segs, la.L, a_salts, a_out, a_slabs)
            out = B.get(a_out, (out_rows + 1) * pw).reshape(out_rows + 1, pw)
            slabs = B.get(a_slabs, progs * sw + 64)
            back = B.get(a_in, rows.size).reshape(rows.shape)
        fails = []
        if not np.array_equal(back, rows):
            fails.append("the input buffer changed")
        if not np.all(slabs[progs * sw:] == FILL):
            fails.append("the guard row behind the slabs changed")
        fails += compare_rows(G, out, want)
        return ["%s / %s: %s" % (build, case.name, x) for x in fails]


def compare_rows(G, out, want):
    """every row of the buffer (its guard row included) against {row: multiple | ZERO}; absent rows must hold the fill"""
    fails = []
    for row in range(len(out)):
        if row not in want:
            if not np.all(out[row] == FILL):
                fails.append("row %d%s was written" % (row, " (the guard row)" if row == len(out) - 1 else ""))
        elif want[row] is R.ZERO or want[row] == R.ZERO:
            if not np.array_equal(out[row], G.form.zero_row):
                fails.append("row %d is not proj_zero limb for limb" % row)
        elif np.all(out[row] == FILL):
            fails.append("row %d was not written" % row)
        else:
            why = G.same_point(out[row], want[row])
            if why:
                fails.append("row %d: %s" % (row, why))
    return fails[:6] + (["... %d failures" % len(fails)] if len(fails) > 6 else [])


def slab_words(cid):
    """WaveSlab<T>::WORDS: three accumulators, word-major over 64 lanes; T = Proj<C> on G1, P3 (one coefficient per lane) on G2"""
    return 3 * 64 * (form(cid).proj_words if form(cid).k == 1 else 3 * R.NL)


@pytest.fixture(scope="module")
def dev(gpu):
    d = Reduce()
    print("\nlibmsm_reduce_*.so: %s" % (d.build_seconds or "up to date"))
    yield d
    print("\n%d launches" % d.launches)
    d.close()


# ------------------------------------------------------------------ CPU: the shim, the model, the operand sets, the addresses
def test_shim_cross_compiles_for_gfx950():
    took = build_shim()
    if took:
        print("\ncompiled: %s" % {k: round(v, 1) for k, v in took.items()})
    names = {0: ("Mnt4G1",), 1: ("Mnt4G2", "F2S"), 2: ("Mnt6G1",), 3: ("Mnt6G2", "F3S")}
    for k in range(4):
        blob = open(so_path(k), "rb").read()
        assert b"gfx950" in blob
        kernels = ("msm_heavy_combine_kernel", "msm_wave_reduce_kernel" if k in (0, 2) else "msm_wave_reduce_split_kernel")
        for s in kernels + names[k] + tuple(LAUNCHERS) + ("rd_sizeof",):
            assert s.encode() in blob, (k, s)
    # the lane-group fields the shim names are the ones msm_impl.h chooses, and the launch shapes are the ones it uses
    impl = open(os.path.join(shim_build.CSRC, "msm_impl.h")).read()
    assert "typename std::conditional<C::F::DEG == 2, F2S<P4, 13>, F3S<P6, 11>>::type" in impl
    assert "msm_wave_reduce_split_kernel<C, FS, FS::LANES, DEG == 2 ? 32 : 16>), dim3(grid), dim3(64), 64 * sizeof(P3)" in impl
    assert "msm_wave_reduce_kernel<C, 1>), dim3(grid), dim3(64), 64 * sizeof(Proj<C>)" in impl
    assert "msm_heavy_combine_kernel<C>), dim3(n_heavy), dim3(64), 64 * sizeof(Proj<C>)" in impl


def test_internal_form_round_trip():
    for cid in range(4):
        f = form(cid)
        G = group(cid, 1)
        assert (f.one_row[:R.NL] == R.to_limbs([R.RADIX % f.p])[0]).all() and R.from_limbs(R.to_limbs([f.p - 1])[0]) == f.p - 1
        rows = G.item_rows([1, -1, 0, 2, R.UNREAD, 70000], random.Random(5))
        assert int(rows[[0, 1, 2, 3, 5]].max()) < 1 << R.LB and (rows[4] == FILL).all()
        for row, m in zip(rows, [1, -1, 0, 2, None, 70000]):
            if m is not None:
                assert G.same_point(row, m % f.r) is None and G.same_point(row, (m + 1) % f.r) is not None
        # the group's own projective arithmetic against the affine definition of pyref: both tables' edges, a multiple above
        # 2^16, negatives, one of full size, and on another base point
        C, H = G.C, group(cid, BASE_T)
        for m in (1, 2, 3, 255, 256, 257, 65535, 65536, 70000, (1 << 33) + 12345, f.r - 1, f.r - 3, (f.r - 1) // 2):
            assert G.point(m) == C.mul(m, C.G), m
        assert G.point(-3) == C.neg(C.mul(3, C.G)) and G.point(0) is None and G.point(f.r) is None
        assert H.point(1) == C.mul(BASE_T, C.G) and H.point(77777) == C.mul(77777 * BASE_T % f.r, C.G) and H.point(-2) == C.neg(C.mul(2, H.point(1)))
        assert G.same_point(f.zero_row, 0) is None
        bad = rows[0].copy()
        bad[3] |= 1 << 29
        assert "limb" in G.same_point(bad, 1)
        bad = rows[0].copy()
        bad[:R.NL] = R.to_limbs([f.p])[0]
        assert "below p" in G.same_point(bad, 1)
        S = G.salt_rows()
        assert S.shape == (2, f.aff_words)
        one = np.concatenate([f.one_row])
        assert G.same_point(np.concatenate([S[1], one]), 2) is None


def abi_points(cid, mults):
    """multiples of G -> the u64 words of projective ABI points, as the fold reads them"""
    C, F = pyref.CURVES[R.CURVE_NAMES[cid]], pyref.CURVES[R.CURVE_NAMES[cid]].F
    E = C.E
    words = []
    for m in mults:
        pt = group(cid, 1).point(m)
        X, Y, Z = (E.zero(), E.one(), E.zero()) if pt is None else (pt[0], pt[1], E.one())
        words += pyref.ext_to_abi(F, X) + pyref.ext_to_abi(F, Y) + pyref.ext_to_abi(F, Z)
    return (u64 * len(words))(*words)


def fold_result(cid, out):
    C = pyref.CURVES[R.CURVE_NAMES[cid]]
    v, k = [int(x) for x in out], C.deg
    X, Y, Z = (pyref.ext_from_abi(C.F, v[12 * k * j:12 * k * (j + 1)], k) for j in range(3))
    return C.proj_to_affine(X, Y, Z)


@pytest.mark.parametrize("tpw, cid, lean", [(64, 0, False), (64, 2, True), (64, 0, True), (32, 1, False), (16, 3, False)])
def test_model_through_both_levels_and_the_fold_is_the_msm(tpw, cid, lean):
    """sum s_i b_i over the integers mod r: buckets from digits, the model's level 1, the model's level 2 over what level 1
    wrote, the host fold of msm_fold.h (generic, and the lean re-slot) over what level 2 wrote"""
    rnd = random.Random(31 * tpw + cid + lean)
    r = form(cid).r
    sw = tpw.bit_length() - 1
    for W, Q, L1, L2, c, top in ((1, tpw + 3, 1, 2, 9, 0), (2, 5 * tpw + 1, 2, 3, 11, 0), (3, 3 * tpw * 4, 4, 5, 12, 1), (2, 17, 16, 1, 8, 1)):
        n = 60
        b = draw(rnd, n, 1, 50)
        digits = [[rnd.randrange(Q) for _ in range(W)] for _ in range(n)]
        in_top = [rnd.randrange(2) for _ in range(n)]
        B = [[0] * Q for _ in range(W)]
        s = [0] * n
        for i in range(n):
            for w in range(W):
                if top and w == W - 1:
                    if in_top[i]:                     # the top window's slot k is digit k + 2^(c-1) of window W - 2
                        B[w][digits[i][w]] += b[i]
                        s[i] += (digits[i][w] + (1 << (c - 1))) << (c * (W - 2))
                else:
                    B[w][digits[i][w]] += b[i]
                    s[i] += digits[i][w] << (c * w)
        buckets = [v for row in B for v in row]
        segs = (Q + tpw * L1 - 1) // (tpw * L1)
        if lean:
            l1 = R.Launch([R.In(1, 0, Q, 2, W * Q)], W * segs, segs, L1, 64)
            lane_out = l1.expect(buckets, r)
            assert sorted(lane_out) == list(range(W * segs * 128))
            mid = [lane_out[k] for k in range(W * segs * 128)]
            l2 = R.Launch([R.In(2, 0, segs * 64, 0), R.In(2, 1, segs * 64, 1)], W, 1, segs, 64)
        else:
            l1 = R.Launch([R.In(1, 0, Q, 0, W * Q)], W * segs, segs, L1, tpw)
            seg_out = l1.expect(buckets, r)
            assert sorted(seg_out) == list(range(W * segs * 3))
            mid = [seg_out[k] for k in range(W * segs * 3)]
            assert tpw * L2 >= segs
            l2 = R.Launch([R.In(3, 0, segs, 0), R.In(3, 1, segs, 1), R.In(3, 2, segs, 1)], W, 1, L2, tpw)
        win = l2.expect(mid, r)
        pts = abi_points(cid, [win.get(k, 7) for k in range(9 * W)])      # rows level 2 does not write: never read, any value
        out = (u64 * (36 * form(cid).k))()
        assert host_shim().t_fold(cid, 1 if lean else 0, pts, W, c, sw + L1.bit_length() - 1, sw, top, 0, out) == 0
        assert fold_result(cid, out) == group(cid, 1).point(sum(si * bi for si, bi in zip(s, b)) % r), (W, Q, L1, L2, c, top)


def test_flat_addressing_and_heavy_combine_definition():
    i = R.In(3, 2, 7, 1)
    assert [i.flat(0, 0), i.flat(0, 6), i.flat(1, 0), i.flat(2, 3)] == [2, 20, 23, 53]
    la = strided(16, 1, 2, 7, (0, 1, 1))
    assert la.reads() == set(range(42)) and la.out_rows() == 18
    assert sorted(la.expect(list(range(42)), 1000)) == [0, 1, 2, 3, 4, 5, 6, 9, 12, 15]
    assert R.heavy_combine([1, 2, 3, 4, 5, 6], [4, 0, 2], [0, 1, 3, 6], 11) == {4: 1, 0: 5, 2: 4}


@pytest.mark.parametrize("tpw, cid", [(64, 0), (64, 2), (32, 1), (16, 3)])
def test_operand_sets_hold_the_collisions_they_are_named_for(tpw, cid):
    """every set is found by find(), which takes a seed only when the replay shows the named collision and no other; here the
    statement is made again for the finished list, and the list's coverage is asserted: a detour at ITEM and at WACC, at every
    offset of TREE_WACC, SCAN and TREE_RUN in mode 0 and of TREE_RUN in mode 1, each for one pair alone and for all pairs"""
    r = form(cid).r
    sets = sets_for(tpw, cid)
    seen, salts = {}, set()
    for s in sets:
        assert s.holds(tpw, r) is None
        for st in s.steps(tpw, r):
            if st.detour:
                key = (s.mode, st.kind, 0 if st.kind in (ITEM, WACC) else st.off)
                seen[key] = max(seen.get(key, 0), len(st.detour))
                salts.update((pg, sid) for pg, sid in st.detour.items() if s.t == 1)
                if st.inf:
                    seen["detour next to an infinite operand"] = 1
                if st.detour_inf:
                    seen["infinity inside a detour"] = 1
    offs = [tpw >> (k + 1) for k in range(tpw.bit_length() - 1)]
    modes = (0, 1, 2) if tpw == 64 else (0, 1)
    need = [(m, ITEM, 0) for m in modes] + [(m, WACC, 0) for m in modes if m != 1]
    need += [(0, k, off) for k in (TREE_WACC, SCAN, TREE_RUN) for off in offs] + [(1, TREE_RUN, off) for off in offs]
    need += ["detour next to an infinite operand", "infinity inside a detour"]
    assert [k for k in need if k not in seen] == []
    assert {sid for _, sid in salts} == {0, 1}                       # both salts are taken
    names = [s.name for s in sets]
    assert len(set(names)) == len(names)
    for off in offs:                                                 # all pairs: as many groups as the step has pairs
        assert seen[(0, TREE_WACC, off)] == off and seen[(0, SCAN, off)] == tpw - off and seen[(1, TREE_RUN, off)] == off
        assert seen[(0, TREE_RUN, off)] == (off - 1 if off == tpw // 2 else off)
    # the random baseline claims no collision
    for c in shape_cases(tpw, 3)[-2:]:
        la = c.launch
        for gb in range(la.programs()):
            _, w, item0, _ = la.segment(gb)
            seg = [m for m in c.mult[w * la.ins[0].count + item0:(w + 1) * la.ins[0].count][:tpw * la.L]]
            assert R.collisions(R.replay(host_shim(), 0, la.L, tpw, seg, r, BASE_T)[3]) == {}


@pytest.mark.parametrize("build", list(BUILDS))
def test_every_address_is_inside_its_buffer(build):
    """what Reduce.check allocates -- len(mult) input slots, out_rows() + 1 output rows, programs() slabs + 64 words -- holds
    every address the kernel forms: validated here for every case, and again by check() before each launch"""
    b = BUILDS[build]
    for c in all_cases(build):
        la = c.launch
        c.validate(len(c.mult), la.out_rows(), la.programs())
        assert la.tpw == b["tpw"]
        want = la.expect(c.mult, form(b["cid"]).r)
        assert all(0 <= row < la.out_rows() for row in want)
        for i in la.ins:                     # the largest index the kernel can form, by its own formula
            w_max = (la.per_input - 1) // la.segs
            k_max = min(i.count, la.segs * la.tpw * la.L) - 1
            reach = (w_max * i.count + k_max) * i.stride + i.offset
            assert reach < len(c.mult)


def all_cases(build):
    b = BUILDS[build]
    tpw = b["tpw"]
    rnd = random.Random(5)
    out = [c for L in LS for c in shape_cases(tpw, L)] + valid_cases(tpw) + strided_cases(tpw)
    if b["waves"]:
        out += lean_cases()
    return out + [set_case(s, tpw, rnd) for s in sets_for(tpw, b["cid"])]


def heavy_case(cid):
    """heavy buckets of 1, 2, 63, 64, 65 and 129 chunk sums, a non-identity order into 10 buckets; the partials hold infinity,
    P and -P side by side, and equal points a lane meets in a row (k and k + 64) and the tree meets (lanes l and l + 32)"""
    rnd = random.Random(600 + cid)
    sizes = (1, 2, 63, 64, 65, 129)
    order = [7, 2, 9, 0, 4, 5]
    chunk_start = [0]
    for s in sizes:
        chunk_start.append(chunk_start[-1] + s)
    partials = draw(rnd, chunk_start[-1], 1, 1 << 14)
    at = chunk_start[:-1]
    partials[at[1]:at[1] + 2] = [33, 33]                      # two equal chunk sums: the tree doubles
    partials[at[2] + 3], partials[at[2] + 35] = 41, 41        # lanes 3 and 35 hold equal sums at the tree's first step
    partials[at[3] + 5], partials[at[3] + 6] = 0, 0           # infinity
    partials[at[3] + 10], partials[at[3] + 42] = 77, -77      # P, -P across the tree
    partials[at[4]], partials[at[4] + 64] = 55, 55            # a lane adds the point it holds: proj_add_call doubles inline
    partials[at[5] + 1], partials[at[5] + 65] = 91, -91       # a lane's sum returns to infinity, then takes chunk 129
    partials[at[5] + 128] = 0
    return partials, order, chunk_start


def test_heavy_case_is_what_it_says():
    for cid in range(4):
        p, order, cs = heavy_case(cid)
        assert [cs[h + 1] - cs[h] for h in range(6)] == [1, 2, 63, 64, 65, 129] and order != sorted(order) and len(set(order)) == 6
        assert max(order) < 10 and len(p) == cs[-1] and 0 in p and any(-m in p for m in p if m)
        want = R.heavy_combine(p, order, cs, form(cid).r)
        assert sorted(want) == sorted(order) and want[7] == p[0] and want[2] == 66


# ------------------------------------------------------------------ the card
def run_cases(dev, build, cases):
    fails = []
    for c in cases:
        fails += dev.check(build, c)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("build", list(BUILDS))
def test_gpu_shapes(dev, build, L):
    """one input in mode 0 over random items: every count of {1, TPW-1, TPW, TPW+1, TPW L-1, TPW L, TPW L+1, 2 TPW L+TPW+1}
    (segs 1, 2 and 3, ragged last segments, groups without items), one and three windows"""
    run_cases(dev, build, shape_cases(BUILDS[build]["tpw"], L))


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_gpu_valid_forms(dev, build):
    """valid at the start of the last window's last segment (its slots hold 0xFF.. and the rows must be exact proj_zero) and inside
    that segment (the slots behind it hold infinity)"""
    run_cases(dev, build, valid_cases(BUILDS[build]["tpw"]))


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_gpu_level2_inputs(dev, build):
    """three inputs (0, 1, 1) at stride 3 and two (0, 1) at stride 2 over one buffer, L = 1, 2, 3, 5; the rows a mode-1 program
    leaves alone (gb 3 + 1, gb 3 + 2) keep the fill"""
    run_cases(dev, build, strided_cases(BUILDS[build]["tpw"]))


@pytest.mark.gpu
@pytest.mark.parametrize("build", [b for b in BUILDS if BUILDS[b]["waves"]])
def test_gpu_lean_mode(dev, build):
    """mode 2 (the G1 kernel only): every lane's (run, wacc); run_if null, all ones and mixed -- the rows of a program with
    run_if = 0 keep the fill; an all-padding program writes proj_zero to its 128 rows"""
    run_cases(dev, build, lean_cases())


@pytest.mark.gpu
@pytest.mark.parametrize("part", ["tree", "scan", "treerun", "tree1", "serial"])
@pytest.mark.parametrize("build", list(BUILDS))
def test_gpu_operand_sets(dev, build, part):
    """the sets of sets_for(): the salt detour at every step kind and tree offset, next to infinite operands, with both salts"""
    b = BUILDS[build]
    rnd = random.Random(11)
    sets = [s for s in sets_for(b["tpw"], b["cid"]) if (s.name.split("_")[0] == part) or (part == "serial" and " mode " in s.name)]
    assert sets
    run_cases(dev, build, [set_case(s, b["tpw"], rnd) for s in sets])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", range(4))
def test_gpu_heavy_combine(dev, cid):
    f, G = form(cid), group(cid, BASE_T)
    partials, order, chunk_start = heavy_case(cid)
    n_heavy, total = len(order), 10
    assert max(order) < total and chunk_start[-1] == len(partials) and len(chunk_start) == n_heavy + 1
    rows = G.item_rows(partials, random.Random(cid))
    with Bufs(dev.card) as B:
        a_p, a_o, a_c = B.put(rows), B.put(np.array(order, dtype=np.uint32)), B.put(np.array(chunk_start, dtype=np.uint32))
        a_b = B.filled((total + 1) * f.proj_words)
        dev.run(cid, "rd_heavy_combine", cid, a_p, a_o, a_c, n_heavy, a_b)
        out = B.get(a_b, (total + 1) * f.proj_words).reshape(total + 1, f.proj_words)
    fails = compare_rows(G, out, R.heavy_combine(partials, order, chunk_start, f.r))
    assert not fails, fails
