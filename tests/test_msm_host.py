"""The MSM's HIP-free host code compiled with g++ (tests/host_shim/msm_host_shim.cpp): the window folds of
ginger-lib_amd/csrc/msm_fold.h against their definition, computed from Python integers, the plans of msm_plan.h (one MSM,
its bucket sort, its affine rounds) against the invariants the launch sequence relies on and the values the project documents,
the bucket accumulation's task decode (msm_schedule.h) against an enumeration, and the bucket reduction's step schedule
(msm_schedule.h) run over integers against the sums the wave program promises.
Nothing here is a recording of the code's own output."""
import ctypes

import pytest

import pyref
import shim_build

U64 = ctypes.c_uint64
CURVE_NAMES = ("mnt4753_g1", "mnt4753_g2", "mnt6753_g1", "mnt6753_g2")


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("msm_host")
    for f in (lib.t_auto_window, lib.t_precompute_window):
        f.argtypes = [U64, ctypes.c_int, ctypes.c_int]
    lib.t_plan_msm.argtypes = [U64] + [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int64)]
    lib.t_plan_sort.argtypes = [U64, U64, U64, ctypes.POINTER(ctypes.c_uint32)]
    lib.t_tree_plan.argtypes = [ctypes.c_uint32, U64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, U64, U64, ctypes.POINTER(U64)]
    lib.t_tree_piece.argtypes = [ctypes.c_uint32] * 5 + [ctypes.c_int, ctypes.POINTER(U64)]
    lib.t_acc_task.argtypes = ([ctypes.c_int, ctypes.c_uint32] + [ctypes.POINTER(ctypes.c_uint32)] * 4 + [ctypes.c_uint32] * 5
                               + [ctypes.POINTER(ctypes.c_uint32)])
    lib.t_wave_step.argtypes = [ctypes.c_uint32] + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    lib.t_wave_step_active.argtypes = [ctypes.c_int] * 5
    return lib


# ------------------------------------------------------------------------------------------------ folds

class FoldCase:
    """Window sums as small multiples k G of the generator (k = 0: infinity), in random projective representatives; the fold's
    result must be (the definition's integer combination of the k) G."""

    def __init__(self, cid, seed):
        self.cid = cid
        self.C = pyref.CURVES[CURVE_NAMES[cid]]
        self.F, self.E, self.k = self.C.F, self.C.E, self.C.deg
        self.rng = pyref.Rng(seed)
        self.small = {0: None}

    def multiple(self, m):
        if m not in self.small:
            self.small[m] = self.C.mul(m, self.C.G)
        return self.small[m]

    def proj_limbs(self, m):
        Pt, E, F = self.multiple(m), self.E, self.F
        if Pt is None:
            X, Y, Z = E.zero(), tuple(self.rng.field_elem(F.p) for _ in range(self.k)), E.zero()     # any (0 : y : 0)
            if self.rng.next_u64() & 1:
                X, Y = E.zero(), E.one()
        else:
            z = tuple(self.rng.field_elem(F.p) for _ in range(self.k))
            X, Y, Z = E.mul(Pt[0], z), E.mul(Pt[1], z), z
        return pyref.ext_to_abi(F, X) + pyref.ext_to_abi(F, Y) + pyref.ext_to_abi(F, Z)

    def pack(self, RW, T, PW, PS, PA, PB):
        """the layout the reduction writes: point (which * RW + w) * 3 + k; which 0: (T, PW, PS), 1: PA at k = 0, 2: PB at k = 0"""
        per = 36 * self.k
        buf = (U64 * (9 * RW * per))()
        filler = 7          # the two unused points behind PA and PB: never read, so any value
        for w in range(RW):
            pts = {(0, 0): T[w], (0, 1): PW[w], (0, 2): PS[w], (1, 0): PA[w], (1, 1): filler, (1, 2): filler,
                   (2, 0): PB[w], (2, 1): filler, (2, 2): filler}
            for (which, k), m in pts.items():
                base = ((which * RW + w) * 3 + k) * per
                for i, v in enumerate(self.proj_limbs(m)):
                    buf[base + i] = v
        return buf

    def result(self, out):
        v, k, F = [int(x) for x in out], self.k, self.F
        X, Y, Z = (pyref.ext_from_abi(F, v[12 * k * j:12 * k * (j + 1)], k) for j in range(3))
        if all(c == 0 for c in Z):
            assert all(c == 0 for c in X) and Y == self.E.one()          # the canonical (0, 1, 0)
            return None
        return self.C.proj_to_affine(X, Y, Z)

    def expect(self, scalar):
        return self.C.mul(scalar, self.C.G) if scalar else None


def window_value(u, sw, PW, PS, PA, PB, w):
    return (PW[w] << (u + sw)) + (PS[w] << u) + (PA[w] << sw) + PB[w]


def draw(rng, count, kind):
    if kind == "zero":
        return [0] * count
    if kind == "sparse":
        return [int(rng.next_u64() % 40) if rng.next_u64() % 3 == 0 else 0 for _ in range(count)]
    return [1 + int(rng.next_u64() % 40) for _ in range(count)]


# (W, c, L1, top_unsigned): one, two and three windows, and the per-window path's typical shapes (c = 16 divides 752)
GENERIC_SHAPES = [(1, 13, 16, 0), (2, 16, 32, 0), (2, 16, 32, 1), (3, 7, 4, 0), (3, 16, 32, 1), (48, 16, 32, 1), (58, 13, 16, 0)]


@pytest.mark.parametrize("cid", range(4))
def test_fold_generic_against_definition(shim, cid):
    fc = FoldCase(cid, 900 + cid)
    sw = {1: 6, 2: 5, 3: 4}[fc.k]
    out = (U64 * (36 * fc.k))()
    for W, c, L1, top in GENERIC_SHAPES:
        u = sw + L1.bit_length() - 1
        for kind in ("dense", "sparse", "zero", "equal"):
            T, PW, PS, PA, PB = (draw(fc.rng, W, "dense" if kind == "equal" else kind) for _ in range(5))
            if kind == "equal":
                # PS_w = 2^sw PW_w: when the fold adds PS it holds exactly that point (the addition's doubling branch);
                # the windows above contribute nothing so that this also holds below the top window
                PW, PS = [3] * W, [3 << sw] * W
                T, PA, PB = [0] * W, [0] * W, [0] * W
                if W > 1:
                    PW[1:], PS[1:] = [0] * (W - 1), [0] * (W - 1)
            assert shim.t_fold(cid, 0, fc.pack(W, T, PW, PS, PA, PB), W, c, u, sw, top, 0, out) == 0
            if top:
                s = sum(window_value(u, sw, PW, PS, PA, PB, w) << (c * w) for w in range(W - 2))
                s += (window_value(u, sw, PW, PS, PA, PB, W - 2) + window_value(u, sw, PW, PS, PA, PB, W - 1)
                      + (T[W - 1] << (c - 1))) << (c * (W - 2))
            else:
                s = sum(window_value(u, sw, PW, PS, PA, PB, w) << (c * w) for w in range(W))
            assert fc.result(out) == fc.expect(s), (W, c, L1, top, kind)


# (sets, pseudo-windows per set, c, q, L1): a full table below and above 2^15 slots, and the partial tables' 3 and 8 sets
MERGED_SHAPES = [(1, 1, 13, 12, 4), (1, 32, 21, 15, 16), (3, 32, 21, 15, 16), (8, 32, 21, 15, 32), (3, 1, 16, 15, 8), (8, 2, 17, 15, 8)]


@pytest.mark.parametrize("cid", range(4))
def test_fold_merged_against_definition(shim, cid):
    fc = FoldCase(cid, 950 + cid)
    sw = {1: 6, 2: 5, 3: 4}[fc.k]
    out = (U64 * (36 * fc.k))()
    for sets, Wp, c, q, L1 in MERGED_SHAPES:
        u = sw + L1.bit_length() - 1
        RW = sets * Wp
        for kind in ("dense", "sparse", "zero", "equal"):
            T, PW, PS, PA, PB = (draw(fc.rng, RW, "dense" if kind == "equal" else kind) for _ in range(5))
            if kind == "equal":      # every pseudo-window the same point in every array: the running sums double
                T, PW, PS, PA, PB = ([5] * RW for _ in range(5))
            assert shim.t_fold(cid, 2, fc.pack(RW, T, PW, PS, PA, PB), RW, c, u, sw, sets, q, out) == 0
            s = 0
            for g in range(sets):
                ws = range(g * Wp, (g + 1) * Wp)
                S = sum(window_value(u, sw, PW, PS, PA, PB, w) for w in ws)
                S += sum((w - g * Wp) * T[w] for w in ws) << q
                S += sum(T[w] for w in ws)
                s += S << (c * g)
            assert fc.result(out) == fc.expect(s), (sets, Wp, c, q, L1, kind)


@pytest.mark.parametrize("cid", [0, 2])
def test_lean_reslot_against_definition(shim, cid):
    """the lane-level reduction delivers (T, A2, Bv2) and PA' per window: R_w = 64 PA' + 64 L1 A2 + Bv2"""
    fc = FoldCase(cid, 990 + cid)
    out = (U64 * 36)()
    for W, c, L1, top in GENERIC_SHAPES:
        u = 6 + L1.bit_length() - 1
        for kind in ("dense", "sparse", "zero"):
            T, A2, Bv2, PAp = (draw(fc.rng, W, kind) for _ in range(4))
            junk = draw(fc.rng, W, "dense")            # the third array is not written by the lean form
            assert shim.t_fold(cid, 1, fc.pack(W, T, A2, Bv2, PAp, junk), W, c, u, 6, top, 0, out) == 0
            R = [64 * PAp[w] + 64 * L1 * A2[w] + Bv2[w] for w in range(W)]
            if top:
                s = sum(R[w] << (c * w) for w in range(W - 2)) + ((R[W - 2] + R[W - 1] + (T[W - 1] << (c - 1))) << (c * (W - 2)))
            else:
                s = sum(R[w] << (c * w) for w in range(W))
            assert fc.result(out) == fc.expect(s), (W, c, L1, top, kind)


# ------------------------------------------------------------------------------------------------ plans

PLAN_FIELDS = ("status merged c W top_unsigned sets nb entries total RW Q segs tpw sw L1 L2 lean lane_buf tree heavy_thr heavy_chunk "
               "max_heavy max_chunks fold_u fold_lq").split()


def plan(shim, n, deg, table=False, pre_c=0, pre_G=1, solo=True, last=True, override=0, mode=2):
    out = (ctypes.c_int64 * 25)()
    shim.t_plan_msm(n, deg, int(table), pre_c, pre_G, int(solo), int(last), override, mode, out)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def sizes():
    ns = set()
    for lg in range(0, 27):
        ns.update(v for v in ((1 << lg) - 1, 1 << lg, (1 << lg) + 1) if 1 <= v <= 1 << 26)
    return sorted(ns)


def heavy_plan(hist, thr, chunk):
    """what the sort stage's heavy plan makes of a bucket histogram: buckets above the threshold, cut into chunks"""
    heavy = [(s, m) for s, m in hist if s > thr]
    return sum(m for _, m in heavy), sum(m * ((s + chunk - 1) // chunk) for s, m in heavy)


def check_plan(p, n, deg, merged, pre_G, solo, last, mode):
    c, W = p["c"], p["W"]
    assert p["merged"] == int(merged)
    assert W == 752 // c + 1
    assert p["top_unsigned"] == int(not merged and 752 % c == 0 and W >= 2)
    assert p["sets"] == (pre_G if merged else W)
    assert p["nb"] == (1 << (c - 1)) + (0 if merged else 1)
    assert p["entries"] == W * n and p["total"] == p["sets"] * p["nb"]
    assert p["RW"] * p["Q"] == p["total"]                       # no padding slots behind the last pseudo-window, ever
    assert p["Q"] <= 1 << 15 or not merged
    tpw, L1, segs = p["tpw"], p["L1"], p["segs"]
    assert tpw == {1: 64, 2: 32, 3: 16}[deg] and 1 << p["sw"] == tpw
    assert L1 in (4, 8, 16, 32)
    assert segs * tpw * L1 >= p["Q"] > (segs - 1) * tpw * L1
    assert p["L2"] * tpw >= segs
    assert 1 << p["fold_u"] == tpw * L1
    assert 1 << p["fold_lq"] >= p["Q"] > (1 << p["fold_lq"]) >> 1
    # one wave program per SIMD where the bucket array allows it: a shorter segment only if the launch stays within 1024 programs
    if L1 < 16:
        assert p["RW"] * segs <= 1024
    assert p["lean"] == int(deg == 1 and not solo and not last and W * n >= 1 << 25)
    assert p["lane_buf"] >= p["lean"]
    too_large = W * n >= 1 << 31 or p["total"] >= 1 << 31
    assert p["status"] == int(too_large)
    if too_large:
        return
    assert p["tree"] == int(mode == 1 or (mode == 2 and deg >= 2 and W * n >= 1 << 21))
    thr, chunk, entries = p["heavy_thr"], p["heavy_chunk"], p["entries"]
    assert 128 <= thr <= 1024 and chunk == thr
    # upper bounds of the heavy plan for any histogram of `entries` list entries: everything in one bucket; as many buckets just
    # above the threshold as there can be (with and without the remainder on top of one); half and half
    # (as (bucket size, how many such buckets) pairs)
    few = entries // (thr + 1)
    hists = [[(entries, 1)], [(thr + 1, few), (entries - few * (thr + 1), 1)]]
    if few:
        hists.append([(thr + 1, few - 1), (thr + 1 + entries - few * (thr + 1), 1)])
        hists.append([(thr + 1, few // 2), (entries - (few // 2) * (thr + 1), 1)])
    for hist in hists:
        assert sum(s * m for s, m in hist) == entries
        n_heavy, n_chunks = heavy_plan(hist, thr, chunk)
        assert n_heavy <= p["max_heavy"] and n_chunks <= p["max_chunks"]


def test_plan_invariants(shim):
    for n in sizes():
        for deg in (1, 2, 3):
            for solo, last in ((True, True), (False, False), (False, True)):
                for c in range(2, 25):
                    mode = (c + deg) % 3
                    check_plan(plan(shim, n, deg, solo=solo, last=last, override=c, mode=mode), n, deg, False, 1, solo, last, mode)
                    for pre_G in (1, 2, 3, 8):
                        check_plan(plan(shim, n, deg, True, c, pre_G, solo, last, 0, mode), n, deg, True, pre_G, solo, last, mode)
    # a window override that is not the table's: the key runs on the per-window path at that window
    p = plan(shim, 1 << 20, 1, True, 21, 1, override=16)
    assert (p["merged"], p["c"]) == (0, 16)
    p = plan(shim, 1 << 20, 1, True, 21, 1, override=21)
    assert (p["merged"], p["c"]) == (1, 21)
    # without an override the window is auto_window's
    for n in sizes():
        for deg in (1, 2, 3):
            p = plan(shim, n, deg)
            assert p["c"] == shim.t_auto_window(n, deg, 0)
            check_plan(p, n, deg, False, 1, True, True, 2)


def test_plan_refuses_what_31_bit_entries_cannot_hold(shim):
    for c, deg in ((2, 1), (13, 1), (16, 2), (24, 3)):
        W = 752 // c + 1
        edge = -(-(1 << 31) // W)            # the smallest n with W n >= 2^31
        assert plan(shim, edge - 1, deg, override=c)["status"] == 0
        assert plan(shim, edge, deg, override=c)["status"] == 1
        assert plan(shim, edge, deg, True, c, 1)["status"] == 1


def test_documented_windows(shim):
    for lg, c in ((15, 13), (20, 16), (21, 18), (23, 19)):
        assert shim.t_auto_window(1 << lg, 1, 0) == c
    for lg in range(0, 30):
        for n in ((1 << lg), (1 << (lg + 1)) - 1):
            assert shim.t_auto_window(n, 2, 0) == shim.t_auto_window(n, 3, 0) == min(20, max(4, lg - 4))
            assert shim.t_auto_window(n, 1, 17) == 17 and shim.t_precompute_window(n, 2, 9) == 9
    for lg, c in ((10, 18), (17, 18), (18, 20), (19, 21), (22, 21), (23, 23), (26, 23)):
        assert shim.t_precompute_window(1 << lg, 1, 0) == c
        assert shim.t_precompute_window((1 << (lg + 1)) - 1, 1, 0) == c
    for lg, c in ((10, 18), (18, 18), (19, 19), (21, 19), (22, 21), (26, 21)):
        assert shim.t_precompute_window(1 << lg, 2, 0) == shim.t_precompute_window(1 << lg, 3, 0) == c


def test_documented_plans(shim):
    # 2^20 G1 pairs with a full table at c = 21: one set of 2^20 slots in 32 pseudo-windows, exactly 1024 level-1 programs
    p = plan(shim, 1 << 20, 1, True, 21, 1)
    assert (p["sets"], p["total"], p["RW"], p["L1"], p["RW"] * p["segs"], p["L2"]) == (1, 1 << 20, 32, 16, 1024, 1)
    # the same key without a table
    p = plan(shim, 1 << 20, 1)
    assert (p["c"], p["W"], p["top_unsigned"], p["L1"]) == (16, 48, 1, 32)
    assert [shim.t_const(i) for i in range(6)] == [16, 1024, 1026, 2048, 4096, 26]


def test_sort_plan(shim):
    out = (ctypes.c_uint32 * 5)()
    for n in sizes():
        for c in (4, 13, 16, 19, 21, 24):
            W = 752 // c + 1
            for total in (W * ((1 << (c - 1)) + 1), 1 << (c - 1), 8 << (c - 1)):
                entries = W * n
                if entries >= 1 << 31 or total >= 1 << 31:
                    continue
                shim.t_plan_sort(entries, n, total, out)
                tile, shift, n_bins, n_blocks, part = (int(v) for v in out)
                assert tile in (16384, 65536) and shift >= 8
                assert n_bins << shift >= total > (n_bins - 1) << shift
                assert n_bins <= 1024 or (n_bins <= shim.t_const(3) and shift == 13)
                assert n_blocks * tile >= entries > (n_blocks - 1) * tile
                if part:        # a bin's buckets fit the LDS of one block; every tile is full of one window's... at least n >= tile
                    assert shift <= 13 and n >= tile and entries >= 1 << 22
                else:
                    assert entries < 1 << 22 or n < tile or shift > 13
    # 2^24 pairs per window at c = 19 (40 x 2^18 buckets): the partitioned sort with 2^13-bucket bins
    shim.t_plan_sort(40 << 24, 1 << 24, 40 * ((1 << 18) + 1), out)
    assert (int(out[1]), int(out[4])) == (13, 1) and 1024 < int(out[2]) <= 2048


def test_tree_plan(shim):
    out = (U64 * 6)()
    GB = 1 << 30
    max_rounds, finish_max = shim.t_const(5), 64
    for deg, lanes, left in ((1, 1, 4.5), (2, 2, 2.5), (3, 3, 1.5)):
        for n0 in (1, 1000, 1 << 21, 40 << 20, (1 << 31) - 1):
            for total in (1, 2, 1 << 12, 1 << 20, 1 << 24):
                for maxc in (1, 63, 64, 65, 1 << 12, n0):
                    for free_b, have in ((280 * GB, 0), (20 * GB, 8 * GB), (4 * GB, 0), (3 * GB, GB // 8), (GB, 0)):
                        shim.t_tree_plan(n0, total, maxc, deg, lanes, free_b, have, out)
                        R, stride, room, K = (int(v) for v in out[:4])
                        assert 1 <= R <= max_rounds
                        assert maxc >> R <= finish_max or R == max_rounds
                        mean = n0 / max(total - 1, 1)
                        assert (1 << R) * left >= mean or R == max_rounds                # down to `left` points per bucket
                        assert R == 1 or (1 << (R - 1)) * left < mean or maxc >> (R - 1) > finish_max      # and no deeper than needed
                        assert stride % 64 == 0 and total <= stride < total + 64
                        budget = min(64.0 * GB, (free_b + have - 3.0 * GB) * 0.9)
                        assert room == int(budget >= 256 * (1 << 20))
                        if room:
                            need = 430.0 * lanes * n0 * 1.13
                            assert K >= 1 and (K * budget >= need or K == 4096)
                            assert K == 1 or (K - 1) * budget < need
    rng = pyref.Rng(77)
    for tpw in (64, 32, 21):
        for max_waves, asm_max in ((1024, 2048), (2048, 2048), (304 * 4, 304 * 8)):
            ns = [1, tpw, 4 * tpw, 8 * tpw - 1, 8 * tpw, 8 * tpw + 1, asm_max * tpw * 8, asm_max * tpw * 8 + 1, (1 << 31) - 1]
            ns += [1 + int(rng.next_u64() % (1 << 30)) for _ in range(40)]
            for n_piece in ns:
                for aff_asm in (0, 1):
                    o0 = 4 * tpw * int(rng.next_u64() % 1000)
                    shim.t_tree_piece(n_piece, o0, tpw, max_waves, asm_max, aff_asm, out)
                    t0, waves, aw, Bq, nA, split = (int(v) for v in out)
                    assert t0 * tpw == o0
                    assert waves % 4 == 0 and 4 <= waves <= max_waves
                    assert aw % 4 == 0 and 4 <= aw <= asm_max
                    assert Bq >= 8 and aw * tpw * Bq >= n_piece
                    assert waves * tpw * 8 >= n_piece or waves == max_waves
                    assert nA % (4 * tpw) == 0 and 0 <= nA - n_piece // 2 < 4 * tpw
                    if split:       # only the assembly rounds, only with two non-empty halves and a batch of 32 per lane group in one piece
                        assert aff_asm and 0 < nA < n_piece and n_piece > 31 * asm_max * tpw
                    else:
                        assert not aff_asm or nA >= n_piece or n_piece <= 31 * asm_max * tpw


# ------------------------------------------------------------------------------------------------ the accumulation's task decode

def u32_array(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


def test_acc_task_decode_against_enumeration(shim):
    out = (ctypes.c_uint32 * 4)()
    # (bucket sizes, heavy threshold = chunk): no heavy bucket; one whose last chunk is short; exact multiples of the chunk; all heavy
    cases = [([3, 0, 7, 1, 5], 8), ([3, 21, 0, 2], 8), ([16, 1, 8, 24, 0, 9], 8), ([5, 4, 1], 4), ([9, 10, 17], 4), ([1], 1), ([2], 1)]
    for sizes_, chunk in cases:
        total = len(sizes_)
        starts = [sum(sizes_[:g]) for g in range(total)]
        order = sorted(range(total), key=lambda g: (-min(sizes_[g], chunk + 1), g))     # by descending size bin: the heavy ones first
        n_heavy = sum(1 for c in sizes_ if c > chunk)
        chunk_start, expect = [], []
        for h in range(n_heavy):                                                        # the enumeration: chunk after chunk
            g = order[h]
            chunk_start.append(len(expect))
            for b in range(0, sizes_[g], chunk):
                expect.append((starts[g] + b, min(chunk, sizes_[g] - b), len(expect), 1))
        chunk_start.append(len(expect))
        n_chunks = len(expect)
        expect += [(starts[g], sizes_[g], g, 0) for g in order[n_heavy:]]
        assert len(expect) == n_chunks + total - n_heavy
        a = [u32_array(v) for v in (starts, sizes_, order, chunk_start)]
        for t, want in enumerate(expect):
            shim.t_acc_task(0, t, a[0], a[1], a[2], a[3], n_heavy, n_chunks, chunk, 0, 0, out)
            assert tuple(int(v) for v in out) == want, (sizes_, chunk, t)
        assert sorted(e for b, c, _, _ in expect for e in range(b, b + c)) == list(range(sum(sizes_)))   # every list entry once
        # the affine rounds' output list: task t is bucket g_first + t, its records start at starts[g] - list_base
        for g_first in range(total):
            for t in range(total - g_first):
                g = g_first + t
                shim.t_acc_task(1, t, a[0], a[1], a[2], a[3], n_heavy, n_chunks, chunk, g_first, starts[g_first], out)
                assert tuple(int(v) for v in out) == (starts[g] - starts[g_first], sizes_[g], g, 0)


# ------------------------------------------------------------------------------------------------ the reduction's step schedule

def run_wave_schedule(shim, mode, L, TPW, items):
    """The decoded schedule over integers for points: every group has run and wacc, the exchange is a list, group g owns the
    segment's items g, g + TPW, ...; items past the end are padding.  Returns (run, wacc, the published runW)."""
    LT = TPW.bit_length() - 1
    out = (ctypes.c_int * 6)()
    shim.t_wave_step(mode, L, LT, 0, out)
    ns1, nst = out[0], out[1]
    assert ns1 == (L if mode == 1 else 2 * L - 1) and nst == ns1 + (LT if mode == 1 else (0 if mode == 2 else 3 * LT))
    run, wacc, published = [0] * TPW, [0] * TPW, []
    for step in range(nst):
        shim.t_wave_step(mode, L, LT, step, out)
        kind, off, i, publish = out[2], out[3], out[4], out[5]
        if publish:                                  # runW leaves the program, group 0 leaves the last tree
            published.append(run[0])
            run[0] = 0
        exch = list(wacc if kind == 2 else run)      # what the groups put into the exchange before the step
        for g in range(TPW):
            k = g + TPW * i
            if not shim.t_wave_step_active(kind, off, g, TPW, int(k < len(items))):
                continue
            if kind == 0:
                run[g] += items[k]
            elif kind == 1:
                wacc[g] += run[g]
            elif kind == 2:
                wacc[g] += exch[g + off]
            else:
                assert kind in (3, 4)
                run[g] += exch[g + off]
    assert len(published) == (1 if mode == 0 else 0)
    return run, wacc, (published[0] if published else None)


def test_wave_schedule_over_integers(shim):
    rng = pyref.Rng(0x5C4ED)
    for TPW in (64, 32, 16):
        for mode in ((0, 1, 2) if TPW == 64 else (0, 1)):
            for L in (1, 2, 4, 16, 32):
                seg_items = TPW * L
                # a window of 2 full segments, a ragged third and a fourth of padding only; and one shorter than a segment
                for count, n_segs in ((2 * seg_items + max(1, seg_items // 3), 4), (max(1, seg_items - 1), 2), (1, 1)):
                    window = [1 + int(rng.next_u64() % 1000) for _ in range(count)]
                    for seg in range(n_segs):
                        items = window[seg * seg_items:(seg + 1) * seg_items]
                        run, wacc, runW = run_wave_schedule(shim, mode, L, TPW, items)
                        total = sum(items)
                        weighted = sum(k * x for k, x in enumerate(items))
                        where = (TPW, mode, L, count, seg)
                        if mode == 0:       # out[0] = runW, out[1] = A = wacc of group 0, out[2] = Bv = run of group 0
                            assert runW == total, where
                            assert TPW * wacc[0] + run[0] == weighted, where
                        elif mode == 1:
                            assert run[0] == total, where
                        else:               # every lane's (sum_i x, sum_i i x) over its own items g + TPW i
                            for g in range(TPW):
                                own = items[g::TPW]
                                assert (run[g], wacc[g]) == (sum(own), sum(i * x for i, x in enumerate(own))), where + (g,)
