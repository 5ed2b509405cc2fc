"""The MSM's sort stage on the card, kernel by kernel: the integer kernels of ginger-lib_amd/csrc/msm_kernels.h (digits and
histogram with wave_agg_inc, scatter, the partitioned sort, the size order and heavy plan, the task table, the equal-bases
kernels) and the three scan kernels of scan_kernels.h, each launched through tests/device_shim/msm_stages.hip with the product's
grid and read back.  The referee is tests/msm_sort_ref.py, a Python-integer model of what the comments of msm_kernels.h and
msm_plan.h promise.  Every comparison is exact; every output buffer starts as 0xFFFFFFFF words (accumulators as zeros, as the
product clears them) and carries a guard word or row behind it that must survive; every index is validated on the host.

Scope: canonical scalars 0 <= s <= r (s = r folds to 0).  Scalars above r are outside the kernel's contract and outside this
file.

The CPU part (no marker) cross-compiles the shim for gfx950, pins the model to what an MSM means -- over the integers mod r as
the group, the weighted bucket sums of every layout and window size must give sum s_i b_i -- and asserts that the operand sets
hold the rows they exist for."""
import ctypes
import functools
import random

import numpy as np
import pytest

import asm_card
import msm_sort_ref as R
import pyref
import shim_build

SO = shim_build.BUILD + "/libmsm_stages.so"
KERNELS = ("msm_digits_kernel", "msm_scatter_kernel", "msm_part_hist_kernel", "msm_part_scatter_kernel", "msm_bin_sort_kernel",
           "msm_size_hist_kernel", "msm_size_scatter_kernel", "msm_heavy_plan_kernel", "msm_acc_tasks_kernel", "msm_base_hash_kernel",
           "msm_dup_verify_kernel", "msm_merge_scalars_kernel", "msm_merge_groups_kernel", "scan_partials_kernel",
           "scan_block_sums_kernel", "scan_final_kernel")
vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
LAUNCHERS = {
    "st_digits": [vp, vp, u64, cint, cint, u32, cint, vp, vp, vp, cint, u32, u32],
    "st_scan": [vp, vp, u64, vp],
    "st_scatter": [vp, u64, cint, u32, u32, vp, vp, cint, u32, u32],
    "st_part_hist": [vp, u64] + [u32] * 8 + [vp],
    "st_part_scatter": [vp, u64] + [u32] * 8 + [vp, vp],
    "st_bin_sort": [vp, vp, u32, u32, u32, u32, vp, vp, vp],
    "st_size_hist": [vp, u64, u32, vp, vp],
    "st_size_scatter": [vp, u64, u32, vp, vp],
    "st_heavy_plan": [vp, vp, vp, vp, u32, u32, vp, vp],
    "st_acc_tasks": [cint, vp, vp, vp, u32, u64, vp, u32, u32, u32, u64, vp, vp],
    "st_base_hash": [cint, vp, vp, u64, vp],
    "st_dup_verify": [cint, vp, vp, u32, vp, vp],
    "st_merge_scalars": [vp, vp, u64, vp, vp, vp, u32, vp, vp],
    "st_merge_groups": [vp, u64, vp, vp, vp, u32, vp, vp],
}

FILL = 0xFFFFFFFF
SIGN = 0x80000000
# the scalar fields: r of MNT4-753 is the base prime of MNT6-753, and the other way round
FIELDS = {"mnt4": pyref.P6.p, "mnt6": pyref.P4.p}
CS = (4, 5, 8, 13, 16, 18, 21, 23)
NS = (1, 63, 64, 65, 255, 256, 257, 1000)
AGG = (0, 1, 12, 64)
SIZE_BINS, PART_MAX_BINS = 1026, 2048              # msm_plan.h MSM_SIZE_BINS, MSM_PART_MAX_BINS
MERGE_GROUPS = (1, 2, 255, 256, 257, 4096, 4097, 8193)


# ------------------------------------------------------------------ the plans (msm_plan.h through the host shim)
@functools.lru_cache(maxsize=None)
def host_shim():
    lib = shim_build.host_shim("msm_host")
    lib.t_plan_msm.argtypes = [u64] + [cint] * 8 + [ctypes.POINTER(ctypes.c_int64)]
    lib.t_plan_sort.argtypes = [u64, u64, u64, ctypes.POINTER(u32)]
    return lib


@functools.lru_cache(maxsize=None)
def plan(n, c, sets=0):
    """plan_msm for n G1 pairs at window c: sets = 0 without a table, else a key with a shift table of `sets` bucket sets"""
    out = (ctypes.c_int64 * 25)()
    host_shim().t_plan_msm(n, 1, int(sets > 0), c, max(sets, 1), 1, 1, 0 if sets else c, 0, out)
    names = "status merged c W top_unsigned sets nb entries total RW Q segs tpw sw L1 L2 lean lane_buf tree heavy_thr".split()
    p = dict(zip(names, (int(v) for v in out)))
    assert p["status"] == 0 and p["c"] == c and p["merged"] == int(sets > 0)
    return p


def layout(c, sets, row_stride=0, n=1000):
    """the model's Layout with W, nb, top_unsigned and sets as plan_msm gives them"""
    p = plan(n, c, sets)
    lay = (R.Layout.merged_sets(c, p["W"], sets, row_stride) if sets else R.Layout.per_window(c, p["W"], p["top_unsigned"]))
    assert (lay.nb, lay.sets, lay.total, lay.top_unsigned) == (p["nb"], p["sets"], p["total"], p["top_unsigned"])
    return lay


# ------------------------------------------------------------------ operands
def no_carry_scalar(c):
    """windows 0 .. W-2 all 2^(c-1): no window carries"""
    W = 752 // c + 1
    return sum((1 << (c - 1)) << (c * w) for w in range(W - 1))


def all_carry_scalar(c):
    """windows 0 .. W-2 all 2^(c-1) + 1: every signed window carries into the next, up to the top one"""
    W = 752 // c + 1
    return sum(((1 << (c - 1)) + 1) << (c * w) for w in range(W - 1))


@functools.lru_cache(maxsize=None)
def scalar_set(field, c):
    """the edge scalars first (fewer than 1000, so that the n = 1000 prefix holds them all), then 2000 seeded random ones"""
    r = FIELDS[field]
    S = [0, 1, 2, (r - 1) // 2, (r + 1) // 2, r - 2, r - 1, r]
    ks = sorted(set(range(0, 753, c)) | set(range(0, 753, 32)) | {736, 751, 752})
    for k in ks:
        S += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    S += [no_carry_scalar(c), all_carry_scalar(c)]
    assert all(0 <= s <= r for s in S) and len(S) < 1000
    rng = pyref.Rng(0x5EED0000 + 64 * c + len(field) + (field == "mnt6"))
    S += [rng.field_elem(r) for _ in range(2000)]
    return S


@functools.lru_cache(maxsize=None)
def digit_table(field, c, top_unsigned):
    """the model's digits of the whole scalar set -> N x W int32"""
    r, W = FIELDS[field], 752 // c + 1
    return np.array([R.digits(s, c, W, top_unsigned, r) for s in scalar_set(field, c)], dtype=np.int32)


def scalar_words(scalars):
    """integers below 2^768 -> len x 24 words"""
    return np.frombuffer(b"".join(int(s).to_bytes(96, "little") for s in scalars), dtype=np.uint32).reshape(len(scalars), 24).copy()


def words_scalar(row):
    return int.from_bytes(np.ascontiguousarray(row, dtype=np.uint32).tobytes(), "little")


def entries(D, lay):
    """the list entries of a digit array D (n x W), window by window as the kernels number them: (bucket, list value) per
    non-zero digit.  The array form of Layout.bucket / Layout.value (test_array_form_against_the_model holds them together)."""
    n, W = D.shape
    w = np.repeat(np.arange(W, dtype=np.int64), n).reshape(W, n)
    i = np.tile(np.arange(n, dtype=np.int64), W).reshape(W, n)
    d = D.T.astype(np.int64)
    nz = d != 0
    w, i, d = w[nz], i[nz], d[nz]
    bucket = (w % lay.sets) * lay.win_stride + np.abs(d) - lay.slot_shift
    value = (i + (w // lay.sets) * lay.row_stride) | np.where(d < 0, SIGN, 0)
    assert bucket.size == 0 or (0 <= bucket.min() and bucket.max() < lay.total and value.max() <= FILL)
    return bucket, value


def histogram(D, lay):
    b, _ = entries(D, lay)
    return np.bincount(b, minlength=lay.total).astype(np.uint32)


def pair_keys(bucket, value):
    return np.sort((np.asarray(bucket).astype(np.uint64) << np.uint64(32)) | np.asarray(value).astype(np.uint64))


def thirteen_key_wave():
    """64 scalars whose window-0 digits take exactly the 13 values 1 .. 13 and whose other windows are empty"""
    return [1 + i % 13 for i in range(64)]


def merge_case(r, seed=41):
    """groups of MERGE_GROUPS members and a pair that cancels, members ascending inside a group and scattered over the key,
    mixed signs, the scalars 0, 1 and r - 1 among the members -> (scalars, starts, members)"""
    rnd = random.Random(seed)
    sizes = list(MERGE_GROUPS) + [2]
    N = sum(sizes) + 500
    perm = list(range(N))
    rnd.shuffle(perm)
    scalars = [rnd.randrange(r) for _ in range(N)]
    starts, members, at = [0], [], 0
    for gsize in sizes:
        idx = sorted(perm[at:at + gsize])
        at += gsize
        members += [idx[0]] + [m | (SIGN if rnd.random() < 0.5 else 0) for m in idx[1:]]
        starts.append(len(members))
    for g, special in ((4, (0, 1, r - 1)), (5, (r - 1, 0, 1)), (7, (1, r - 1, 0))):     # in a canonical, a plain and a negated member
        lo = starts[g]
        members[lo + 1] &= SIGN - 1
        members[lo + 2] |= SIGN
        for k, v in enumerate(special):
            scalars[members[lo + k] & (SIGN - 1)] = v
        scalars[members[lo + 3] & (SIGN - 1)] = special[2]
        members[lo + 3] |= SIGN
    lo = starts[len(sizes) - 1]                                                          # s - s
    members[lo + 1] |= SIGN
    scalars[members[lo + 1] & (SIGN - 1)] = scalars[members[lo]]
    return scalars, starts, members


# ------------------------------------------------------------------ the shim
def build_shim():
    """build/libmsm_stages.so from the shipped headers with the product's compiler flags; rebuilt when a source is newer.
    -> seconds spent compiling (0.0: up to date)"""
    return shim_build.device_shim("msm_stages.hip", SO)


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

    def filled(self, n, guard=1, value=FILL, dtype=np.uint32):
        """n live elements of `value` and `guard` elements of 0xFF.. behind them"""
        arr = np.full(n + guard, np.iinfo(dtype).max, dtype=dtype)
        if value != FILL:
            arr[:n] = value
        return self.put(arr)

    def get(self, addr, n, dtype=np.uint32):
        out = np.empty(n, dtype=dtype)
        self.card.download(addr, out)
        return out


class Stages:
    def __init__(self):
        self.build_seconds = build_shim()
        self.lib = ctypes.CDLL(SO)
        for name, args in LAUNCHERS.items():
            getattr(self.lib, name).argtypes = args
        self.lib.st_sizeof.argtypes = [cint, cint]
        self.lib.st_sizeof.restype = u32
        self.card = asm_card.Card()
        self.failed = None

    def run(self, name, *args):
        """one launcher; after a launch that did not come back clean nothing more is started on the card"""
        if self.failed:
            raise RuntimeError("not launched: %s failed earlier" % self.failed)
        e = getattr(self.lib, name)(*args)
        if e != 0:
            self.failed = "%s (hip error %d)" % (name, e)
            raise RuntimeError(self.failed)

    def bufs(self):
        return Bufs(self.card)

    def close(self):
        self.card.close()
        assert self.card.allocs == []

    # ---- the chains of msm_impl.h, on buffers of one Bufs
    def scan(self, B, a_in, a_out, n):
        a_sums = B.filled((n + 2047) // 2048 + 1)
        self.run("st_scan", a_in, a_out, n, a_sums)

    def digits(self, B, words, inf, lay, r, agg, with_counts):
        """-> (a_digits, a_counts): W n digits + guard, total counters (zeroed, as launch_sort does) + guard"""
        n = len(words)
        a_s = B.put(words)
        a_inf = B.put(np.asarray(inf, dtype=np.uint8)) if inf is not None else None
        a_d = B.filled(lay.W * n)
        a_c = B.filled(lay.total, value=0) if with_counts else None
        r24 = scalar_words([r])
        self.run("st_digits", a_s, a_inf, n, lay.c, lay.W, lay.win_stride, lay.top_unsigned, r24.ctypes.data_as(vp), a_d, a_c, agg,
                 lay.slot_shift, lay.sets)
        return a_d, a_c

    def atomic_path(self, B, words, inf, lay, r, agg, D):
        """launch_sort's small-input branch: digits with histogram, scan, cursor = starts, scatter -> digits, counts, starts, sorted
        (each with its guard word; sorted has W n words, of which the first `entries` are live).  D: the model's digits; the
        scatter is launched only over digits, counts and starts that agree with them, so every cursor it uses is in bounds."""
        n = len(words)
        a_d, a_c = self.digits(B, words, inf, lay, r, agg, True)
        a_st = B.filled(lay.total)
        self.scan(B, a_c, a_st, lay.total)
        digits, counts, starts = B.get(a_d, lay.W * n + 1).view(np.int32), B.get(a_c, lay.total + 1), B.get(a_st, lay.total + 1)
        want_counts = histogram(D, lay)
        gate = [first_diff("digits", digits, with_guard(D.T, np.int32)), first_diff("counts", counts, with_guard(want_counts)),
                first_diff("starts", starts, with_guard((np.cumsum(want_counts.astype(np.uint64)) - want_counts).astype(np.uint32)))]
        assert not any(gate), ["not scattered"] + [g for g in gate if g]
        a_cur = B.put(starts[:lay.total])
        a_so = B.filled(lay.W * n)
        self.run("st_scatter", a_d, n, lay.W, lay.win_stride, lay.row_stride, a_cur, a_so, agg, lay.slot_shift, lay.sets)
        return digits, counts, starts, B.get(a_so, lay.W * n + 1)

    def partitioned_path(self, B, words, inf, lay, r, tile, bin_shift, D):
        """sort_partitioned: digits without histogram, tile histogram, scan, tile scatter, one block per bin
        -> (counts, starts, sorted), [] or None, the failures that stopped the chain.
        D: the model's digits.  Each kernel that takes offsets from the card is launched only after the host has validated them:
        the tile scatter over offsets that are the scan of the tile histogram and end at the number of entries, the bin sort
        over pairs that are the model's, bin after bin (anything else is returned as a failure and the chain stops)."""
        n = len(words)
        ent = lay.W * n
        n_bins = (lay.total + (1 << bin_shift) - 1) >> bin_shift
        n_blocks = (ent + tile - 1) // tile
        cells = n_bins * n_blocks + 1
        assert tile <= n and n_bins <= PART_MAX_BINS and bin_shift <= 13        # what plan_sort guarantees the kernels
        a_d, _ = self.digits(B, words, inf, lay, r, 12, False)
        digits = B.get(a_d, ent + 1).view(np.int32)
        eb, ev = entries(D, lay)
        E = eb.size
        fails = [first_diff("digits", digits, with_guard(D.T, np.int32))]
        if fails[0]:
            return None, fails
        geo = (n, lay.W, lay.win_stride, lay.row_stride, lay.slot_shift, lay.sets, bin_shift, n_bins, tile)
        hist0 = np.full(cells + 1, FILL, dtype=np.uint32)
        hist0[cells - 1] = 0                                                     # the one cell the product clears: the total's
        a_h = B.put(hist0)
        self.run("st_part_hist", a_d, *geo, a_h)
        a_off = B.filled(cells)
        self.scan(B, a_h, a_off, cells)
        hist, off = B.get(a_h, cells + 1), B.get(a_off, cells + 1)
        # cell (bin, block): the entries of the block's tile that fall into the bin
        e_no = np.nonzero(D.T.reshape(-1))[0]                                    # entry numbers w n + i, in the order of entries()
        want_hist = np.bincount((eb >> bin_shift) * n_blocks + e_no // tile, minlength=cells).astype(np.uint32)
        fails = [first_diff("tile histogram", hist, with_guard(want_hist)),
                 first_diff("block offsets", off, with_guard((np.cumsum(want_hist.astype(np.uint64)) - want_hist).astype(np.uint32)))]
        if int(off[cells - 1]) != E:
            fails.append("the offsets end at %d, entries %d" % (int(off[cells - 1]), E))
        if any(fails):
            return None, [f for f in fails if f]
        a_part = B.filled(2 * ent, guard=2)
        self.run("st_part_scatter", a_d, *geo, a_off, a_part)
        part = B.get(a_part, 2 * ent + 2)
        pairs = part[:2 * E].reshape(E, 2)
        fails = [first_diff("pairs", pair_keys(pairs[:, 0], pairs[:, 1]), pair_keys(eb, ev)),
                 first_diff("pairs beyond the entries", part[2 * E:], np.full(2 * (ent - E) + 2, FILL, dtype=np.uint32))]
        if not np.array_equal(np.sort(pairs[:, 0] >> bin_shift, kind="stable"), pairs[:, 0] >> bin_shift):
            fails.append("the pairs are not grouped by bin")
        if any(fails):
            return None, [f for f in fails if f]
        a_c, a_st, a_so = B.filled(lay.total), B.filled(lay.total), B.filled(ent)
        self.run("st_bin_sort", a_part, a_off, n_blocks, bin_shift, n_bins, lay.total, a_c, a_st, a_so)
        return (B.get(a_c, lay.total + 1), B.get(a_st, lay.total + 1), B.get(a_so, ent + 1)), []

    def size_order(self, B, counts, starts, thr, want_hist):
        """launch_sort's middle: size histogram (+ plan[4]), scan, size scatter, heavy plan
        -> size_hist, size_cursor, order, chunk_start, plan and the device addresses of counts / starts / order / chunk_start.
        The scatter and the heavy plan take offsets from the card: they run only once the histogram and its scan are the model's."""
        total = len(counts)
        a_c, a_st = B.put(np.asarray(counts, dtype=np.uint32)), B.put(np.asarray(starts, dtype=np.uint32))
        a_hist = B.filled(SIZE_BINS, value=0)
        plan0 = np.full(17, FILL, dtype=np.uint32)
        plan0[4] = 0
        a_plan = B.put(plan0)
        self.run("st_size_hist", a_c, total, thr, a_hist, a_plan + 16)
        hist = B.get(a_hist, SIZE_BINS + 1)
        a_cur = B.filled(SIZE_BINS)
        self.scan(B, a_hist, a_cur, SIZE_BINS)
        cursor0 = B.get(a_cur, SIZE_BINS + 1)
        start_of_bin = (np.cumsum(want_hist.astype(np.uint64)) - want_hist).astype(np.uint32)
        gate = [first_diff("size_hist", hist, with_guard(want_hist)), first_diff("size_cursor after the scan", cursor0, with_guard(start_of_bin))]
        assert not any(gate), ["no order made"] + [g for g in gate if g]
        a_order = B.filled(total)
        self.run("st_size_scatter", a_c, total, thr, a_cur, a_order)
        n_heavy = int(hist[0])
        order = B.get(a_order, total)
        assert int(order.max()) < total, "no heavy plan made: order names bucket %d of %d" % (int(order.max()), total)
        a_cs = B.filled(n_heavy + 1)
        self.run("st_heavy_plan", a_hist, a_c, a_order, a_st, total, thr, a_cs, a_plan)
        got = dict(hist=hist, cursor0=cursor0, cursor=B.get(a_cur, SIZE_BINS + 1), order=B.get(a_order, total + 1),
                   chunk_start=B.get(a_cs, n_heavy + 2), plan=B.get(a_plan, 17))
        return got, (a_st, a_c, a_order, a_cs)


@pytest.fixture(scope="module")
def dev(gpu):
    d = Stages()
    print("\nlibmsm_stages.so: %s" % ("up to date" if d.build_seconds == 0.0 else "built in %.1f s" % d.build_seconds))
    yield d
    d.close()


def first_diff(what, got, want):
    """None, or a message naming the first differing element"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        return "%s: %d elements against %d" % (what, got.size, want.size)
    d = np.nonzero(got != want)[0]
    if d.size == 0:
        return None
    k = int(d[0])
    return "%s: %d elements differ; first at %d: %x against %x" % (what, d.size, k, int(got[k]) & M(got), int(want[k]) & M(got))


def M(arr):
    return (1 << (8 * arr.dtype.itemsize)) - 1


def with_guard(live, dtype=np.uint32):
    return np.concatenate([np.asarray(live).astype(dtype).reshape(-1), np.full(1, FILL, dtype=np.uint32).astype(dtype)])


def check_lists(what, D, lay, n, counts, starts, sorted_):
    """counts / starts / sorted as read back (with their guard words) against the model's digits D: the histogram, the starts
    tiling [0, entries), every list value a valid row index, per bucket the same multiset of list values.  -> failures"""
    fails = []
    eb, ev = entries(D, lay)
    E = eb.size
    want_counts = np.bincount(eb, minlength=lay.total).astype(np.uint32)
    fails.append(first_diff(what + " counts", counts, with_guard(want_counts)))
    want_starts = (np.cumsum(want_counts.astype(np.uint64)) - want_counts).astype(np.uint32)
    fails.append(first_diff(what + " starts", starts, with_guard(want_starts)))
    c64, s64 = counts[:-1].astype(np.int64), starts[:-1].astype(np.int64)
    if not (s64[0] == 0 and np.array_equal(s64[1:], s64[:-1] + c64[:-1]) and s64[-1] + c64[-1] == E):
        fails.append(what + ": the starts do not tile [0, %d)" % E)
    fails.append(first_diff(what + " sorted beyond the entries", sorted_[E:], np.full(sorted_.size - E, FILL, dtype=np.uint32)))
    live = sorted_[:E]
    limit = lay.rows() * lay.row_stride if lay.merged else n
    if E and int((live & (SIGN - 1)).max()) >= limit:
        fails.append(what + ": a list value names row %d of %d" % (int((live & (SIGN - 1)).max()), limit))
    if int(c64.sum()) == E:
        fails.append(first_diff(what + " (bucket, value) multiset", pair_keys(np.repeat(np.arange(lay.total), c64), live), pair_keys(eb, ev)))
    return [f for f in fails if f]


def lists_of(counts, starts, sorted_):
    """the card's arrays -> {bucket: list values}"""
    return {int(b): [int(v) for v in sorted_[int(starts[b]):int(starts[b]) + int(counts[b])]] for b in np.nonzero(counts[:-1])[0]}


def group_bases(r, n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(r) for _ in range(n)]


# ------------------------------------------------------------------ CPU: the shim, the model, the operand sets
def test_shim_cross_compiles_for_gfx950():
    build_shim()
    blob = open(SO, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS + tuple(LAUNCHERS) + ("st_sizeof", "Mnt4G1", "Mnt4G2"):
        assert k.encode() in blob, k


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_model_is_an_msm_over_the_integers_mod_r(field, c):
    """base i = a random integer b_i mod r: for every layout the weighted bucket sums give sum s_i b_i mod r -- weight slot
    (per window), slot + 2^(c-1) (region b), slot + 1 (merged; list values name rows of the shift table)"""
    r = FIELDS[field]
    S = scalar_set(field, c)
    S = S[:len(S) - 2000] + S[-150:]                                             # every edge scalar, 150 of the random ones
    n = len(S)
    b = group_bases(r, n, 1000 + c)
    want = sum(s * x for s, x in zip(S, b)) % r
    for sets in (0, 1, 2, 3):
        lay = layout(c, sets, n + 5)
        dig = [R.digits(s, c, lay.W, lay.top_unsigned, r) for s in S]
        assert all(d == [0] * lay.W for d in (dig[0], dig[S.index(r)]))          # s = r folds to 0
        lists = R.bucket_lists(dig, lay)
        assert all(0 <= k < lay.total for k in lists)
        assert R.msm_from_lists(lists, lay, b, r) == want, (field, c, sets)
        if not lay.merged and lay.top_unsigned:                                  # region b is in use, window W-2 stays unsigned
            assert any(k // lay.nb == lay.W - 1 for k in lists) and all(d[lay.W - 2] * d[lay.W - 1] == 0 for d in dig)


@pytest.mark.parametrize("sets", (0, 1, 3))
def test_array_form_against_the_model(sets):
    """entries() (numpy) and Layout.bucket / Layout.value (the model) name the same (bucket, value) pairs"""
    c, field = 8, "mnt4"
    D = digit_table(field, c, layout(c, sets).top_unsigned)[:300]
    lay = layout(c, sets, 307)
    lists = R.bucket_lists([[int(d) for d in row] for row in D], lay)
    want = pair_keys([k for k, v in lists.items() for _ in v], [x for v in lists.values() for x in v])
    assert np.array_equal(pair_keys(*entries(D, lay)), want)
    assert histogram(D, lay).sum() == want.size


def test_operand_sets_hold_the_rows_they_exist_for():
    for field, r in FIELDS.items():
        assert r.bit_length() == 753 and r % 2 == 1
        for c in CS:
            p = plan(1000, c)
            W, top = p["W"], p["top_unsigned"]
            assert top == int(752 % c == 0)
            S = scalar_set(field, c)
            dg = lambda s: R.digits(s, c, W, top, r)
            # each side of the sign fold: (r - 1) / 2 stays, (r + 1) / 2 = r - (r - 1) / 2 is its negative
            lo, hi = (r - 1) // 2, (r + 1) // 2
            assert lo in S and hi in S and dg(hi) == [-d for d in dg(lo)] and max(dg(lo)) > 0 and min(dg(1)) == 0
            assert dg(r - 1) == [-d for d in dg(1)] and dg(r) == [0] * W
            # no carry anywhere / a carry out of every signed window below the top
            half = 1 << (c - 1)
            nc, ac = no_carry_scalar(c), all_carry_scalar(c)
            assert nc in S and ac in S and ac < r - ac
            assert dg(nc)[:W - 1] == [half] * (W - 1) and dg(nc)[W - 1] == 0
            signed = W - 1 - top                                                 # windows recoded with a carry out
            assert dg(ac)[:signed] == [1 - half] + [2 - half] * (signed - 1)
            assert dg(ac)[signed:] == ([0, 2] if top else [1])                   # the carry arrives at the top (unsigned: region b)
    # the two heavy thresholds the size order is run at are the plan's bounds
    assert plan(1000, 13)["heavy_thr"] == 128 and plan(1 << 24, 19)["heavy_thr"] == 1024
    wave = thirteen_key_wave()
    assert len(wave) == 64 and len(set(R.digits(s, 13, 58, 0, FIELDS["mnt4"])[0] for s in wave)) == 13 > 12
    assert all(set(R.digits(s, 13, 58, 0, FIELDS["mnt4"])[1:]) == {0} for s in wave)
    scalars, starts, members = merge_case(FIELDS["mnt4"])
    sizes = [starts[g + 1] - starts[g] for g in range(len(starts) - 1)]
    assert sizes[:-1] == list(MERGE_GROUPS) and 4097 in sizes and R.DUP_CHUNK == 4096
    chunks, first = R.dup_chunks(starts)
    assert [first[g + 1] - first[g] for g in range(len(sizes))] == [1, 1, 1, 1, 1, 1, 2, 3, 1]
    idx = [m & (SIGN - 1) for m in members]
    assert len(set(idx)) == len(idx) and all(idx[starts[g]:starts[g + 1]] == sorted(idx[starts[g]:starts[g + 1]]) for g in range(len(sizes)))
    assert any(m & SIGN for m in members) and not any(members[s] & SIGN for s in starts[:-1])
    r = FIELDS["mnt4"]
    assert {0, 1, r - 1} <= {scalars[i] for i in idx}
    merged = R.merge_scalars(scalars, len(scalars), starts, members, r)
    assert merged[idx[starts[-2]]] == 0 and scalars[idx[starts[-2]]] != 0        # the pair that cancels


# ------------------------------------------------------------------ GPU: digits and histogram
@pytest.mark.gpu
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_digits_and_histogram(dev, field, c):
    """the whole scalar set on every layout; the per-window layout also at every n x agg_iters on the prefixes (the edge scalars
    come first), with infinity flags, and without a histogram (the partitioned path's call).  Histogram where sets * nb <= 2^24."""
    r, S = FIELDS[field], scalar_set(field, c)
    N = len(S)
    words = scalar_words(S)
    fails = []

    def one(lay, n, agg, inf, with_counts, what):
        D = digit_table(field, c, lay.top_unsigned)[:n]
        if inf is not None:
            D = np.where(np.asarray(inf, dtype=bool)[:, None], 0, D)
        with dev.bufs() as B:
            a_d, a_c = dev.digits(B, words[:n], inf, lay, r, agg, with_counts)
            fails.append(first_diff("%s digits" % what, B.get(a_d, lay.W * n + 1).view(np.int32), with_guard(D.T, np.int32)))
            if with_counts:
                fails.append(first_diff("%s counts" % what, B.get(a_c, lay.total + 1), with_guard(histogram(D, lay))))

    for sets in (0, 1, 2, 3):
        lay = layout(c, sets, N + 3)
        hist = lay.total <= 1 << 24
        one(lay, N, 12, None, hist, "%s c %d sets %d n %d" % (field, c, sets, N))
        if sets == 0:
            for n in NS:
                for agg in AGG:
                    one(lay, n, agg, None, hist, "%s c %d n %d agg %d" % (field, c, n, agg))
            inf = [1 if i % 3 == 0 or i in (63, 64, 999) else 0 for i in range(1000)]
            one(lay, 1000, 12, inf, hist, "%s c %d infinity flags" % (field, c))
            one(lay, 257, 12, [0] * 257, hist, "%s c %d no flag set" % (field, c))
            if hist:
                one(lay, 1000, 12, inf, False, "%s c %d counts = nullptr" % (field, c))
    fails = [f for f in fails if f]
    assert not fails, fails[:8]


WAVE_CASES = {
    "all_equal": lambda r: [0x123456789ABCDEF0123456789ABCDEF % r] * 257,
    "zero_one": lambda r: [(i * i + i // 7) & 1 for i in range(1000)],
    "one_key_per_wave": lambda r: [1] * 64 + [2] * 64 + [r - 1] * 64 + [0] * 64 + [1] * 5,
    "thirteen_keys": lambda r: thirteen_key_wave() + [1 + i % 14 for i in range(64)] + [1 + i % 12 for i in range(64)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("agg", AGG)
@pytest.mark.parametrize("case", sorted(WAVE_CASES))
def test_wave_aggregation_in_histogram_and_scatter(dev, case, agg):
    """wave_agg_inc where it can go wrong: all 64 lanes on one key, more distinct keys in a wave than agg_iters (13 with
    agg_iters = 12), agg_iters = 0 -- through the histogram (the sum per key) and the scatter (a distinct position per lane)"""
    r = FIELDS["mnt4"]
    S = WAVE_CASES[case](r)
    n = len(S)
    fails = []
    for c, sets in ((13, 0), (13, 1), (16, 0)):
        lay = layout(c, sets, n + 2)
        D = np.array([R.digits(s, c, lay.W, lay.top_unsigned, r) for s in S], dtype=np.int32)
        with dev.bufs() as B:
            digits, counts, starts, sorted_ = dev.atomic_path(B, scalar_words(S), None, lay, r, agg, D)
        fails += check_lists("%s c %d sets %d agg %d" % (case, c, sets, agg), D, lay, n, counts, starts, sorted_)
    fails = [f for f in fails if f]
    assert not fails, fails[:8]


# ------------------------------------------------------------------ GPU: scan
SCAN_NS = (1, 2047, 2048, 2049, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, 2048 * 1025 + 5)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_NS)
def test_exclusive_scan(dev, n):
    """ones, seeded values below 2^11, and a total of 2^32 - 1; n = 2048 * 1025 + 5 has 1026 block sums: a second trip of
    scan_block_sums_kernel's loop"""
    rng = np.random.default_rng(n)
    big = np.zeros(n, dtype=np.uint32)
    big[rng.integers(0, n, size=min(n, 64))] = 1 << 20
    big[n - 1] = 0
    big[0] += np.uint32(FILL - int(big.astype(np.uint64).sum()))                 # the total: 2^32 - 1, nothing wraps
    inputs = {"ones": np.ones(n, dtype=np.uint32), "below 2^11": rng.integers(0, 1 << 11, size=n, dtype=np.uint32), "total 2^32 - 1": big}
    assert int(big.astype(np.uint64).sum()) == FILL and (SCAN_NS[-1] + 2047) // 2048 == 1026
    fails = []
    for name, v in inputs.items():
        want = (np.cumsum(v.astype(np.uint64)) - v).astype(np.uint32)
        assert name != "ones" or np.array_equal(want, np.arange(n, dtype=np.uint32))
        with dev.bufs() as B:
            a_in, a_out = B.put(v), B.filled(n)
            dev.scan(B, a_in, a_out, n)
            fails.append(first_diff("scan %s n %d" % (name, n), B.get(a_out, n + 1), with_guard(want)))
            fails.append(first_diff("scan %s n %d: the input" % (name, n), B.get(a_in, n), v))
    fails = [f for f in fails if f]
    assert not fails, fails


# ------------------------------------------------------------------ GPU: lists
def list_operands(field, c, n):
    """n scalars drawn (with repetition) from the scalar set, whose digits the model has -> (words, rows of the digit table)"""
    N = len(scalar_set(field, c))
    idx = (np.arange(n, dtype=np.int64) * 7919 + 13) % N
    return scalar_words(scalar_set(field, c))[idx], idx


def identity_on_card_arrays(what, field, S, lay, counts, starts, sorted_):
    r = FIELDS[field]
    b = group_bases(r, len(S), 77)
    want = sum(s * x for s, x in zip(S, b)) % r
    got = R.msm_from_lists(lists_of(counts, starts, sorted_), lay, b, r)
    return None if got == want else "%s: the card's lists sum to %x, the MSM is %x" % (what, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("agg", (0, 12))
@pytest.mark.parametrize("sets", (0, 1, 2, 3))
def test_lists_on_the_atomic_path(dev, sets, agg):
    """digits with histogram, scan, cursor = starts, scatter, as launch_sort chains them; infinity flags on some rows"""
    field, c, n = "mnt6", 13, 1000
    r = FIELDS[field]
    lay = layout(c, sets, n + 9)
    words, idx = list_operands(field, c, n)
    inf = np.array([1 if i % 11 == 5 else 0 for i in range(n)], dtype=np.uint8)
    D = np.where(inf.astype(bool)[:, None], 0, digit_table(field, c, lay.top_unsigned)[idx])
    with dev.bufs() as B:
        digits, counts, starts, sorted_ = dev.atomic_path(B, words, inf, lay, r, agg, D)
    what = "atomic sets %d agg %d" % (sets, agg)
    fails = check_lists(what, D, lay, n, counts, starts, sorted_)
    assert not fails, fails
    S = [0 if inf[i] else scalar_set(field, c)[int(k)] for i, k in enumerate(idx)]
    assert identity_on_card_arrays(what, field, S, lay, counts, starts, sorted_) is None


def both_paths(dev, field, c, sets, n, tile, bin_shifts, identity):
    r = FIELDS[field]
    lay = layout(c, sets, n + 9)
    words, idx = list_operands(field, c, n)
    D = digit_table(field, c, lay.top_unsigned)[idx]
    fails = []
    with dev.bufs() as B:
        _, a_counts, a_starts, a_sorted = dev.atomic_path(B, words, None, lay, r, 12, D)
    fails += check_lists("atomic n %d" % n, D, lay, n, a_counts, a_starts, a_sorted)
    for bin_shift in bin_shifts:
        what = "partitioned c %d sets %d n %d tile %d bin_shift %d" % (c, sets, n, tile, bin_shift)
        with dev.bufs() as B:
            got, stopped = dev.partitioned_path(B, words, None, lay, r, tile, bin_shift, D)
        if got is None:
            fails += ["%s: %s" % (what, f) for f in stopped]
            continue
        counts, starts, sorted_ = got
        fails += check_lists(what, D, lay, n, counts, starts, sorted_)
        fails.append(first_diff(what + ": counts against the atomic path", counts, a_counts))
        fails.append(first_diff(what + ": starts against the atomic path", starts, a_starts))
        if identity:
            S = [scalar_set(field, c)[int(k)] for k in idx]
            fails.append(identity_on_card_arrays(what, field, S, lay, counts, starts, sorted_))
    return [f for f in fails if f]


@pytest.mark.gpu
@pytest.mark.parametrize("sets", (0, 2, 3))
@pytest.mark.parametrize("n", (256, 257, 767))
def test_lists_on_both_paths_small_tile(dev, n, sets):
    """tile = 256 at n = tile, tile + 1, 3 tile - 1; bin_shift 8 and 13.  Per window at c = 13: 58 x 4097 buckets, no multiple
    of either bin size.  Identical counts and starts on both paths, the model's multiset per bucket, and the MSM identity on
    the card's lists."""
    assert layout(13, 0).total % 256 != 0 and layout(13, 0).total % 8192 != 0
    fails = both_paths(dev, "mnt4", 13, sets, n, 256, (8, 13), True)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("n", (16384, 16385, 3 * 16384 - 1))
def test_lists_on_both_paths_shipped_tile(dev, n):
    """the shipped tile of 16384 entries at n = tile, tile + 1, 3 tile - 1; bin_shift 8 (929 bins) and 13 (30 bins)"""
    fails = both_paths(dev, "mnt4", 13, 0, n, 16384, (8, 13), False)
    assert not fails, fails


@pytest.mark.gpu
def test_lists_at_the_shipped_shape(dev):
    """n = 16384, c = 16 (top_unsigned) with the tile and the bins plan_sort chooses"""
    n, c = 16384, 16
    lay = layout(c, 0, n=n)
    out = (u32 * 5)()
    host_shim().t_plan_sort(lay.W * n, n, lay.total, out)
    tile, bin_shift, n_bins = int(out[0]), int(out[1]), int(out[2])
    assert lay.top_unsigned == 1 and tile == 16384 and n_bins << bin_shift >= lay.total and lay.total % (1 << bin_shift) != 0
    fails = both_paths(dev, "mnt6", c, 0, n, tile, (bin_shift,), False)
    assert not fails, fails


# ------------------------------------------------------------------ GPU: size order, heavy plan, task table
def synthetic_counts(total, thr, heavy, seed):
    sizes = [0, 1, thr - 1, thr, thr + 1, 5 * thr + 3] if heavy else [0, 1, thr - 1, thr]
    rng = np.random.default_rng(seed)
    counts = rng.choice(np.array(sizes, dtype=np.uint32), size=total)
    if total >= len(sizes):
        counts[rng.permutation(total)[:len(sizes)]] = sizes                     # each size at least once
    return counts


SIZE_CASES = [(thr, total, True) for thr in (128, 1024) for total in (1, 255, 256, 257, 100000)] + [(128, 257, False), (1024, 1, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("thr,total,heavy", SIZE_CASES)
def test_size_order_heavy_plan_and_task_table(dev, thr, total, heavy):
    """counts of 0, 1, thr - 1, thr, thr + 1 and 5 thr + 3 (one case without a heavy bucket; total = 1 is one heavy bucket or
    one empty one): size_hist and plan[0..4] exact, order a permutation by size bin with the heavy buckets first, the chunks
    against the card's own order, then the task table of both point types against the enumeration"""
    counts = synthetic_counts(total, thr, heavy, 1000 * thr + total)
    if total == 1:
        counts[0] = 5 * thr + 3 if heavy else 0
    starts = (np.cumsum(counts.astype(np.uint64)) - counts).astype(np.uint32)
    assert int(counts.astype(np.uint64).sum()) < 1 << 32
    bins = np.array([R.size_bin(int(x), thr) for x in counts])
    want_hist = np.bincount(bins, minlength=SIZE_BINS).astype(np.uint32)
    n_heavy = int((counts > thr).sum())
    assert n_heavy == int(want_hist[0]) and (n_heavy > 0) == (heavy and (total > 1 or counts[0] > thr))
    tables = {}
    with dev.bufs() as B:
        got, (a_st, a_c, a_order, a_cs) = dev.size_order(B, counts, starts, thr, want_hist)     # size_hist and its scan: checked in there
        order = got["order"][:total]
        start_of_bin = (np.cumsum(want_hist.astype(np.uint64)) - want_hist).astype(np.uint32)
        fails = [first_diff("size_cursor after the scatter", got["cursor"], with_guard(start_of_bin + want_hist))]
        assert got["order"][total] == FILL and np.array_equal(np.sort(order), np.arange(total)), "order is no permutation"
        assert np.array_equal(bins[order], np.sort(bins)), "order is not sorted by size bin"
        assert np.all(counts[order[:n_heavy]] > thr) and np.all(counts[order[n_heavy:]] <= thr)
        want_cs = R.heavy_chunks([int(x) for x in counts], [int(g) for g in order], n_heavy, thr)
        fails.append(first_diff("chunk_start", got["chunk_start"], with_guard(want_cs)))
        n_chunks = want_cs[-1]
        want_plan = np.full(17, FILL, dtype=np.uint32)
        want_plan[:5] = [n_heavy, n_chunks, int(counts.astype(np.uint64).sum()), 0, int(counts.max())]
        fails.append(first_diff("plan", got["plan"], want_plan))
        fails = [f for f in fails if f]
        assert not fails, fails
        # the task table, from the card's own arrays
        n_tasks = n_chunks + total - n_heavy
        for curve, deg in ((0, 1), (1, 2)):
            a_out = B.filled(4 * n_tasks, guard=4)
            a_tile = B.put(np.array([0xDEADBEEF, FILL], dtype=np.uint32))
            buckets, partials = 0x7E0000000000 + 8 * curve, 0x7F0000001000
            dev.run("st_acc_tasks", curve, a_st, a_c, a_order, total, buckets, a_cs, n_heavy, n_chunks, thr, partials, a_out, a_tile)
            tables[curve] = (B.get(a_out, 4 * n_tasks + 4), B.get(a_tile, 2), buckets, partials, 3 * deg * 26 * 4)
            assert dev.lib.st_sizeof(curve, 1) == 3 * deg * 26 * 4 and dev.lib.st_sizeof(curve, 2) == 16
    model = R.tasks([int(x) for x in starts], [int(x) for x in counts], [int(g) for g in order], n_heavy, thr)
    assert len(model) == n_tasks
    spans = np.array(sorted((beg, cnt) for beg, cnt, _, _ in model if cnt), dtype=np.int64).reshape(-1, 2)
    assert spans.size == 0 or (spans[0, 0] == 0 and np.array_equal(spans[1:, 0], spans[:-1].sum(axis=1))
                               and spans[-1].sum() == int(counts.astype(np.uint64).sum())), "the model's tasks: every list entry once"
    for curve, (out, tile, buckets, partials, size) in tables.items():
        want = np.full(4 * n_tasks + 4, FILL, dtype=np.uint32)
        rec = want[:4 * n_tasks].reshape(n_tasks, 4)
        dst = np.array([(partials if is_chunk else buckets) + size * k for _, _, is_chunk, k in model], dtype=np.uint64)
        rec[:, 0] = [m[0] for m in model]
        rec[:, 1] = [m[1] for m in model]
        rec[:, 2] = (dst & np.uint64(FILL)).astype(np.uint32)
        rec[:, 3] = (dst >> np.uint64(32)).astype(np.uint32)
        assert first_diff("task table, curve %d" % curve, out, want) is None
        assert [int(x) for x in tile] == [0, FILL], "tile_counter"


# ------------------------------------------------------------------ GPU: equal bases
def random_points(n, deg, seed):
    """n rows of Aff words: x then y, deg x 26 words each (any words: these kernels hash and compare, they do no arithmetic)"""
    return np.random.default_rng(seed).integers(0, 1 << 29, size=(n, 2 * deg * 26), dtype=np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("curve,deg", [(0, 1), (1, 2)])
def test_base_hash(dev, curve, deg):
    nx = 26 * deg
    fails = []
    for n in (1, 255, 256, 257):
        pts = random_points(n, deg, 500 + n + deg)
        pts[n // 2, :nx] = 0                                                     # an all-zero abscissa is a base like any other
        for inf in (None, np.array([1 if i % 5 == 1 else 0 for i in range(n)], dtype=np.uint8)):
            want = np.full(2 * n + 1, (1 << 64) - 1, dtype=np.uint64)
            for i in range(n):
                h1, h2 = (0, 0) if inf is not None and inf[i] else R.base_hash([int(x) for x in pts[i, :nx]])
                want[2 * i], want[2 * i + 1] = h1, h2
            with dev.bufs() as B:
                assert dev.lib.st_sizeof(curve, 0) == pts.shape[1] * 4
                a_out = B.filled(2 * n, dtype=np.uint64)
                dev.run("st_base_hash", curve, B.put(pts), B.put(inf) if inf is not None else None, n, a_out)
                fails.append(first_diff("hash curve %d n %d" % (curve, n), B.get(a_out, 2 * n + 1, np.uint64), want))
    fails = [f for f in fails if f]
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("curve,deg", [(0, 1), (1, 2)])
def test_dup_verify(dev, curve, deg):
    """groups of 600, 2 and 257 members that are equal to the canonical base, opposite (same x, other y) or different in one
    word of x (every word position in turn): the different ones flagged with no sign, the opposite ones signed"""
    nx = 26 * deg
    sizes = (600, 2, 257)
    n_pts = sum(sizes) + 10
    pts = random_points(n_pts, deg, 900 + deg)
    perm = np.random.default_rng(5).permutation(n_pts)
    members, starts, want_m, want_f = [], [0], [], []
    at = 0
    for gsize in sizes:
        idx = sorted(int(x) for x in perm[at:at + gsize])
        at += gsize
        canon = idx[0]
        members.append(canon)
        want_m.append(canon)
        want_f.append(0xFF)                                                      # the canonical member: not written
        for k, m in enumerate(idx[1:]):
            kind = k % 4
            pts[m] = pts[canon]
            if kind == 1:                                                        # opposite: y differs, in one word only
                pts[m, nx + (k // 4) % nx] ^= 1
            elif kind >= 2:                                                      # another point: x differs in one word; y equal (2) or not (3)
                pts[m, (k // 4) % nx] ^= 1 << 28
                if kind == 3:
                    pts[m, nx + nx - 1] ^= 5
            members.append(m | (SIGN if k % 3 == 0 else 0))                      # whatever bit 31 held before is replaced
            want_m.append(m | (SIGN if kind == 1 else 0))
            want_f.append(1 if kind >= 2 else 0)
        starts.append(len(members))
    assert sizes[0] - 1 >= 4 * nx and sizes[0] - 1 > 2 * 256                     # every word position in each kind; three trips of a block's loop
    with dev.bufs() as B:
        a_m = B.put(np.array(members + [FILL], dtype=np.uint32))
        a_f = B.filled(len(members), dtype=np.uint8)
        dev.run("st_dup_verify", curve, B.put(pts), B.put(np.array(starts, dtype=np.uint32)), len(sizes), a_m, a_f)
        got_m, got_f = B.get(a_m, len(members) + 1), B.get(a_f, len(members) + 1, np.uint8)
    fails = [first_diff("members", got_m, with_guard(want_m)), first_diff("flags", got_f, with_guard(want_f, np.uint8))]
    fails = [f for f in fails if f]
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_merge_of_equal_bases(dev, field):
    """groups of 1 .. 8193 members in chunks of 4096 as the key builder cuts them, for a call with every scalar and for calls
    that use fewer scalars than the key has bases: the canonical member holds the signed sum mod r, the other members below n
    are zero, everything else keeps its value; the chunk sums are checked as well"""
    r = FIELDS[field]
    scalars, starts, members = merge_case(r)
    N = len(scalars)
    chunks, first = R.dup_chunks(starts)
    idx = [m & (SIGN - 1) for m in members]
    words = scalar_words(scalars)
    r24 = scalar_words([r])
    fails = []
    for n in (N, N // 2, idx[starts[7]] + 1, 1):
        want = R.merge_scalars(scalars, n, starts, members, r)
        assert want[n:] == scalars[n:] and (n < N // 2 or want != scalars)
        want_partial = [sum((-scalars[m & (SIGN - 1)] if m & SIGN else scalars[m & (SIGN - 1)])
                            for m in members[lo:hi] if m & (SIGN - 1) < n) % r for lo, hi, _ in chunks]
        with dev.bufs() as B:
            a_in = B.put(words)
            a_out = B.put(np.concatenate([words, np.full((1, 24), FILL, dtype=np.uint32)]))      # merge_equal_bases: out starts as a copy
            a_st, a_mem = B.put(np.array(starts, dtype=np.uint32)), B.put(np.array(members, dtype=np.uint32))
            a_ch = B.put(np.array([x for ck in chunks for x in ck] + first, dtype=np.uint32))    # the key's layout: triples, then offsets
            a_part = B.filled(24 * len(chunks), guard=24)
            dev.run("st_merge_scalars", a_in, a_out, n, a_st, a_mem, a_ch, len(chunks), a_part, r24.ctypes.data_as(vp))
            dev.run("st_merge_groups", a_out, n, a_st, a_mem, a_ch + 12 * len(chunks), len(starts) - 1, a_part, r24.ctypes.data_as(vp))
            out, partial = B.get(a_out, 24 * (N + 1)), B.get(a_part, 24 * len(chunks) + 24)
            fails.append(first_diff("n %d: the input" % n, B.get(a_in, 24 * N), words))
        guard_row = np.full(24, FILL, dtype=np.uint32)
        fails.append(first_diff("n %d: merged scalars (24 words each)" % n, out, np.concatenate([scalar_words(want).reshape(-1), guard_row])))
        fails.append(first_diff("n %d: chunk sums (24 words each)" % n, partial, np.concatenate([scalar_words(want_partial).reshape(-1), guard_row])))
    fails = [f for f in fails if f]
    assert not fails, fails
