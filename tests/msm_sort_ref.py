"""msm_sort_ref.py -- a Python-integer model of the MSM's sort stage, stage by stage, written from the comments of
ginger-lib_amd/csrc/msm_kernels.h and msm_plan.h (what each stage promises), not from the kernel bodies.  Not a test module:
tests/test_gpu_msm_stages.py compares the kernels with it and pins it to what an MSM means.

Scope of digits(): canonical scalars 0 <= s <= r.  s = r folds to 0.  Scalars above r are outside the model (and outside the
kernel's contract: "scalars: n x 24 words canonical").
"""
M64 = (1 << 64) - 1
SIGN = 1 << 31
DUP_CHUNK = 4096          # msm_plan.h MSM_DUP_CHUNK


# ------------------------------------------------------------------ digits
def digits(s, c, W, top_unsigned, r, inf=False):
    """the W signed digits of scalar s (window w weighs 2^(c w)); 0 = no contribution.
    (a) sign fold: r - s replaces s, with every digit negated, if r - s < s -- the magnitude is then below 2^752.
    (b) signed recoding: v = bits(s, c w, c) + carry; v > 2^(c-1) gives d = v - 2^c and a carry into the next window.
    (c) the last window holds the leftover bits plus the carry and never carries out.  With top_unsigned (c divides 752) window
        W-2 is taken unsigned instead: v <= 2^(c-1) is its digit; a larger v is filed as v - 2^(c-1) under window W-1, which is
        region b of window W-2 (same window weight, slot offset 2^(c-1)), and window W-2's own digit is 0."""
    assert 0 <= s <= r and W == 752 // c + 1
    if inf:
        return [0] * W
    neg = r - s < s
    if neg:
        s = r - s
    assert s < 1 << 752
    half, out, carry, region_b = 1 << (c - 1), [], 0, 0
    for w in range(W):
        v = ((s >> (c * w)) & ((1 << c) - 1)) + carry
        if top_unsigned and w == W - 2:
            d, region_b, carry = (0, v - half, 0) if v > half else (v, 0, 0)
        elif top_unsigned and w == W - 1:
            assert v == 0
            d = region_b
        elif v > half:
            d, carry = v - (1 << c), 1
        else:
            d, carry = v, 0
        out.append(-d if neg else d)
    assert carry == 0
    return out


# ------------------------------------------------------------------ slots, buckets, list values
class Layout:
    """where a digit goes.  Per window: every window its own bucket set, sets = W, nb = 2^(c-1) + 1 slots (slot 0 unused),
    slot = |d|.  Merged (a key with a shift table of `sets` bucket sets): window w files into set w % sets and reads table row
    w // sets, nb = 2^(c-1), slot = |d| - 1, row_stride = the key's length."""

    def __init__(self, c, W, top_unsigned, sets, nb, slot_shift, row_stride):
        self.c, self.W, self.top_unsigned, self.sets, self.nb = c, W, top_unsigned, sets, nb
        self.win_stride, self.slot_shift, self.row_stride = nb, slot_shift, row_stride
        self.total = sets * nb
        self.merged = slot_shift == 1

    @staticmethod
    def per_window(c, W, top_unsigned):
        return Layout(c, W, top_unsigned, W, (1 << (c - 1)) + 1, 0, 0)

    @staticmethod
    def merged_sets(c, W, sets, row_stride):
        return Layout(c, W, 0, sets, 1 << (c - 1), 1, row_stride)

    def bucket(self, w, d):
        assert d != 0 and 0 <= abs(d) - self.slot_shift < self.nb
        return (w % self.sets) * self.win_stride + abs(d) - self.slot_shift

    def value(self, w, i, d):
        return (i + (w // self.sets) * self.row_stride) | (SIGN if d < 0 else 0)

    def rows(self):
        return (self.W + self.sets - 1) // self.sets if self.merged else 1

    def weight(self, bucket):
        """the integer a bucket's sum is multiplied by in the MSM"""
        g, slot = divmod(bucket, self.win_stride)
        if self.merged:
            return (slot + 1) << (self.c * g)
        if self.top_unsigned and g == self.W - 1:                    # region b of window W-2
            return (slot + (1 << (self.c - 1))) << (self.c * (self.W - 2))
        return slot << (self.c * g)

    def base_of(self, value, b, r):
        """the group element a list value names, in the group of integers mod r with base i = b[i]: +-b[i], or row j of the
        shift table, 2^(c sets j) b[i]"""
        idx = value & (SIGN - 1)
        if self.merged:
            j, i = divmod(idx, self.row_stride)
            x = (b[i] << (self.c * self.sets * j)) % r
        else:
            x = b[idx]
        return -x if value & SIGN else x


def bucket_lists(dig, lay):
    """dig[i] = the digits of scalar i -> {bucket: sorted list values}"""
    lists = {}
    for i, row in enumerate(dig):
        for w, d in enumerate(row):
            if d:
                lists.setdefault(lay.bucket(w, d), []).append(lay.value(w, i, d))
    return {k: sorted(v) for k, v in lists.items()}


def msm_from_lists(lists, lay, b, r):
    """sum over buckets of weight(bucket) * (sum of the bucket's +-bases), mod r"""
    return sum(lay.weight(k) * sum(lay.base_of(v, b, r) for v in vals) for k, vals in lists.items()) % r


# ------------------------------------------------------------------ scan, size bins, heavy chunks, tasks
def exclusive_scan(v):
    out, run = [], 0
    for x in v:
        out.append(run & 0xFFFFFFFF)
        run += x
    return out


def size_bin(cnt, heavy_thr):
    """larger sizes first: the heavy buckets (cnt > heavy_thr) in bin 0, then the sizes heavy_thr .. 0"""
    return 0 if cnt > heavy_thr else heavy_thr + 1 - cnt


def heavy_chunks(counts, order, n_heavy, chunk):
    """chunk_start[0 .. n_heavy]: heavy bucket h owns ceil(counts / chunk) chunks"""
    out = [0]
    for h in range(n_heavy):
        out.append(out[-1] + (counts[order[h]] + chunk - 1) // chunk)
    return out


def tasks(starts, counts, order, n_heavy, chunk):
    """the accumulation's task list by enumeration: the chunks of the heavy buckets order[0 .. n_heavy) one after the other, then
    one task per remaining bucket in order.  -> [(beg, cnt, is_chunk, index)]: a chunk's sum goes to partials[task number], a
    bucket's to buckets[bucket]"""
    out = []
    for h in range(n_heavy):
        g = order[h]
        for b in range(0, counts[g], chunk):
            out.append((starts[g] + b, min(chunk, counts[g] - b), 1, len(out)))
    out += [(starts[g], counts[g], 0, g) for g in order[n_heavy:]]
    return out


# ------------------------------------------------------------------ equal bases
def base_hash(words):
    """128 bits over the 32-bit words of a base's abscissa, in 64-bit wrap-around arithmetic; never (0, 0), which stands for
    infinity"""
    h1, h2 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
    for x in words:
        h1 = ((h1 ^ x) * 0xFF51AFD7ED558CCD) & M64
        h1 ^= h1 >> 29
        h2 = ((h2 + x) * 0x94D049BB133111EB) & M64
        h2 = ((h2 << 27) | (h2 >> 37)) & M64
    if h1 == 0 and h2 == 0:
        h1 = 1
    return h1, h2


def dup_chunks(starts):
    """the groups cut into chunks of at most DUP_CHUNK members, as the key builder lays them out: (first, end, group) per chunk,
    and the first chunk of every group (one more entry: the number of chunks)"""
    chunks, first = [], []
    for g in range(len(starts) - 1):
        first.append(len(chunks))
        for lo in range(starts[g], starts[g + 1], DUP_CHUNK):
            chunks.append((lo, min(lo + DUP_CHUNK, starts[g + 1]), g))
    first.append(len(chunks))
    return chunks, first


def merge_scalars(scalars, n, starts, members, r):
    """the first n scalars with, per group, the canonical (first) member's scalar replaced by the signed sum of the group's
    scalars mod r and the other members' zeroed; members at or above n take no part and keep their value"""
    out = list(scalars)
    for g in range(len(starts) - 1):
        grp = members[starts[g]:starts[g + 1]]
        canon = grp[0] & (SIGN - 1)
        if canon >= n:
            continue
        acc = 0
        for e in grp:
            m = e & (SIGN - 1)
            if m < n:
                acc += -scalars[m] if e & SIGN else scalars[m]
                out[m] = 0
        out[canon] = acc % r
    return out
