"""msm_reduce_ref.py -- the referee of the MSM's bucket reduction (ginger-lib_amd/csrc/msm_reduce_kernels.h) and of
msm_heavy_combine_kernel, in Python integers.  Not a test module; tests/test_gpu_msm_reduce.py uses it.

Every item of a reduction is a known multiple m P of one base point P of the curve (m = 0: infinity), so the model lives in the
integers mod r, the group order.  What a program must deliver is written down BY DEFINITION, from the sums the kernels' header
promises, not by following the program:

  segment with items x_j, j = g + TPW i  (g < TPW the group, i < L the group's slot; x_j = 0 where item0 + j >= count)
    mode 0   out[gb 3 + 0] = runW = sum_j x_j     out[gb 3 + 1] = A = sum_g sum_i i x_(g,i)     out[gb 3 + 2] = Bv = sum_g g run_g
             so that sum_j j x_j = TPW A + Bv
    mode 1   out[gb 3] = sum_j x_j
    mode 2   (G1, TPW = 64) out[(blk 64 + l) 2 + 0] = run_l = sum_i x_(l,i),  out[(blk 64 + l) 2 + 1] = wacc_l = sum_i i x_(l,i)
    a segment with w count + item0 >= valid: proj_zero, limb for limb, in every row the mode writes
  item (w, k) of an input is base[(w count + k) stride + offset]                                                    (flat)
  heavy_combine: buckets[order[h]] = sum partials[chunk_start[h] .. chunk_start[h + 1]), every other bucket untouched

Separately, replay() runs the step schedule of msm_schedule.h (through the host shim: t_wave_step, t_wave_step_active) over the
same integers and records, step by step, which groups meet equal non-zero operands (the salt detour), which salt the detour
must take, and which groups meet an infinite operand.  It produces no expected value: it only proves that an operand set holds
the collision it is named for.

The internal form of a point (fp29.h, ec29.h): a coordinate is DEG coefficients c0, c1, .. of Fp; an Fp is the Montgomery residue
x 2^754 mod p, fully reduced, in 26 limbs of 29 bits (uint32 each); Proj<C> = x, y, z and Aff<C> = x, y, coordinate after
coordinate, which is the coefficient order ld_coeff / st_coeff address (Fp number DEG e + comp of the point)."""
import numpy as np

import pyref

NL, LB = 26, 29
RADIX = 1 << 754
FILL = 0xFFFFFFFF
CURVE_NAMES = ("mnt4753_g1", "mnt4753_g2", "mnt6753_g1", "mnt6753_g2")
ITEM, WACC, TREE_WACC, SCAN, TREE_RUN = range(5)
KIND_NAMES = ("ITEM", "WACC", "TREE_WACC", "SCAN", "TREE_RUN")
ZERO = "proj_zero"            # an expected row that must be (0, one, 0) limb for limb
UNREAD = None                 # a slot no program may read: filled with 0xFFFFFFFF words


# ------------------------------------------------------------------ limbs
def to_limbs(vals):
    """integers below 2^754 -> len(vals) x 26 limbs of 29 bits"""
    vals = list(vals)
    if not vals:
        return np.zeros((0, NL), dtype=np.uint32)
    raw = np.frombuffer(b"".join(int(v).to_bytes(95, "little") for v in vals), dtype=np.uint8).reshape(len(vals), 95)
    bits = np.unpackbits(raw, axis=1, bitorder="little")[:, :NL * LB].reshape(len(vals), NL, LB)
    return (bits.astype(np.uint32) << np.arange(LB, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)


def from_limbs(row):
    return sum(int(v) << (LB * i) for i, v in enumerate(row))


class Form:
    """the internal form of one curve's points"""

    def __init__(self, cid):
        self.cid, self.C = cid, pyref.CURVES[CURVE_NAMES[cid]]
        self.E, self.k, self.p, self.r = self.C.E, self.C.deg, self.C.F.p, self.C.order
        self.rinv = pow(RADIX, -1, self.p)
        self.proj_words, self.aff_words = 3 * self.k * NL, 2 * self.k * NL
        self.one_row = to_limbs([RADIX % self.p] + [0] * (self.k - 1)).reshape(-1)
        self.zero_row = np.concatenate([np.zeros(self.k * NL, dtype=np.uint32), self.one_row, np.zeros(self.k * NL, dtype=np.uint32)])

    def rows(self, coords, n_coords):
        """points as tuples of n_coords canonical Ext elements -> len x (n_coords DEG 26) words"""
        flat = [c * RADIX % self.p for pt in coords for e in pt for c in e]
        return to_limbs(flat).reshape(len(coords), n_coords * self.k * NL)

    def decode(self, row):
        """one Proj row -> (X, Y, Z) canonical; raises AssertionError when a limb has more than 29 bits or a coefficient is not
        below p (the form fp29.h keeps: always fully reduced into [0, p))"""
        row = np.asarray(row).reshape(3 * self.k, NL)
        assert int(row.max()) < 1 << LB, "a limb of %x" % int(row.max())
        vals = [from_limbs(r) for r in row]
        assert all(v < self.p for v in vals), "a coefficient that is not below p"
        c = [v * self.rinv % self.p for v in vals]
        k = self.k
        return tuple(c[0:k]), tuple(c[k:2 * k]), tuple(c[2 * k:3 * k])


# ------------------------------------------------------------------ the group: multiples of one base point
class Group:
    """P = t G and its multiples m P, m an integer mod r, as homogeneous projective points (X : Y : Z) over pyref's field tower
    (None: infinity).  The textbook formulas (add-1998-cmo-2, dbl-2007-bl) with the equal and the opposite case branched, so that
    building thousands of items costs no field inversion; tests/test_gpu_msm_reduce.py holds proj() against pyref.Curve.mul, the
    affine chord-and-tangent definition."""

    def __init__(self, form, t=1):
        self.form, self.C, self.E, self.r, self.t = form, form.C, form.E, form.r, t % form.r
        G = (form.C.G[0], form.C.G[1], form.E.one())
        self.kept = {}
        self.lo = self.hi = None
        self.P = self._ladder(self.t, G)
        self.lo = self._table(self.P)
        self.hi = self._table(self.lo[255] and self.add(self.lo[255], self.P))

    def _table(self, step):
        tab = [None, step]
        for _ in range(254):
            tab.append(self.add(tab[-1], step))
        return tab

    def dbl(self, A):
        if A is None:
            return None
        E = self.E
        X, Y, Z = A
        if E.is_zero(Y):
            return None
        XX, ZZ = E.mul(X, X), E.mul(Z, Z)
        w = E.add(E.mul(self.C.a, ZZ), E.smul(3, XX))
        s = E.smul(2, E.mul(Y, Z))
        ss = E.mul(s, s)
        R = E.mul(Y, s)
        RR = E.mul(R, R)
        XR = E.add(X, R)
        B = E.sub(E.sub(E.mul(XR, XR), XX), RR)
        h = E.sub(E.mul(w, w), E.smul(2, B))
        return (E.mul(h, s), E.sub(E.mul(w, E.sub(B, h)), E.smul(2, RR)), E.mul(s, ss))

    def add(self, A, B):
        if A is None:
            return B
        if B is None:
            return A
        E = self.E
        y1z2, x1z2, z1z2 = E.mul(A[1], B[2]), E.mul(A[0], B[2]), E.mul(A[2], B[2])
        u, v = E.sub(E.mul(B[1], A[2]), y1z2), E.sub(E.mul(B[0], A[2]), x1z2)
        if E.is_zero(v):
            return self.dbl(A) if E.is_zero(u) else None
        vv = E.mul(v, v)
        vvv, R = E.mul(v, vv), E.mul(vv, x1z2)
        a = E.sub(E.sub(E.mul(E.mul(u, u), z1z2), vvv), E.smul(2, R))
        return (E.mul(v, a), E.sub(E.mul(u, E.sub(R, a)), E.mul(vvv, y1z2)), E.mul(vvv, z1z2))

    def _ladder(self, m, A):
        out = None
        for bit in bin(m)[2:]:
            out = self.dbl(out)
            if bit == "1":
                out = self.add(out, A)
        return out

    def proj(self, m):
        """m P as (X : Y : Z), or None"""
        m %= self.r
        if m == 0:
            return None
        if m > self.r // 2:
            X, Y, Z = self.proj(self.r - m)
            return (X, self.E.neg(Y), Z)
        if m not in self.kept:
            if m < 1 << 16:
                self.kept[m] = self.add(self.lo[m & 255], self.hi[m >> 8])
            else:                                    # 16 bits at a time, from the top
                acc = self.proj(m >> 16)
                for _ in range(16):
                    acc = self.dbl(acc)
                self.kept[m] = self.add(acc, self.proj(m & 0xFFFF))
        return self.kept[m]

    def point(self, m):
        """m P affine, or None"""
        A = self.proj(m)
        return None if A is None else self.C.proj_to_affine(*A)

    def item_rows(self, mults, rng):
        """the slots of an input buffer -> len x proj_words: m P in a random projective representative each, infinity as
        (0, y, 0) with y one or random, UNREAD as 0xFF.. words"""
        f, E = self.form, self.form.E
        pts, live = [], []
        for j, m in enumerate(mults):
            if m is UNREAD:
                continue
            pt = self.proj(m)
            z = tuple(1 + rng.randrange(f.p - 1) if c == 0 else rng.randrange(f.p) for c in range(f.k))
            if pt is None:
                pts.append((E.zero(), E.one() if rng.random() < 0.5 else z, E.zero()))
            else:
                pts.append((E.mul(pt[0], z), E.mul(pt[1], z), E.mul(pt[2], z)))
            live.append(j)
        out = np.full((len(mults), f.proj_words), FILL, dtype=np.uint32)
        if live:
            out[live] = f.rows(pts, 3)
        return out

    def salt_rows(self):
        """S0 = G, S1 = 2 G in internal affine form, as msm_impl.h make_salts documents"""
        G = self.C.G
        return self.form.rows([G, self.C.add(G, G)], 2)

    def same_point(self, row, m):
        """None, or how the decoded row differs from m P: the row is divided by its Z and the affine point compared with
        m P = (Xe : Ye : Ze), i.e. x Ze == Xe and y Ze == Ye"""
        try:
            X, Y, Z = self.form.decode(row)
        except AssertionError as e:
            return str(e)
        E = self.E
        got, want = self.C.proj_to_affine(X, Y, Z), self.proj(m)
        if got is None and want is not None:
            return "infinity (X %s zero, Y %s zero) where a point is due" % ("is" if not any(X) else "not", "is" if not any(Y) else "not")
        if got is None:
            return None if any(Y) else "(X, 0, 0): no point at all"
        if want is not None and E.mul(got[0], want[2]) == want[0] and E.mul(got[1], want[2]) == want[1]:
            return None
        return "another point than %d P" % (m if m <= self.r // 2 else m - self.r)


# ------------------------------------------------------------------ the definition
class In:
    """a WaveReduceIn: item (w, k) = slot (w count + k) stride + offset of its buffer"""

    def __init__(self, stride, offset, count, mode, valid=FILL):
        self.stride, self.offset, self.count, self.mode, self.valid = stride, offset, count, mode, valid

    def flat(self, w, k):
        return (w * self.count + k) * self.stride + self.offset

    def words(self, base):
        return [base, self.stride, self.offset, self.count, self.mode, self.valid]


class Launch:
    """one reduce_level: per_input * n_inputs programs; program gb = which per_input + blk reduces segment blk % segs of window
    blk / segs of input `which`"""

    def __init__(self, ins, per_input, segs, L, tpw, run_if=None):
        self.ins, self.per_input, self.n_inputs, self.segs, self.L, self.tpw, self.run_if = ins, per_input, len(ins), segs, L, tpw, run_if
        assert 1 <= len(ins) <= 3 and (run_if is None or len(run_if) == self.programs())
        assert all(i.mode in (0, 1) or (i.mode == 2 and tpw == 64 and len(ins) == 1) for i in ins)

    def programs(self):
        return self.per_input * self.n_inputs

    def segment(self, gb):
        """-> (input, w, item0, skipped)"""
        which, blk = divmod(gb, self.per_input)
        i = self.ins[which]
        w, seg = divmod(blk, self.segs)
        item0 = seg * self.tpw * self.L
        return i, w, item0, w * i.count + item0 >= i.valid

    def runs(self, gb):
        return self.run_if is None or self.run_if[gb] != 0

    def reads(self):
        """every buffer slot a program may load (an item with k < count of a segment that is not skipped)"""
        out = set()
        for gb in range(self.programs()):
            i, w, item0, skipped = self.segment(gb)
            if self.runs(gb) and not skipped:
                out.update(i.flat(w, k) for k in range(item0, min(item0 + self.tpw * self.L, i.count)))
        return out

    def rows_of(self, gb):
        i = self.ins[gb // self.per_input]
        if i.mode == 2:
            blk = gb % self.per_input
            return [(blk * 64 + l) * 2 + e for l in range(64) for e in (0, 1)]
        return [gb * 3] if i.mode == 1 else [gb * 3, gb * 3 + 1, gb * 3 + 2]

    def expect(self, mult, r):
        """mult: the buffer's slots as multiples -> {output row: multiple mod r | ZERO}; a row that is absent is never written"""
        out = {}
        for gb in range(self.programs()):
            if not self.runs(gb):
                continue
            i, w, item0, skipped = self.segment(gb)
            rows = self.rows_of(gb)
            if skipped:
                out.update((row, ZERO) for row in rows)
                continue
            x = [[0] * self.L for _ in range(self.tpw)]                    # x[g][i]
            for j in range(self.tpw * self.L):
                if item0 + j < i.count:
                    m = mult[i.flat(w, item0 + j)]
                    assert m is not UNREAD, "the model reads a slot that is marked unread"
                    assert item0 + j + w * i.count < i.valid or m % r == 0, "a padding slot that is not infinity"
                    x[j % self.tpw][j // self.tpw] = m
            run = [sum(xs) for xs in x]
            wacc = [sum(n * v for n, v in enumerate(xs)) for xs in x]
            if i.mode == 0:
                vals = [sum(run), sum(wacc), sum(g * v for g, v in enumerate(run))]
            elif i.mode == 1:
                vals = [sum(run)]
            else:
                vals = [v for l in range(64) for v in (run[l], wacc[l])]
            out.update((row, v % r) for row, v in zip(rows, vals))
        return out

    def out_rows(self):
        """rows of the output buffer the launch may touch at all (its extent): 3 per program, or 128 per program in mode 2"""
        return self.programs() * (128 if self.ins[0].mode == 2 else 3)


def heavy_combine(partials, order, chunk_start, r):
    """-> {bucket: multiple}"""
    return {order[h]: sum(partials[chunk_start[h]:chunk_start[h + 1]]) % r for h in range(len(chunk_start) - 1)}


# ------------------------------------------------------------------ the replay: which collisions a segment's items meet
class Step:
    def __init__(self, kind, off, i):
        self.kind, self.off, self.i = kind, off, i
        self.detour = {}          # group -> salt the detour must take (0: S0 = G, 1: S1 = 2 G)
        self.inf = {}             # group -> "p", "q" or "pq": which operand of the step is infinity
        self.detour_inf = set()   # groups whose detour itself meets an infinite operand (p + S or (p + S) + q is infinity)

    def __repr__(self):
        return "%s(off %d, i %d: detour %s, inf %s)" % (KIND_NAMES[self.kind], self.off, self.i, sorted(self.detour), sorted(self.inf))


def replay(shim, mode, L, tpw, items, r, t=1):
    """The schedule over the integers mod r.  items: the segment's multiples of P = t G (shorter than tpw L: the rest is padding)
    -> (run, wacc, published runW, [Step])"""
    import ctypes
    LT = tpw.bit_length() - 1
    out = (ctypes.c_int * 6)()
    shim.t_wave_step(mode, L, LT, 0, out)
    nst = out[1]
    run, wacc, published, steps = [0] * tpw, [0] * tpw, None, []
    for step in range(nst):
        shim.t_wave_step(mode, L, LT, step, out)
        kind, off, i, publish = out[2], out[3], out[4], out[5]
        if publish:
            published, run[0] = run[0], 0
        exch = list(wacc if kind == TREE_WACC else run)
        dst = wacc if kind in (WACC, TREE_WACC) else run
        st = Step(kind, off, i)
        for g in range(tpw):
            k = g + tpw * i
            if not shim.t_wave_step_active(kind, off, g, tpw, int(k < len(items))):
                continue
            q = items[k] if kind == ITEM else (run[g] if kind == WACC else exch[g + off])
            p = dst[g]
            p, q = p % r, q % r
            if p == 0 or q == 0:
                st.inf[g] = ("p" if p == 0 else "") + ("q" if q == 0 else "")
            elif p == q:
                pg = p * t % r                                            # p in units of G
                salt = 1 if pg in (1, r - 1) else 0                       # S0 = G has the x of p: take S1 = 2 G
                st.detour[g] = salt
                s = salt + 1
                if (pg + s) % r == 0 or (2 * pg + s) % r == 0:
                    st.detour_inf.add(g)
            dst[g] = (p + q) % r
        steps.append(st)
    return run, wacc, published, steps


def collisions(steps):
    """-> {(kind, off or i): sorted groups that detour}"""
    return {(s.kind, s.i if s.kind in (ITEM, WACC) else s.off): sorted(s.detour) for s in steps if s.detour}
