"""The lane-split tower arithmetic of the G2 kernels on the card, operation by operation: F2S<P4, 13> (an Fq2 element over a lane
pair) and F3S<P6, 11> (an Fq3 element over a lane triple) of ginger-lib_amd/csrc/msm_kernels.h, and the out-of-line inverses of
the table builder (dev_fp_inv, DevInv).  These forms exist on the device only; tests/device_shim/tower_ops.hip wraps them in
test kernels over the shipped headers (one code object, build/tower_ops.co, loaded through the module API of asm_card.Card).
The device build of the one-lane form F1S<P4> / F1S<P6> (aff_kernels.h) runs through the same kernel template; it has no
mul_sub_mul and no sel, and its sub_lazy is the lazy one: a - b + p as it stands, below 2p, not reduced.

The referee is Python integers.  The limbs are Montgomery residues to RADIX = 2^754, so for raw values
    mul(a, b)   = a b RADIX^-1              (in Fp[X]/(X^k - NR), coefficient by coefficient mod p)
    one()       = (RADIX mod p, 0, ..)
    inv(a)      = the raw r with mul(r, a) == one(), i.e. a^-1 RADIX^2;  inv(0) = 0
    add / sub / dbl / neg / sub_lazy are the plain operations mod p (the split forms return sub_lazy fully reduced).
Every comparison is exact, limb for limb, against the canonical value below p in 26 limbs of 29 bits, so a result that is not
fully reduced or a limb above 29 bits fails as well.

The CPU part (no marker) checks these identities, the operand sets and the cross-compile of the code object for gfx950."""
import functools
import itertools

import numpy as np
import pytest

import asm_card
import pyref
import shim_build
import support as S

CO = shim_build.BUILD + "/tower_ops.co"
KERNELS = ("tower_ops_f2s", "tower_ops_f3s", "tower_ops_f1s_p4", "tower_ops_f1s_p6", "dev_inv_p4", "dev_inv_p6", "dev_inv_fq2", "dev_inv_fq3")

NL, LB = 26, 29
RADIX = 1 << 754
FILL = 0xFFFFFFFF
OPS = ("add", "sub", "dbl", "neg", "mul", "sqr", "mul_sub_mul", "sub_lazy", "inv", "is_zero", "eq", "one", "sel", "swap", "bcast0",
       "bcast1")                                    # the kernel's op numbers, in this order
F2S_ONLY = ("sel", "swap", "bcast0", "bcast1")
TOWER_ONLY = ("mul_sub_mul",)                        # F2S and F3S
BOOLEAN = ("is_zero", "eq")
# the smallest; groups per wave (triples, pairs, single lanes); groups per 256-lane block
N_EDGES = (1, 21, 22, 32, 33, 64, 65, 84, 85, 128, 129, 256, 257)


class Tower:
    """one lane-split field: its kernel, its Ext referee and the raw-limb meaning of every operation"""

    def __init__(self, name, kernel, field, k, nr):
        self.name, self.kernel, self.k, self.p = name, kernel, k, field.p
        self.E = pyref.Ext(field, k, nr)
        self.tpw = 64 // k                           # groups per wave
        self.rinv = pow(RADIX, -1, self.p)
        self.one = (RADIX % self.p,) + (0,) * (k - 1)
        self.pm1 = (self.p - 1,) * k

    def mul(self, a, b):
        return self.E.smul(self.rinv, self.E.mul(a, b))

    def inv(self, a):
        if self.E.is_zero(a):
            return self.E.zero()
        return self.E.smul(RADIX * RADIX % self.p, self.E.inv(a))

    def apply(self, op, a, b, c, d):
        """the group's result: a k-tuple of raw values, or a bool; sel takes its condition per lane from bit 0 of c"""
        E = self.E
        if op == "add":
            return E.add(a, b)
        if op == "sub_lazy" and self.k == 1:
            return (a[0] - b[0] + self.p,)               # F1S: fp_sub_lazy, the operand of one product, in (0, 2p)
        if op in ("sub", "sub_lazy"):
            return E.sub(a, b)
        if op == "dbl":
            return E.add(a, a)
        if op == "neg":
            return E.neg(a)
        if op == "mul":
            return self.mul(a, b)
        if op == "sqr":
            return self.mul(a, a)
        if op == "mul_sub_mul":
            return E.sub(self.mul(a, b), self.mul(c, d))
        if op == "inv":
            return self.inv(a)
        if op == "is_zero":
            return E.is_zero(a)
        if op == "eq":
            return a == b
        if op == "one":
            return self.one
        if op == "sel":
            return tuple(x if z & 1 else y for x, y, z in zip(a, b, c))
        if op == "swap":
            return (a[1], a[0])
        if op == "bcast0":
            return (a[0], a[0])
        if op == "bcast1":
            return (a[1], a[1])
        raise KeyError(op)


TOWERS = {"f2s": Tower("f2s", "tower_ops_f2s", pyref.P4, 2, 13), "f3s": Tower("f3s", "tower_ops_f3s", pyref.P6, 3, 11),
          "f1s_p4": Tower("f1s_p4", "tower_ops_f1s_p4", pyref.P4, 1, 1), "f1s_p6": Tower("f1s_p6", "tower_ops_f1s_p6", pyref.P6, 1, 1)}


# ------------------------------------------------------------------ operands
def core_values(T):
    p = T.p
    k6 = [0, 1, p - 1, (p + 1) // 2, RADIX % p, 1 << 752]
    assert (1 << 752) < p and len(set(k6)) == 6
    if T.k == 1:
        return S.edge_values(p)                      # one lane: every ordered pair of the edge values, as the plain fp_mul test has
    return k6 if T.k == 2 else k6[:4]


@functools.lru_cache(maxsize=None)
def set_a(name):
    """all tuples over the core values, the all-(p-1) element first: the ordered pairs A x A then start with the all-(p-1) pair,
    so that every prefix of them holds it"""
    T = TOWERS[name]
    tuples = list(itertools.product(core_values(T), repeat=T.k))
    A = [T.pm1] + [t for t in tuples if t != T.pm1]
    assert len(A) == len(set(A)) and (len(A) == {2: 36, 3: 64}[T.k] if T.k > 1 else len(A) >= 55) and T.E.zero() in A
    return A


@functools.lru_cache(maxsize=None)
def set_b(name):
    """every edge value in one slot with p - 1 in the others, and in all slots at once"""
    T = TOWERS[name]
    V = S.edge_values(T.p)
    assert len(V) >= 55 and len(set(V)) == len(V) and max(V) == T.p - 1
    B = []
    for v in V:
        for j in range(T.k):
            B.append(tuple(v if i == j else T.p - 1 for i in range(T.k)))
        B.append((v,) * T.k)
    assert len(B) == len(V) * (T.k + 1) and T.pm1 in B and T.E.zero() in B
    return B


def random_elements(T, count, seed):
    rng = pyref.Rng(seed)
    return [tuple(rng.field_elem(T.p) for _ in range(T.k)) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def quads(name, cls):
    """the rows of an operand class: (a, b, c, d) per group; a unary op takes a, a binary one (a, b), mul_sub_mul all four (the
    list of pairs zipped with itself reversed).  The assertions are about the inputs: that the rows the class exists for are there."""
    T = TOWERS[name]
    if cls == "A":
        A = set_a(name)
        pairs = [(a, b) for a in A for b in A]
        assert len(pairs) == len(A) ** 2 and (T.k == 1 or len(pairs) == {2: 1296, 3: 4096}[T.k])
        assert pairs[0] == (T.pm1, T.pm1) and len(pairs) > max(N_EDGES)
        eq = [T.apply("eq", a, b, None, None) for a, b in pairs]
        assert [i for i, e in enumerate(eq) if e] == [i * len(A) + i for i in range(len(A))]     # the diagonal, nowhere else
        assert sum(T.apply("is_zero", a, None, None, None) for a in A) == 1
        one_slot = [(a, b) for a, b in pairs if a != b and sum(x == y for x, y in zip(a, b)) == T.k - 1]
        assert len(one_slot) >= len(A)                                   # equal in all coefficients but one: what eq exists for
        assert any(b == T.E.neg(a) and not T.E.is_zero(a) for a, b in pairs)
        for j in range(T.k):                                             # a zero coefficient in slot j alone
            assert any(a[j] == 0 and all(a[i] != 0 for i in range(T.k) if i != j) for a in A)
    elif cls == "B":
        B = set_b(name)
        pairs = list(zip(B, B[1:] + B[:1])) + [(b, T.pm1) for b in B]
        assert (T.pm1, T.pm1) in pairs
    else:
        assert cls == "R"
        el = random_elements(T, 4000, 7540 + T.k)
        pairs = list(zip(el[:2000], el[2000:]))
        assert len(pairs) == 2000
    return [ab + cd for ab, cd in zip(pairs, pairs[::-1])]


def expected(T, op, mode, rows):
    """per group: mode 0 op(a, b, c, d); mode 1 the same in even groups and op(b, a, d, c) in odd ones (sel keeps c)"""
    out = []
    for g, (a, b, c, d) in enumerate(rows):
        if mode == 1 and g & 1:
            out.append(T.apply(op, b, a, c if op == "sel" else d, c))
        else:
            out.append(T.apply(op, a, b, c, d))
    return out


# ------------------------------------------------------------------ limbs and rows
def to_limbs(vals):
    """integers below 2^754 -> len(vals) x 26 limbs of 29 bits"""
    n = len(vals)
    raw = np.frombuffer(b"".join(int(v).to_bytes(96, "little") for v in vals), dtype=np.uint8).reshape(n, 96)
    bits = np.unpackbits(raw, axis=1, bitorder="little")
    assert not bits[:, NL * LB:].any()
    w = (np.uint32(1) << np.arange(LB, dtype=np.uint32))
    return (bits[:, :NL * LB].reshape(n, NL, LB).astype(np.uint32) * w).sum(axis=2, dtype=np.uint32)


def from_limbs(row):
    return sum(int(v) << (LB * i) for i, v in enumerate(row))


def lane_rows(T, n):
    """row (= global lane) of coefficient j of group g, as the shipped split kernels map tasks to lanes -> n x k indices"""
    g = np.arange(n)[:, None]
    return (g // T.tpw) * 64 + (g % T.tpw) * T.k + np.arange(T.k)[None, :]


def blocks_for(T, n):
    waves = (n + T.tpw - 1) // T.tpw
    return max(1, (waves + 3) // 4)


def place(T, elems, nrows):
    """k-tuples, one per group -> nrows x 26 limbs (rows that belong to no group stay zero: no lane reads them)"""
    out = np.zeros((nrows, NL), dtype=np.uint32)
    if elems:
        out[lane_rows(T, len(elems)).reshape(-1)] = to_limbs([x for e in elems for x in e])
    return out


# ------------------------------------------------------------------ the code object
def build_code_object():
    """build/tower_ops.co from the shipped headers, with the product's compiler flags; rebuilt when a source is newer.
    -> seconds spent compiling (0.0: up to date)"""
    return shim_build.device_shim("tower_ops.hip", CO, genco=True)


class Device:
    def __init__(self):
        self.build_seconds = build_code_object()
        self.card = asm_card.Card()
        self.module = self.card.load(CO)
        self.fn = {k: self.card.function(self.module, k) for k in KERNELS}

    def _buffers(self, arrays):
        addrs = []
        for a in arrays:
            a = np.ascontiguousarray(a, dtype=np.uint32)
            addrs.append(self.card.malloc(a.nbytes))
            self.card.upload(addrs[-1], a)
        return addrs

    @staticmethod
    def _words(*addrs):
        return [w for a in addrs for w in (a & 0xFFFFFFFF, a >> 32)]

    def tower_op(self, T, op, mode, n, rows):
        """rows: at least n quads.  -> (out, flags) with one guard row behind the lanes of the launch, 0xFF.. before the call"""
        blocks = blocks_for(T, n)
        nrows = blocks * 256
        assert n >= 1 and len(rows) >= n and lane_rows(T, n).max() < nrows       # every row a live lane touches is inside
        ins = [place(T, [r[i] for r in rows[:n]], nrows) for i in range(4)]
        out = np.full((nrows + 1, NL), FILL, dtype=np.uint32)
        flags = np.full(nrows + 1, FILL, dtype=np.uint32)
        addrs = self._buffers(ins + [out, flags])
        try:
            karg = np.array([OPS.index(op), mode, n, 0] + self._words(*addrs), dtype=np.uint32)
            self.card.launch(self.fn[T.kernel], (blocks, 1), 256, karg)
            self.card.download(addrs[4], out)
            self.card.download(addrs[5], flags)
        finally:
            for a in addrs:
                self.card.free(a)
        return out, flags

    def dev_inv(self, kernel, k, elems, threads):
        """one element of k coefficients per lane -> the kernel's rows, one guard row behind the last element"""
        n = len(elems)
        a = to_limbs([x for e in elems for x in e]).reshape(n, k * NL)
        out = np.full((n + 1, k * NL), FILL, dtype=np.uint32)
        addrs = self._buffers([a, out])
        try:
            karg = np.array([n, 0] + self._words(*addrs), dtype=np.uint32)
            self.card.launch(self.fn[kernel], ((n + threads - 1) // threads, 1), threads, karg)
            self.card.download(addrs[1], out)
        finally:
            for x in addrs:
                self.card.free(x)
        return out

    def close(self):
        self.card.close()
        assert self.card.allocs == []


@pytest.fixture(scope="module")
def dev(gpu):
    d = Device()
    print("\ntower_ops.co: %s" % ("up to date" if d.build_seconds == 0.0 else "built in %.1f s" % d.build_seconds))
    yield d
    d.close()


def check(dev, T, op, mode, n, rows, want, what):
    """one launch on the first n rows against the referee: the live rows limb for limb, every other row and the guard untouched.
    -> None, or a message naming the first differing group"""
    out, flags = dev.tower_op(T, op, mode, n, rows)
    idx = lane_rows(T, n)
    exp_out = np.full_like(out, FILL)
    exp_flags = np.full_like(flags, FILL)
    if op in BOOLEAN:
        exp_flags[idx.reshape(-1)] = np.repeat(np.array([1 if w else 0 for w in want[:n]], dtype=np.uint32), T.k)
    else:
        exp_out[idx.reshape(-1)] = to_limbs([x for w in want[:n] for x in w])
    if np.array_equal(out, exp_out) and np.array_equal(flags, exp_flags):
        return None
    bad = np.nonzero((out != exp_out).any(axis=1) | (flags != exp_flags))[0]
    r = int(bad[0])
    wave, lane = r // 64, r % 64
    where = "row %d (wave %d, lane %d" % (r, wave, lane)
    g = wave * T.tpw + lane // T.k
    if r < len(flags) - 1 and lane < T.tpw * T.k and g < n:
        where += ", group %d coefficient %d, operands %s" % (g, lane % T.k, [["%x" % x for x in e] for e in rows[g]])
    elif r == len(flags) - 1:
        where += ", the guard row"
    else:
        where += ", no live group"
    return "%s %s %s mode %d n %d: %d rows differ; first at %s): out %x against %x, flag %x against %x" % (
        what, T.name, op, mode, n, len(bad), where, from_limbs(out[r]), from_limbs(exp_out[r]), int(flags[r]), int(exp_flags[r]))


# ------------------------------------------------------------------ CPU: the referee, the operand sets, the cross-compile
@pytest.mark.parametrize("name", sorted(TOWERS))
def test_referee_identities(name):
    """the raw-limb meaning of the operations, as the module docstring states it, on the core set and the edge set"""
    T = TOWERS[name]
    E, p = T.E, T.p
    assert T.one[0] == (1 << 754) % p and (T.rinv << 754) % p == 1
    raw = lambda e: E.smul(RADIX, e)                                           # canonical element -> its Montgomery form
    assert raw(E.one()) == T.one
    els = set_a(name) + set_b(name) + random_elements(T, 20, 99)
    for a in els:
        assert T.mul(a, T.one) == a and T.mul(T.one, a) == a
        r = T.inv(a)
        if E.is_zero(a):
            assert E.is_zero(r)
        else:
            assert T.mul(r, a) == T.one and all(0 <= x < p for x in r)
    x, y = random_elements(T, 2, 5)
    assert T.mul(raw(x), raw(y)) == raw(E.mul(x, y))                           # the Montgomery product of the forms is the form of
    assert T.inv(raw(x)) == raw(E.inv(x))                                      # the product, and likewise the inverse
    assert T.apply("mul_sub_mul", raw(x), raw(y), raw(y), raw(x)) == E.zero()
    assert T.apply("sqr", T.pm1, None, None, None) == T.mul(T.pm1, T.pm1) != E.zero()


@pytest.mark.parametrize("name", sorted(TOWERS))
def test_operand_sets_hold_the_rows_they_exist_for(name):
    T = TOWERS[name]
    for cls in "ABR":
        rows = quads(name, cls)                                                # the assertions on the inputs run in there
        assert all(len(r) == 4 and all(len(e) == T.k and all(0 <= x < T.p for x in e) for e in r) for r in rows)
    rows = quads(name, "A")
    for n in N_EDGES:                                                          # the prefixes the small launches run on
        assert n <= len(rows) and (T.pm1, T.pm1) == rows[0][:2]
    assert (T.pm1, T.pm1) in [r[:2] for r in quads(name, "B")]
    # the lane map: pairs fill a wave, triples leave lane 63 of every wave idle; rows of distinct (group, coefficient) are distinct
    idx = lane_rows(T, 4 * T.tpw + 1)
    assert len(set(idx.reshape(-1).tolist())) == idx.size and idx[T.tpw, 0] == 64
    assert (63 in idx.reshape(-1).tolist()) == (T.k != 3)
    # limbs round trip, and the canonical limbs of p - 1 are what the kernels must return
    v = [0, 1, T.p - 1, (1 << 754) - 1]
    L = to_limbs(v)
    assert [from_limbs(r) for r in L] == v and int(L.max()) < 1 << LB


def test_code_object_cross_compiles_for_gfx950():
    build_code_object()
    blob = open(CO, "rb").read()
    assert b"gfx950" in blob
    for k in KERNELS:
        assert k.encode() in blob, k


# ------------------------------------------------------------------ GPU
def ops_of(T):
    return [op for op in OPS if (T.k == 2 or op not in F2S_ONLY) and (T.k > 1 or op not in TOWER_ONLY)]


CASES = [(name, op, cls) for name in sorted(TOWERS) for cls in "ABR" for op in ops_of(TOWERS[name])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,op,cls", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_tower_op_against_python_integers(dev, name, op, cls):
    """class A (all tuples over the core values, all ordered pairs): every n around the group, wave and block edges on a prefix that
    starts with the all-(p-1) pair, then the full set; divergent (mode 1) at the full set and at one group past a full wave.
    Classes B (edge values slot by slot) and R (seeded random): the full set, uniform and divergent."""
    T = TOWERS[name]
    rows = quads(name, cls)
    want = {m: expected(T, op, m, rows) for m in (0, 1)}
    past_wave = T.tpw + 1                                                      # 33 pairs / 22 triples / 65 single lanes
    assert past_wave in N_EDGES
    runs = [(0, len(rows)), (1, len(rows)), (1, past_wave)]
    if cls == "A":
        runs += [(0, n) for n in N_EDGES]
    failures = [f for f in (check(dev, T, op, m, n, rows, want[m], cls) for m, n in runs) if f]
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,field", [("dev_inv_p4", pyref.P4), ("dev_inv_p6", pyref.P6)])
def test_dev_fp_inv_on_the_edge_values(dev, kernel, field):
    """dev_fp_inv<P> (a^(p-2) by out-of-line products) on every edge value, one per lane: a^-1 RADIX^2, 0 -> 0"""
    p = field.p
    V = S.edge_values(p)
    assert len(V) >= 55 and V[0] == 0 and max(V) == p - 1
    out = dev.dev_inv(kernel, 1, [(v,) for v in V], 256)
    want = [pow(v, -1, p) * RADIX * RADIX % p if v else 0 for v in V]
    assert all(w * v % p == RADIX * RADIX % p for w, v in zip(want, V) if v)
    exp = np.concatenate([to_limbs(want), np.full((1, NL), FILL, dtype=np.uint32)])
    bad = np.nonzero((out != exp).any(axis=1))[0]
    assert bad.size == 0, (kernel, len(bad), "first: element %d = %x: %x against %x" % (
        bad[0], V[min(bad[0], len(V) - 1)], from_limbs(out[bad[0]]), from_limbs(exp[bad[0]])))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,name", [("dev_inv_fq2", "f2s"), ("dev_inv_fq3", "f3s")])
def test_dev_inv_of_the_towers(dev, kernel, name):
    """DevInv<F2<P4, 13>> / DevInv<F3<P6, 11>> as the table builder instantiates them, on A, B and 200 random elements"""
    T = TOWERS[name]
    sets = {"A": set_a(name), "B": set_b(name), "R": random_elements(T, 200, 31 + T.k)}
    failures = []
    for cls, els in sets.items():
        out = dev.dev_inv(kernel, T.k, els, 64)
        want = [T.inv(e) for e in els]
        exp = np.concatenate([to_limbs([x for w in want for x in w]).reshape(len(els), T.k * NL),
                              np.full((1, T.k * NL), FILL, dtype=np.uint32)])
        bad = np.nonzero((out != exp).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            failures.append("%s %s: %d elements differ; first %d = %s" % (
                kernel, cls, len(bad), i, ["%x" % x for x in els[min(i, len(els) - 1)]]))
    assert not failures, failures
