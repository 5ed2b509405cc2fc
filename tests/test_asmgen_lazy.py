"""The lazy G1 bucket update (asmgen/field.py mul27 / sqr27 / dual27 / lazy_diff / zero_or_p_mask and the kernel of
asmgen/g1_xyzz.py built on them) in asmgen/sim.py -- no GPU.

REDC27(a, b) = a b 2^-783 mod p with 27 digits: below p + 2^733 for any operands the bound checker admits, so nothing is
reduced behind a product and the differences stay a - b + 2^s p.  Checked here, for both primes:
* every routine against Python integers, with random operands and with every operand at its declared bound (limbs 0 .. 24 at
  2^29 - 1, the top limb at its cap), the mad counts, the columns the dual product closes in two parts;
* the bound checker: it accepts the kernel's ranges (building the kernel runs it) and refuses an unsplit dual product of lazy
  operands, a 10 p squaring operand, a difference that can turn negative;
* the {0, p} test;
* the whole kernel in both launch forms against the affine group law: the special lists of tests/test_asmgen.py, one list of 60
  entries (the lazy ranges over a long chain), acc == q and acc == -q reached by a running sum (P = 0 mod p arrives there as a
  multiple k p, 4 <= k <= 8, whose square leaves REDC27 as exactly p: test_a_zero_difference_squares_to_p), every output below p.
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
import test_asmgen as TA                                          # noqa: E402  (its _execute: the simulator, or the card runner)
import test_asmgen_acc_persist as TP                              # noqa: E402  (its memory image and launchers of both forms)
from asmgen import g1_xyzz                                        # noqa: E402
from asmgen.field import Bound, BoundError, Chain, FieldGen, LB, LM, NL, limbs, run, runv, unlimbs   # noqa: E402
from asmgen.isa import Prog, S, V                                 # noqa: E402
from asmgen.sim import Memory, Wave                               # noqa: E402

R = 1 << 754
RD = 1 << 783
EPS = 1 << 733
TOP = LB * (NL - 1)
AR, B_X, B_P, B_W, B_T = Bound(1, EPS), Bound(5, EPS), Bound(9, EPS), Bound(3, EPS), Bound(7, EPS)


def sl(i):
    return V(20 + NL * i, NL)


def _field(tag):
    p = pyref.FIELDS[tag].p
    g = Prog("t")
    f = FieldGen(g, p, 24, 50, 21, 20)
    chA = Chain(V(248, 2), V(252), V(253), S(14, 2), S(16, 2))
    chB = Chain(V(250, 2), V(254), V(255), S(18, 2), S(22, 2))
    f.load_constants()
    return p, g, f, chA, chB


def _at_bound(p, bd):
    """every limb at the largest value the checker assumes for the bound"""
    return ((bd.value(p) >> TOP) << TOP) | ((1 << TOP) - 1)


def _operands(p, bd, rnd, extra=()):
    """64 lanes: the bound, 0, the given values, random values below the bound"""
    v = [_at_bound(p, bd), 0] + list(extra)
    return v + [rnd.randrange(bd.value(p) + 1) for _ in range(64 - len(v))]


def _put(w, s, vals):
    for l in range(64):
        for i in range(NL):
            w.V[s.idx + i][l] = (vals[l] >> (LB * i)) & (LM if i < NL - 1 else 0xFFFFFFFF)
        assert vals[l] >> (TOP + 32) == 0


def _get(w, s, normalised=True):
    out = []
    for l in range(64):
        ls = [int(x) for x in w.V[s.idx:s.idx + NL, l]]
        assert not normalised or max(ls[:NL - 1]) <= LM
        out.append(unlimbs(ls))
    return out


def _run(g, puts):
    g.s_endpgm()
    return TA._execute(g, lambda w: [_put(w, s, v) for s, v in puts])


@pytest.mark.parametrize("tag", ["p4", "p6"])
def test_products_with_27_digits(tag):
    rnd = random.Random(31)
    p, g, f, chA, chB = _field(tag)
    inv = pow(RD, -1, p)
    # mul27 with the widest pair the kernel forms (P PP: 9 p by an almost reduced value), over an operand's slot
    assert runv(f.mul27(chA, sl(0), sl(1), sl(2), B_P, AR, r=sl(0))).value(p) < p + EPS
    a, b = _operands(p, B_P, rnd), _operands(p, AR, rnd)
    a[1], b[1] = a[0], b[0] - 1                                     # lane 1: a zero operand on either side of lanes 1, 2
    a[2], b[2] = 0, b[0]
    w = _run(g, [(sl(0), a), (sl(1), b)])
    for l, v in enumerate(_get(w, sl(0))):
        assert v % p == a[l] * b[l] * inv % p and v < p + EPS, l
    assert w.hist["v_mad_u64_u32"] == 1378
    # sqr27 of P at 9 p: the doubled top limb is just inside 32 bits
    p, g, f, chA, chB = _field(tag)
    runv(f.sqr27(chA, sl(0), sl(1), sl(2), B_P))
    w = _run(g, [(sl(0), a)])
    for l, v in enumerate(_get(w, sl(2))):
        assert v % p == a[l] * a[l] * inv % p and v < p + EPS, l
    assert w.hist["v_mad_u64_u32"] == 1053
    # dual27 W T + V PPP with W and T lazy: two parts in columns 25, 26 (MNT4) / 25 (MNT6), found by the checker
    p, g, f, chA, chB = _field(tag)
    runv(f.dual27(chA, chB, sl(0), sl(1), sl(2), sl(3), sl(4), B_W, B_T, AR, AR))
    assert f.last_split == ([25, 26] if tag == "p4" else [25])
    ops = [_operands(p, bd, rnd) for bd in (B_W, B_T, AR, AR)]
    for o in ops:
        o[1] = o[0]
    ops[0][1] = ops[2][2] = 0
    w = _run(g, list(zip((sl(0), sl(1), sl(2), sl(3)), ops)))
    for l, v in enumerate(_get(w, sl(4))):
        assert v % p == (ops[0][l] * ops[1][l] + ops[2][l] * ops[3][l]) * inv % p and v < p + EPS, l
    assert w.hist["v_mad_u64_u32"] == 2054


@pytest.mark.parametrize("tag", ["p4", "p6"])
def test_lazy_differences_are_exact_and_normalised(tag):
    rnd = random.Random(32)
    p, g, f, chA, chB = _field(tag)
    bp = runv(f.lazy_diff(chA, sl(0), [(sl(1), 1)], 3, sl(4), AR, [B_X]))                  # P = U2 - X + 8 p
    bx = runv(f.lazy_diff(chB, sl(0), [(sl(2), 1), (sl(3), 2)], 2, sl(5), AR, [AR, AR]))   # X3 = RR - PPP - 2 Q + 4 p
    bn = runv(f.lazy_diff(chA, None, [(sl(2), 1)], 1, sl(6), None, [AR]))                  # 2 p - V
    bt = runv(f.lazy_diff(chA, sl(1), [(sl(2), 1)], 1, sl(1), B_X, [AR]))                  # T = X3 - Q + 2 p, over its operand
    assert (bp.k, bx.k, bn.k, bt.k) == (9, 5, 2, 7)
    top_ar = p + EPS
    a = [0, top_ar, 0, top_ar] + [rnd.randrange(top_ar + 1) for _ in range(60)]
    x = [5 * p + EPS, 0, 0, 5 * p + EPS] + [rnd.randrange(5 * p + EPS + 1) for _ in range(60)]   # the accumulator at 5 p entering P
    c = [top_ar, 0, top_ar, 0] + [rnd.randrange(top_ar + 1) for _ in range(60)]
    d = [top_ar, 0, 0, top_ar] + [rnd.randrange(top_ar + 1) for _ in range(60)]
    w = _run(g, [(sl(0), a), (sl(1), x), (sl(2), c), (sl(3), d)])
    assert _get(w, sl(4)) == [a[l] - x[l] + 8 * p for l in range(64)]
    assert _get(w, sl(5)) == [a[l] - c[l] - 2 * d[l] + 4 * p for l in range(64)]
    assert _get(w, sl(6)) == [2 * p - c[l] for l in range(64)]
    assert _get(w, sl(1)) == [x[l] - c[l] + 2 * p for l in range(64)]
    assert min(_get(w, sl(4))) > 0 and max(_get(w, sl(4))) <= bp.value(p)


@pytest.mark.parametrize("tag", ["p4", "p6"])
def test_the_update_chain_with_the_accumulator_at_its_bounds(tag):
    """P = U2 - X + 8 p with X at 5 p (and at 0 under the largest U2), then PP = P^2 and PPP = P PP: the path the parked X takes"""
    rnd = random.Random(33)
    p, g, f, chA, chB = _field(tag)
    inv = pow(RD, -1, p)
    bp = runv(f.lazy_diff(chA, sl(0), [(sl(1), 1)], 3, sl(0), AR, [B_X]))
    runv(f.sqr27(chA, sl(0), sl(2), sl(3), bp))
    runv(f.mul27(chB, sl(0), sl(3), sl(2), bp, AR, r=sl(0)))
    u2 = [0, _at_bound(p, AR)] + [rnd.randrange(p + EPS) for _ in range(62)]
    x = [_at_bound(p, B_X), 0] + [rnd.randrange(5 * p + EPS) for _ in range(62)]
    w = _run(g, [(sl(0), u2), (sl(1), x)])
    for l in range(64):
        P = u2[l] - x[l] + 8 * p
        assert P > 0
        pp, ppp = _get(w, sl(3))[l], _get(w, sl(0))[l]
        assert pp % p == P * P * inv % p and pp < p + EPS
        assert ppp % p == P * pp * inv % p and ppp < p + EPS


@pytest.mark.parametrize("tag", ["p4", "p6"])
def test_a_zero_difference_squares_to_p(tag):
    """acc == +-q: P = U2 - X + 8 p is k p with 4 <= k <= 8, never the zero word; REDC27 of its square is exactly p (a positive
    multiple of p below 2 p), and that is what the zero test has to see"""
    p, g, f, chA, chB = _field(tag)
    runv(f.sqr27(chA, sl(0), sl(1), sl(2), B_P))
    f.zero_or_p_mask(chA, sl(2), S(80, 2), S(82, 2))
    vals = [(4 + l % 5) * p for l in range(64)]
    vals[7] = 0
    vals[9] = 4 * p + 1
    w = _run(g, [(sl(0), vals)])
    got = _get(w, sl(2))
    assert all(got[l] == p for l in range(64) if l not in (7, 9)) and got[7] == 0 and got[9] not in (0, p)
    assert w.rd_smask(S(80, 2)) == (1 << 64) - 1 - (1 << 9)


@pytest.mark.parametrize("tag", ["p4", "p6"])
def test_zero_or_p(tag):
    p, g, f, chA, chB = _field(tag)
    f.zero_or_p_mask(chA, sl(0), S(80, 2), S(82, 2))
    f.zero_or_p_mask(chB, sl(1), S(84, 2), S(86, 2))
    pl = limbs(p)
    vals, want = [0, p], [1, 1]
    for i in range(NL):                                  # p with one limb changed (limb 0: the filter; the others: the full comparison)
        vals.append(p ^ (1 << (LB * i + i % 7)))
        want.append(0)
    for i in range(1, NL):                               # 0 with one limb set: passes the filter, is not zero
        vals.append(1 << (LB * i))
        want.append(0)
    vals += [pl[0] + (5 << LB), pl[0], (p >> LB) << LB, p + 1, p - 1]      # low limb p_0 but not p; ...; low limb 0 but not 0
    want += [0, 0, 0, 0, 0]
    vals += [0] * (64 - len(vals))
    want += [1] * (64 - len(want))
    quiet = [(7 + l) | ((l * 977) << LB) for l in range(64)]               # no lane passes the filter: the comparison is skipped
    w = _run(g, [(sl(0), vals), (sl(1), quiet)])
    assert w.rd_smask(S(80, 2)) == sum(b << l for l, b in enumerate(want))
    assert w.rd_smask(S(84, 2)) == 0
    assert w.hist["v_xor_b32"] == NL                     # one full comparison ran, not two


def test_bound_checker_refuses_what_does_not_fit():
    for tag in ("p4", "p6"):
        p, g, f, chA, chB = _field(tag)
        with pytest.raises(BoundError, match="column 25"):           # W T + V PPP with lazy W and T on one accumulator
            run(f.dual27(chA, chB, sl(0), sl(1), sl(2), sl(3), sl(4), B_W, B_T, AR, AR, allow_split=False))
        run(f.dual27(chA, chB, sl(0), sl(1), sl(2), sl(3), sl(4), AR, AR, AR, AR, allow_split=False))   # reduced operands fit
        assert f.last_split == []
        with pytest.raises(BoundError, match="doubled"):
            run(f.sqr27(chA, sl(0), sl(1), sl(2), Bound(10)))
        run(f.sqr27(chA, sl(0), sl(1), sl(2), B_P))
        with pytest.raises(BoundError, match="negative"):            # X up to 5 p against 4 p
            run(f.lazy_diff(chA, sl(0), [(sl(1), 1)], 2, sl(0), AR, [B_X]))
        with pytest.raises(BoundError, match="2\\^32"):              # a top limb beyond 32 bits
            run(f.mul27(chA, sl(0), sl(1), sl(2), Bound(19), AR))
        with pytest.raises(BoundError, match="column"):              # two 9 p operands: a plain product's columns overflow
            run(f.mul27(chA, sl(0), sl(1), sl(2), Bound(18), Bound(18)))
        # the issue's three widest single products, and the kernel's own ranges (building it runs the checker over all of them)
        run(f.mul27(chA, sl(0), sl(1), sl(2), B_P, AR))
        run(f.mul27(chA, sl(0), sl(1), sl(2), B_X, AR))
    for persistent in (False, True):
        for tag in ("p4", "p6"):
            p = pyref.FIELDS[tag].p
            k = g1_xyzz.build("k", p, R % p, persistent=persistent)
            assert k.max_v == 256 and k.max_a < 0 and k.max_s <= 102
            assert k.lds_bytes == (19968 if persistent else 4 * 19968)
            c = g1_xyzz.update_counts(k)
            assert c["update_mads"] == 6 * 1378 + 2 * 1053 + 2054 + 2                 # 6 products, 2 squares, 1 dual, 2 address mads
            assert c["update_valu"] < 14400


# ------------------------------------------------------------------ the whole kernel, both launch forms
SPECIAL = [
    [],                                              # empty list -> infinity
    [(5, 0)],
    [(5, 0), (5, 0)],                                # P + P: the detour through a salt point
    [(5, 0), (5, 1)],                                # P - P -> infinity
    [(5, 0), (5, 1), (7, 0)],                        # ... and a restart from infinity
    [(0, 0), (0, 0)],                                # G + G: the salt must be 2G
    [(1, 0), (1, 0), (3, 1)],                        # 2G + 2G: the salt must be G
    [(4, 1), (4, 1), (4, 1)],
    [(6, 0), (7, 0), (6, 1), (7, 1), (9, 0)],        # cancels after four entries
]
N_PTS = 32
_ST = {}


def _state(cname):
    if cname in _ST:
        return _ST[cname]
    C = pyref.CURVES[cname]
    p = C.F.p
    rnd = random.Random(41 + len(cname))
    h = C.mul(rnd.randrange(1, 1 << 60), C.G)
    pts = [C.G, C.add(C.G, C.G)]
    pt = C.mul(rnd.randrange(1, 1 << 60), C.G)
    while len(pts) < N_PTS:
        pts.append(pt)
        pt = C.add(pt, h)
    s3 = C.add(C.add(pts[10], pts[11]), C.neg(pts[12]))              # a running sum of three entries, as a table row
    pts.append(s3)
    lists = list(SPECIAL)
    lists.append([(rnd.randrange(N_PTS), rnd.randrange(2)) for _ in range(60)])      # the lazy ranges over a long chain
    lists.append([(10, 0), (11, 0), (12, 1), (N_PTS, 0)])            # acc == q after three updates: the detour
    lists.append([(10, 0), (11, 0), (12, 1), (N_PTS, 1)])            # acc == -q: infinity
    lists.append([(10, 0), (11, 0), (12, 1), (N_PTS, 1), (13, 1)])   # ... and a restart
    lists.append([(10, 1), (11, 1), (12, 0), (N_PTS, 1), (N_PTS, 1)])    # -acc == -q: the detour on negated entries, then once more
    while len(lists) < 64 + 3:                                       # a second, ragged tile / wave
        lists.append([(rnd.randrange(N_PTS + 1), rnd.randrange(2)) for _ in range(rnd.randrange(1, 4))])
    expect = []
    for l in lists:
        e = None
        for (i, s) in l:
            e = C.add(e, C.neg(pts[i]) if s else pts[i])
        expect.append(e)
    st = dict(C=C, p=p, pts=pts, lists=lists, expect=expect,
              pw=g1_xyzz.build("acc_pw_" + cname, p, R % p, persistent=True),
              blk=g1_xyzz.build("acc_" + cname, p, R % p))
    _ST[cname] = st
    return st


@pytest.mark.parametrize("cname", TP.CURVES)
def test_kernel_against_the_group_law_in_both_forms(cname):
    st = _state(cname)
    nt = len(st["lists"])
    assert st["expect"][3] is None and st["expect"][len(SPECIAL) + 2] is None and st["expect"][len(SPECIAL) + 1] is not None
    block = TP._launch_block(st, nt)
    TP._check_law(st, block, nt)                                     # the affine law, every word below p, (0, 1, 0) for infinity
    mem, a_karg = TP._memory(st, nt)
    TP._launch_pw(st, mem, a_karg, 2)
    out = mem.get("out").reshape(nt, 78)
    TP._check_law(st, out, nt)
    assert np.array_equal(out, block)
