"""The lazy G1 bucket arithmetic of ginger-lib_amd/csrc/fp29.h and ec29.h (fp_mul27, fp_sqr27, fp_mul2s27, fp_lazy_sub, fp_lazy_x3,
fp_is_zero_or_p, xyzz_madd_lazy with its init and exit conversions) compiled for the host with g++
(tests/host_shim/fp29_lazy_shim.cpp), as tests/test_fp29_host.py builds its harness:
* against Python integers (random operands and operands with every limb at its bound);
* limb for limb against the generated assembly (asmgen/field.py) run in the simulator on the same inputs, and word for word
  against the whole generated kernel on a task list;
* the same source as a stand-alone program under -fsanitize=address,undefined must run clean.
"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ginger-lib_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyref                                                      # noqa: E402
import shim_build                                                 # noqa: E402
import test_asmgen_acc_persist as TP                              # noqa: E402
import test_asmgen_lazy as TL                                     # noqa: E402  (its operand sets and simulator harness)
from asmgen import g1_xyzz                                        # noqa: E402
from asmgen.field import LB, LM, NL, limbs, runv, unlimbs         # noqa: E402

SAN = os.path.join(ROOT, "build", "fp29_lazy_san")
U = ctypes.c_uint32
R, RD, EPS = TL.R, TL.RD, TL.EPS
FIELDS = [(4, "p4", "mnt4753_g1"), (6, "p6", "mnt6753_g1")]


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("fp29_lazy")
    lib.t_lazy_split.restype = ctypes.c_uint64
    return lib


def _w(x):
    """26 raw limbs, the top one wide"""
    assert x >> (LB * (NL - 1) + 32) == 0
    return (U * NL)(*[(x >> (LB * i)) & (LM if i < NL - 1 else 0xFFFFFFFF) for i in range(NL)])


def _op(shim, fid, op, a=0, b=0, c=0, d=0):
    out = (U * NL)()
    shim.t_lazy_op(fid, op, _w(a), _w(b), _w(c), _w(d), out)
    return [int(v) for v in out]


@pytest.mark.parametrize("fid,tag,curve", FIELDS)
def test_lazy_functions_against_integers_and_the_simulator(shim, fid, tag, curve):
    p = pyref.FIELDS[tag].p
    inv = pow(RD, -1, p)
    rnd = random.Random(60 + fid)
    # the same programs and operand sets as tests/test_asmgen_lazy.py: lane l of the simulator against call l of the C++
    pp, g, f, chA, chB = TL._field(tag)
    a, b = TL._operands(p, TL.B_P, rnd), TL._operands(p, TL.AR, rnd)
    w3, t7 = TL._operands(p, TL.B_W, rnd), TL._operands(p, TL.B_T, rnd)
    c, d = TL._operands(p, TL.AR, rnd), TL._operands(p, TL.AR, rnd)
    x5 = TL._operands(p, TL.B_X, rnd)
    x5[0] = 5 * p + EPS                                             # lazy differences take values, not limb caps
    b[0], c[0], d[0] = p + EPS, p + EPS, p + EPS
    sl = TL.sl
    runv(f.mul27(chA, sl(0), sl(1), sl(7), TL.B_P, TL.AR))                              # -> 7
    runv(f.lazy_diff(chA, sl(1), [(sl(4), 1)], 3, sl(6), TL.AR, [TL.B_X]))             # b - x5 + 8 p -> 6
    runv(f.lazy_diff(chB, sl(1), [(sl(5), 1), (sl(3), 2)], 2, sl(4), TL.AR, [TL.AR, TL.AR]))   # b - c - 2 d + 4 p -> 4
    runv(f.lazy_diff(chA, None, [(sl(5), 1)], 1, sl(1), None, [TL.AR]))                 # 2 p - c -> 1
    w = TL._run(g, [(sl(0), a), (sl(1), b), (sl(3), d), (sl(4), x5), (sl(5), c)])
    sim = {k: [[int(v) for v in w.V[sl(k).idx:sl(k).idx + NL, l]] for l in range(64)] for k in (7, 6, 4, 1)}
    pp, g, f, chA, chB = TL._field(tag)
    runv(f.sqr27(chA, sl(0), sl(1), sl(2), TL.B_P))                                     # -> 2
    runv(f.dual27(chA, chB, sl(3), sl(4), sl(5), sl(6), sl(7), TL.B_W, TL.B_T, TL.AR, TL.AR))   # -> 7
    assert shim.t_lazy_split(fid) == sum(1 << k for k in f.last_split)                  # the columns the generator's checker found
    w = TL._run(g, [(sl(0), a), (sl(3), w3), (sl(4), t7), (sl(5), c), (sl(6), d)])
    sim2 = {k: [[int(v) for v in w.V[sl(k).idx:sl(k).idx + NL, l]] for l in range(64)] for k in (2, 7)}
    for l in range(64):
        r = _op(shim, fid, 0, a[l], b[l])
        assert r == sim[7][l] and unlimbs(r) % p == a[l] * b[l] * inv % p and unlimbs(r) < p + EPS, l
        r = _op(shim, fid, 1, a[l])
        assert r == sim2[2][l] and unlimbs(r) % p == a[l] * a[l] * inv % p and unlimbs(r) < p + EPS, l
        r = _op(shim, fid, 2, w3[l], t7[l], c[l], d[l])
        assert r == sim2[7][l] and unlimbs(r) % p == (w3[l] * t7[l] + c[l] * d[l]) * inv % p and unlimbs(r) < p + EPS, l
        r = _op(shim, fid, 3, b[l], x5[l])
        assert r == sim[6][l] and unlimbs(r) == b[l] - x5[l] + 8 * p and max(r[:NL - 1]) <= LM, l
        r = _op(shim, fid, 5, b[l], c[l], d[l])
        assert r == sim[4][l] and unlimbs(r) == b[l] - c[l] - 2 * d[l] + 4 * p, l
        r = _op(shim, fid, 4, 0, c[l])
        assert r == sim[1][l] and unlimbs(r) == 2 * p - c[l], l
    # p - y keeps p for y = 0; the zero test; the accumulator's one
    for y in (0, 1, p - 1, rnd.randrange(p)):
        assert unlimbs(_op(shim, fid, 6, y)) == p - y
    for v, z in ((0, 1), (p, 1), (p ^ 1, 0), (p ^ (1 << 400), 0), (1 << 290, 0), (limbs(p)[0], 0), (p + 1, 0)):
        assert _op(shim, fid, 7, v)[0] == z, hex(v)
    assert unlimbs(_op(shim, fid, 8)) == (R % p) * (1 << 58) % p


@pytest.mark.parametrize("fid,tag,curve", FIELDS)
def test_lazy_update_against_the_group_law_and_the_generated_kernel(shim, fid, tag, curve):
    """xyzz_madd_lazy over task lists: the affine law, and the very words the generated kernel stores for the same list"""
    st = TL._state(curve)
    C, p, pts = st["C"], st["p"], st["pts"]
    r = R % p
    ri = pow(r, -1, p)
    picks = [1, 3, 4, 8, len(TL.SPECIAL) + 2, len(TL.SPECIAL) + 3, 64, 65, 66]      # no P + P inside (the kernel detours there)
    sub = dict(st, lists=[st["lists"][t] for t in picks], expect=[st["expect"][t] for t in picks])
    kernel = TP._launch_block(sub, len(picks))
    TP._check_law(sub, kernel, len(picks))
    for j, t in enumerate(picks):
        l = st["lists"][t]
        rows = (U * (2 * NL * len(l)))(*[x for (i, s) in l for x in limbs(pts[i][0][0] * r % p) + limbs(pts[i][1][0] * r % p)])
        neg = (ctypes.c_uint8 * len(l))(*[s for (i, s) in l])
        out, state = (U * (3 * NL))(), (U * (4 * NL + 1))()
        assert shim.t_lazy_chain(fid, len(l), rows, neg, out, state) == 0
        assert [int(v) for v in out] == [int(v) for v in kernel[j]], t
        xyz = [unlimbs(out[NL * k:NL * k + NL]) for k in range(3)]
        assert max(xyz) < p
        assert C.proj_to_affine(*[(v * ri % p,) for v in xyz]) == st["expect"][t]
    # the list of 60 entries: the law only (the kernel takes its P + P entries, if any, through a salt)
    l = st["lists"][len(TL.SPECIAL)]
    rows = (U * (2 * NL * len(l)))(*[x for (i, s) in l for x in limbs(pts[i][0][0] * r % p) + limbs(pts[i][1][0] * r % p)])
    neg = (ctypes.c_uint8 * len(l))(*[s for (i, s) in l])
    out, state = (U * (3 * NL))(), (U * (4 * NL + 1))()
    if shim.t_lazy_chain(fid, len(l), rows, neg, out, state) == 0:
        xyz = [unlimbs(out[NL * k:NL * k + NL]) for k in range(3)]
        assert C.proj_to_affine(*[(v * ri % p,) for v in xyz]) == st["expect"][len(TL.SPECIAL)]
    zz = unlimbs(state[2 * NL:3 * NL])
    assert zz < p + EPS and unlimbs(state[0:NL]) < 5 * p + EPS and unlimbs(state[NL:2 * NL]) < p + EPS


def test_the_same_source_runs_clean_under_the_sanitizers():
    """a stand-alone program (its own main) built with -fsanitize=address,undefined: operands at the kernel's bounds and a chain of
    60 updates per prime against the fully reduced xyzz_madd"""
    out = shim_build.sanitized_check("fp29_lazy_shim.cpp", SAN, defines=("FP29_LAZY_MAIN",))
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["mnt4753:", "ok", "mnt6753:", "ok"] and "runtime error" not in out.stderr
