"""Lean level 1 of the G1 bucket reduction through the generated kernel (asmgen/g1_reduce.py, gh_asm_red_g1_p4 / _p6) on the card,
both G1 curves.  The knobs are read once per process, so every configuration is a child process (tests/msm_knob_child.py, profile
`reduce`, which marks every MSM call on stderr):
GH_REDUCE_LEAN=1 forces the lane-level form on every MSM, GH_REDUCE_DEBUG=1 prints `reduce: programs N redone M` per level 1.

(a) dense: 2^14 pairs on a chain key with a shift table at c = 14 -- 8192 merged buckets of about 108 entries -- with the chosen
    L = 4 (32 programs) and with GH_REDUCE_L=16 (8 programs, the production step count): the result equals the closed form
    (tests/support.py chain_msm_closed_form) and the result of the same call under GH_REDUCE_ASM=0, and no program is computed
    again: an empty bucket has probability about e^-108 here, and without an empty bucket or equal points no doubling arises.
(b) sparse: 100 pairs, no table, against the oracle.  At the default window (c = 4: 9 slots per window) a lane never holds two
    items, so level 1 consists of copies only, nothing can double and `redone` is 0 by construction -- checked as such; that the
    fallback runs and repairs is shown on the same 100 pairs at c = 9 (257 slots per window, two thirds of them empty: a lane
    whose first item is followed by an empty one adds run to an equal wacc), where `redone` must be above 0.
(c) a batch of three MSMs of shape (a) equals the one-by-one results.
(d) the kernel's resources as the loaded code object reports them: no scratch, at most 256 registers, no LDS.
"""
import pytest

import msm_knob_child as K
from msm_knob_child import CURVES, SPARSE_C, TABLE_C

pytestmark = pytest.mark.gpu
KNOBS = ("GH_REDUCE_L", "GH_REDUCE_ASM", "GH_REDUCE_WAVES")
ALL = "dense,batch,sparse,sparse_c9"
_expect = K.expect


def _inputs(curve):
    I = K.inputs("reduce", curve)
    return [I[k] for k in ("C", "P0", "H", "s", "t", "sb", "ss")]


def _run(curve, what, **env_extra):
    """one child: -> (results, {section: [(programs, redone), ...]})"""
    res, stderr = K.run("reduce", curve, what, clear=KNOBS, base_env={"GH_REDUCE_LEAN": "1", "GH_REDUCE_DEBUG": "1"}, **env_extra)
    dbg, section = {}, None
    for line in stderr.splitlines():
        if line.startswith("== "):
            section = line[3:].strip()
            dbg[section] = []
        elif line.startswith("reduce: programs "):
            w = line.split()
            assert w[3] == "redone", line
            dbg[section].append((int(w[2]), int(w[4])))
    return res, dbg


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("L,programs", [(None, 32), (16, 8)])
def test_dense_buckets_through_the_generated_kernel(gpu, curve, L, programs):
    import support as S
    C, P0, H, s, t, sb, ss = _inputs(curve)
    extra = {} if L is None else {"GH_REDUCE_L": str(L)}
    res, dbg = _run(curve, ALL if L is None else "dense", **extra)
    assert res["dense_window"] == [TABLE_C, 752 // TABLE_C + 1]
    assert res["dense"] == _expect(curve, S.chain_msm_closed_form(C, P0, H, s))
    off, dbg_off = _run(curve, "dense", GH_REDUCE_ASM="0", **extra)
    assert res["dense"] == off["dense"]
    assert dbg_off["dense"] == []                                   # the C++ kernel alone: nothing to report
    # 8192 merged slots in one window: 8192 / (64 L) programs, and none of them met a doubling
    assert dbg["dense"] == [(programs, 0)]


@pytest.mark.parametrize("curve", CURVES)
def test_sparse_buckets_reach_the_fallback(gpu, curve):
    import support as S
    C, P0, H, s, t, sb, ss = _inputs(curve)
    res, dbg = _run(curve, ALL)
    exp = S.oracle_affine(curve, S.oracle_msm(curve, sb, None, ss, 16))
    exp = [int(exp[1]), exp[0].tobytes().hex()]
    assert res["sparse"] == exp and res["sparse_c9"] == exp
    # default window c = 4: 752 / 4 + 1 = 189 windows of 9 slots, one program each, copies only
    assert res["sparse_window"] == 4 and dbg["sparse"] == [(189, 0)]
    # c = 9: 84 windows of 257 slots in two segments of 256; lanes that hold an item followed by an empty slot double
    (programs, redone), = dbg["sparse_c9"]
    print("sparse c = 9: programs %d redone %d" % (programs, redone))
    assert programs == (752 // SPARSE_C + 1) * 2 and 0 < redone <= programs


@pytest.mark.parametrize("curve", CURVES)
def test_batch_of_three_equals_one_by_one(gpu, curve):
    res, dbg = _run(curve, ALL)
    assert res["batch"] == [res["dense"], res["single_t"], res["dense"]]
    assert res["single_t"] != res["dense"]
    assert dbg["batch"] == [(32, 0)] * 3 and dbg["single_t"] == [(32, 0)]


def test_generated_reducer_resources(gpu):
    for which in ("g1_red_p4", "g1_red_p6"):
        r = gpu.kernel_resources(which)
        assert r["scratch_bytes_per_lane"] == 0 and 0 < r["registers"] <= 256 and r["lds_bytes"] == 0, (which, r)
