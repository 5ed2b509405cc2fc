"""The persistent form of the assembly G1 accumulation (asmgen/g1_xyzz.py persistent=True: gh_asm_acc_g1_p4_pw / _p6_pw, one-wave
workgroups drawing tiles of 64 tasks from a counter) on the card, both G1 curves.  The knobs are read once per process, so every
configuration is a child process (tests/msm_knob_child.py, profile `persist`), as in tests/test_gpu_reduce_asm.py.

(a) dense: 2^14 pairs on a chain key with a shift table at c = 14 -- 8192 merged buckets = 128 full tiles -- under GH_ACC_PERSIST=1
    (one tile per wave unless GH_ACC_TILES says otherwise: 128 waves): the closed form (tests/support.py chain_msm_closed_form) and the bytes of the same call under GH_ACC_PERSIST=0; the same
    with GH_ACC_WAVES=4 (every wave loops over 32 tiles), with GH_ACC_WAVES=100000 (a grid beyond the tiles: capped) and with
    GH_ACC_TILES=3 (a wave ends after three tiles: 43 waves, the last takes two).
(b) sparse: 100 pairs without a table against the oracle: 189 windows of 9 buckets = 1701 tasks, so the last tile is ragged.
(c) a batch of three under GH_ACC_ALT=1 (the accumulations alternate between two streams) equals the one-by-one results.
(d) the same MSM twice in one process: the task kernel's reset re-arms the counter.
(e) the kernel's resources as the loaded code object reports them.
"""
import pytest

import msm_knob_child as K
from msm_knob_child import CURVES, TABLE_C

pytestmark = pytest.mark.gpu
KNOBS = ("GH_ACC_PERSIST", "GH_ACC_WAVES", "GH_ACC_TILES", "GH_ACC_ALT", "GH_ACC_ASM", "GH_ACC_STAMPS", "GH_ASM_HSACO")
_expect = K.expect


def _inputs(curve):
    I = K.inputs("persist", curve)
    return [I[k] for k in ("C", "P0", "H", "s", "t", "sb", "ss")]


def _run(curve, what, **env_extra):
    return K.run("persist", curve, what, clear=KNOBS, **env_extra)[0]


def _main(curve):
    return _run(curve, "dense,again,batch,sparse", GH_ACC_PERSIST="1", GH_ACC_ALT="1")


@pytest.mark.parametrize("curve", CURVES)
def test_dense_tiles_match_the_closed_form_and_the_block_kernel(gpu, curve):
    import support as S
    C, P0, H, s, t, sb, ss = _inputs(curve)
    res = _main(curve)
    assert res["dense_window"] == [TABLE_C, 752 // TABLE_C + 1]
    assert res["dense"] == _expect(curve, S.chain_msm_closed_form(C, P0, H, s))
    off = _run(curve, "dense,sparse", GH_ACC_PERSIST="0")
    assert res["dense"] == off["dense"]
    assert res["again"] == res["dense"]                             # second launch over the same counter: re-armed by the task kernel


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("waves", [4, 100000])
def test_any_grid_gives_the_same_buckets(gpu, curve, waves):
    """4 waves: each loops over 32 of the 128 tiles; 100000: a grid beyond the tiles is capped at one wave per tile"""
    res = _run(curve, "dense", GH_ACC_PERSIST="1", GH_ACC_WAVES=str(waves))
    assert res["dense"] == _main(curve)["dense"]


@pytest.mark.parametrize("curve", CURVES)
def test_a_tile_budget_gives_the_same_buckets(gpu, curve):
    """GH_ACC_TILES=3: 128 tiles go to 43 waves that end after three tiles each (the last after two)"""
    res = _run(curve, "dense", GH_ACC_PERSIST="1", GH_ACC_TILES="3")
    assert res["dense"] == _main(curve)["dense"]


@pytest.mark.parametrize("curve", CURVES)
def test_sparse_lists_with_a_ragged_last_tile(gpu, curve):
    import support as S
    C, P0, H, s, t, sb, ss = _inputs(curve)
    res = _main(curve)
    exp = S.oracle_affine(curve, S.oracle_msm(curve, sb, None, ss, 16))
    assert res["sparse"] == [int(exp[1]), exp[0].tobytes().hex()]
    assert res["sparse_window"] == 4                                # 189 windows x 9 buckets = 1701 tasks = 26 tiles + 37 tasks
    assert res["sparse"] == _run(curve, "dense,sparse", GH_ACC_PERSIST="0")["sparse"]


@pytest.mark.parametrize("curve", CURVES)
def test_batch_of_three_on_alternating_streams_equals_one_by_one(gpu, curve):
    res = _main(curve)
    assert res["batch"] == [res["dense"], res["single_t"], res["dense"]]
    assert res["single_t"] != res["dense"]


def test_persistent_kernel_resources(gpu):
    for which in ("g1_acc_p4_pw", "g1_acc_p6_pw"):
        r = gpu.kernel_resources(which)
        assert r["scratch_bytes_per_lane"] == 0 and 0 < r["registers"] <= 256 and r["lds_bytes"] == 19968, (which, r)
