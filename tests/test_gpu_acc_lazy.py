"""The lazy G1 bucket update (asmgen/g1_xyzz.py: 27-digit reductions, no conditional subtraction inside the update) on the card,
both G1 curves.  The knobs are read once per process, so every configuration is a child process (tests/msm_knob_child.py, profile
`lazy`), as in tests/test_gpu_acc_persist.py.  Every sum is compared, as an affine point, with an independent expectation AND with the same
call under GH_ACC_ASM=0 (msm_accumulate_xyzz_kernel, which keeps the fully reduced update):

(a) dense: 2^14 pairs on a chain key with a shift table at c = 14, against the closed form (tests/support.py chain_msm_closed_form);
(b) sparse: 100 pairs without a table against the oracle (189 windows of 9 buckets = 1701 tasks: the last tile is ragged);
(c) long lists: 2^13 pairs without a table whose scalars take 64 values, so a bucket's list holds hundreds of entries and the lazy
    ranges are held over a long chain, against the closed form;
(d) a key with repeated and negated bases under equal scalars (P + P and P - P inside buckets), against the oracle;
(e) a batch of three on alternating streams equals the one-by-one results.
"""
import numpy as np
import pytest

import msm_knob_child as K
from msm_knob_child import CURVES, LONG_VALUES

pytestmark = pytest.mark.gpu
KNOBS = ("GH_ACC_PERSIST", "GH_ACC_WAVES", "GH_ACC_TILES", "GH_ACC_ALT", "GH_ACC_ASM", "GH_ACC_STAMPS", "GH_ASM_HSACO")
_expect = K.expect


def _in(curve):
    return K.inputs("lazy", curve)


def _run(curve, **env_extra):
    return K.run("lazy", curve, "dense,batch,long,sparse,dup", clear=KNOBS, **env_extra)[0]


def _lazy(curve):
    return _run(curve, GH_ACC_ALT="1")


def _reduced(curve):
    return _run(curve, GH_ACC_ASM="0")


@pytest.mark.parametrize("curve", CURVES)
def test_dense_tiles_with_a_table_match_the_closed_form(gpu, curve):
    import support as S
    I = _in(curve)
    res = _lazy(curve)
    assert res["dense"] == _expect(curve, S.chain_msm_closed_form(I["C"], I["P0"], I["H"], I["s"]))
    assert res["dense"] == _reduced(curve)["dense"]


@pytest.mark.parametrize("curve", CURVES)
def test_sparse_lists_with_a_ragged_last_tile_match_the_oracle(gpu, curve):
    import support as S
    I = _in(curve)
    res = _lazy(curve)
    exp = S.oracle_affine(curve, S.oracle_msm(curve, I["sb"], None, I["ss"], 16))
    assert res["sparse"] == [int(exp[1]), exp[0].tobytes().hex()]
    assert res["sparse"] == _reduced(curve)["sparse"]


@pytest.mark.parametrize("curve", CURVES)
def test_lists_of_hundreds_of_entries_match_the_closed_form(gpu, curve):
    import support as S
    I = _in(curve)
    res = _lazy(curve)
    assert len(np.unique(I["sl"], axis=0)) == LONG_VALUES
    assert res["long"] == _expect(curve, S.chain_msm_closed_form(I["C"], I["P0"], I["H"], I["sl"]))
    assert res["long"] == _reduced(curve)["long"]


@pytest.mark.parametrize("curve", CURVES)
def test_repeated_and_negated_bases_inside_buckets_match_the_oracle(gpu, curve):
    import support as S
    I = _in(curve)
    res = _lazy(curve)
    exp = S.oracle_affine(curve, S.oracle_msm(curve, I["db"], None, I["ds"], 16))
    assert res["dup"] == [int(exp[1]), exp[0].tobytes().hex()]
    assert res["dup"] == _reduced(curve)["dup"]


@pytest.mark.parametrize("curve", CURVES)
def test_batch_of_three_on_alternating_streams_equals_one_by_one(gpu, curve):
    res = _lazy(curve)
    assert res["batch"] == [res["dense"], res["single_t"], res["dense"]]
    assert res["single_t"] != res["dense"]
    assert res["batch"] == _reduced(curve)["batch"]
