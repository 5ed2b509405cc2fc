"""The lazy G1 bucket update (asmgen/g1_xyzz.py: 27-digit reductions, no conditional subtraction inside the update) on the card,
both G1 curves.  The knobs are read once per process, so every configuration is a child process of this file (run as a script),
as in tests/test_gpu_acc_persist.py.  Every sum is compared, as an affine point, with an independent expectation AND with the same
call under GH_ACC_ASM=0 (msm_accumulate_xyzz_kernel, which keeps the fully reduced update):

(a) dense: 2^14 pairs on a chain key with a shift table at c = 14, against the closed form (tests/support.py chain_msm_closed_form);
(b) sparse: 100 pairs without a table against the oracle (189 windows of 9 buckets = 1701 tasks: the last tile is ragged);
(c) long lists: 2^13 pairs without a table whose scalars take 64 values, so a bucket's list holds hundreds of entries and the lazy
    ranges are held over a long chain, against the closed form;
(d) a key with repeated and negated bases under equal scalars (P + P and P - P inside buckets), against the oracle;
(e) a batch of three on alternating streams equals the one-by-one results.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, TABLE_C = 14, 14
LONG_LOG_N, LONG_VALUES = 13, 64
SPARSE_N = 100
CURVES = ["mnt4753_g1", "mnt6753_g1"]


def _chain_points(curve):
    import pyref
    C = pyref.CURVES[curve]
    rng = pyref.Rng(7300 + len(curve) + (1 if "6" in curve else 0))
    return C, C.mul(rng.next_u64() | 1, C.G), C.mul(rng.next_u64() | 1, C.G)


def _inputs(curve):
    import pyref
    import support as S
    C, P0, H = _chain_points(curve)
    n = 1 << LOG_N
    s = S.random_scalars_np(n, seed=91, below=C.order)
    t = S.random_scalars_np(n, seed=92, below=C.order)
    s[3] = 0
    s[9] = np.array(pyref.int_to_limbs(C.order - 1), dtype=np.uint64)
    # (c) 64 scalar values over 2^13 pairs
    vals = S.random_scalars_np(LONG_VALUES, seed=93, below=C.order)
    pick = np.random.default_rng(94).integers(0, LONG_VALUES, size=1 << LONG_LOG_N)
    sl = vals[pick]
    # (b) and (d): explicit keys
    pool = S.chain_points(C, SPARSE_N, pyref.Rng(95))
    sb, _ = S.bases_array(C, pool)
    ss = S.random_scalars_np(SPARSE_N, seed=96, below=C.order)
    dup = pool[:40] + pool[:20] + [C.neg(P) for P in pool[20:40]]          # 20 bases twice, 20 bases with their negatives
    db, _ = S.bases_array(C, dup)
    d40 = S.random_scalars_np(40, seed=97, below=C.order)
    ds = np.concatenate([d40, d40[:20], d40[20:40]])                        # equal scalars: the pairs meet in every bucket
    return dict(C=C, P0=P0, H=H, s=s, t=t, sl=sl, sb=sb, ss=ss, db=db, ds=ds)


# ------------------------------------------------------------------------------ the child process
def _child(curve):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import support as S
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.load_library()
    gl.init()
    I = _inputs(curve)
    C, s, t, sl = I["C"], I["s"], I["t"], I["sl"]
    n, nl = 1 << LOG_N, 1 << LONG_LOG_N

    def aff(xyz):
        xy, inf = gl.proj_to_affine(curve, xyz)
        return [int(inf), xy.tobytes().hex()]
    res = {}
    xy, _ = S.bases_array(C, [I["P0"], I["H"]])
    rb = gl.ResidentBases.chain(curve, xy[0], xy[1], n)
    ds, dt = gl.DeviceBuffer(s.nbytes).upload(s), gl.DeviceBuffer(t.nbytes).upload(t)
    try:
        assert rb.precompute(TABLE_C) == TABLE_C
        res["dense"] = aff(rb.msm_dev(ds, n))
        res["single_t"] = aff(rb.msm_dev(dt, n))
        res["batch"] = [aff(o) for o in gl.msm_batch_dev([(rb, ds, n), (rb, dt, n), (rb, ds, n)])]
    finally:
        ds.free(); dt.free()
        rb.free()
    rl = gl.ResidentBases.chain(curve, xy[0], xy[1], nl)
    dl = gl.DeviceBuffer(sl.nbytes).upload(np.ascontiguousarray(sl))
    try:
        res["long"] = aff(rl.msm_dev(dl, nl))
    finally:
        dl.free()
        rl.free()
    for key, bases, scalars in (("sparse", I["sb"], I["ss"]), ("dup", I["db"], I["ds"])):
        r = gl.ResidentBases(curve, bases)
        try:
            res[key] = aff(r.msm(scalars))
        finally:
            r.free()
    gl.dev_trim()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


# ------------------------------------------------------------------------------ the tests
pytestmark = pytest.mark.gpu
_RUNS = {}
_INPUTS = {}


def _in(curve):
    if curve not in _INPUTS:
        _INPUTS[curve] = _inputs(curve)
    return _INPUTS[curve]


def _run(curve, **env_extra):
    key = (curve, tuple(sorted(env_extra.items())))
    if key in _RUNS:
        return _RUNS[key]
    env = dict(os.environ)
    for k in ("GH_ACC_PERSIST", "GH_ACC_WAVES", "GH_ACC_TILES", "GH_ACC_ALT", "GH_ACC_ASM", "GH_ACC_STAMPS", "GH_ASM_HSACO"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), curve], env=env, capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    _RUNS[key] = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    return _RUNS[key]


def _lazy(curve):
    return _run(curve, GH_ACC_ALT="1")


def _reduced(curve):
    return _run(curve, GH_ACC_ASM="0")


def _expect(curve, P):
    import pyref
    import support as S
    xy, inf = S.affine_abi_of_point(pyref.CURVES[curve], P)
    return [int(inf), xy.tobytes().hex()]


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
