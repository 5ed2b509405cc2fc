"""The persistent form of the assembly G1 accumulation (asmgen/g1_xyzz.py persistent=True: gh_asm_acc_g1_p4_pw / _p6_pw, one-wave
workgroups drawing tiles of 64 tasks from a counter) on the card, both G1 curves.  The knobs are read once per process, so every
configuration is a child process of this file (run as a script), as in tests/test_gpu_reduce_asm.py.

(a) dense: 2^14 pairs on a chain key with a shift table at c = 14 -- 8192 merged buckets = 128 full tiles -- under GH_ACC_PERSIST=1
    (one tile per wave unless GH_ACC_TILES says otherwise: 128 waves): the closed form (tests/support.py chain_msm_closed_form) and the bytes of the same call under GH_ACC_PERSIST=0; the same
    with GH_ACC_WAVES=4 (every wave loops over 32 tiles), with GH_ACC_WAVES=100000 (a grid beyond the tiles: capped) and with
    GH_ACC_TILES=3 (a wave ends after three tiles: 43 waves, the last takes two).
(b) sparse: 100 pairs without a table against the oracle: 189 windows of 9 buckets = 1701 tasks, so the last tile is ragged.
(c) a batch of three under GH_ACC_ALT=1 (the accumulations alternate between two streams) equals the one-by-one results.
(d) the same MSM twice in one process: the task kernel's reset re-arms the counter.
(e) the kernel's resources as the loaded code object reports them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, TABLE_C = 14, 14
SPARSE_N = 100
CURVES = ["mnt4753_g1", "mnt6753_g1"]


def _chain_points(curve):
    import pyref
    C = pyref.CURVES[curve]
    rng = pyref.Rng(5200 + len(curve) + (1 if "6" in curve else 0))
    return C, C.mul(rng.next_u64() | 1, C.G), C.mul(rng.next_u64() | 1, C.G)


def _inputs(curve):
    import pyref
    import support as S
    C, P0, H = _chain_points(curve)
    n = 1 << LOG_N
    s = S.random_scalars_np(n, seed=81, below=C.order)
    t = S.random_scalars_np(n, seed=82, below=C.order)
    s[5] = 0
    s[7] = np.array(pyref.int_to_limbs(C.order - 1), dtype=np.uint64)
    pool = S.chain_points(C, SPARSE_N, pyref.Rng(83))
    sb, _ = S.bases_array(C, pool)
    ss = S.random_scalars_np(SPARSE_N, seed=84, below=C.order)
    return C, P0, H, s, t, sb, ss


# ------------------------------------------------------------------------------ the child process
def _child(curve, what):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import support as S
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.load_library()
    gl.init()
    C, P0, H, s, t, sb, ss = _inputs(curve)
    n = 1 << LOG_N

    def aff(xyz):
        xy, inf = gl.proj_to_affine(curve, xyz)
        return [int(inf), xy.tobytes().hex()]
    res = {}
    xy, _ = S.bases_array(C, [P0, H])
    rb = gl.ResidentBases.chain(curve, xy[0], xy[1], n)
    ds, dt = gl.DeviceBuffer(s.nbytes).upload(s), gl.DeviceBuffer(t.nbytes).upload(t)
    try:
        assert rb.precompute(TABLE_C) == TABLE_C
        res["dense"] = aff(rb.msm_dev(ds, n))
        tm = gl.msm_last_timing()
        res["dense_window"] = [int(tm["window_bits"]), int(tm["num_windows"])]
        if "again" in what:
            res["again"] = aff(rb.msm_dev(ds, n))
        if "batch" in what:
            res["single_t"] = aff(rb.msm_dev(dt, n))
            res["batch"] = [aff(o) for o in gl.msm_batch_dev([(rb, ds, n), (rb, dt, n), (rb, ds, n)])]
    finally:
        ds.free(); dt.free()
        rb.free()
    if "sparse" in what:
        rs = gl.ResidentBases(curve, sb)
        try:
            res["sparse"] = aff(rs.msm(ss))
            res["sparse_window"] = int(gl.msm_last_timing()["window_bits"])
        finally:
            rs.free()
    gl.dev_trim()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ------------------------------------------------------------------------------ the tests
pytestmark = pytest.mark.gpu
_RUNS = {}


def _run(curve, what, **env_extra):
    key = (curve, what, tuple(sorted(env_extra.items())))
    if key in _RUNS:
        return _RUNS[key]
    env = dict(os.environ)
    for k in ("GH_ACC_PERSIST", "GH_ACC_WAVES", "GH_ACC_TILES", "GH_ACC_ALT", "GH_ACC_ASM", "GH_ACC_STAMPS", "GH_ASM_HSACO"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), curve, what], env=env, capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    _RUNS[key] = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    return _RUNS[key]


def _main(curve):
    return _run(curve, "dense,again,batch,sparse", GH_ACC_PERSIST="1", GH_ACC_ALT="1")


def _expect(curve, P):
    import pyref
    import support as S
    xy, inf = S.affine_abi_of_point(pyref.CURVES[curve], P)
    return [int(inf), xy.tobytes().hex()]


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
