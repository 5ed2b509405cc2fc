"""Lean level 1 of the G1 bucket reduction through the generated kernel (asmgen/g1_reduce.py, gh_asm_red_g1_p4 / _p6) on the card,
both G1 curves.  The knobs are read once per process, so every configuration is a child process of this file (run as a script):
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
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, TABLE_C = 14, 14
SPARSE_N, SPARSE_C = 100, 9
CURVES = ["mnt4753_g1", "mnt6753_g1"]


def _chain_points(curve):
    import pyref
    C = pyref.CURVES[curve]
    rng = pyref.Rng(4100 + len(curve) + (1 if "6" in curve else 0))
    return C, C.mul(rng.next_u64() | 1, C.G), C.mul(rng.next_u64() | 1, C.G)


def _inputs(curve):
    import pyref
    import support as S
    C, P0, H = _chain_points(curve)
    n = 1 << LOG_N
    s = S.random_scalars_np(n, seed=71, below=C.order)
    t = S.random_scalars_np(n, seed=72, below=C.order)
    s[5] = 0
    s[7] = np.array(pyref.int_to_limbs(C.order - 1), dtype=np.uint64)
    pool = S.chain_points(C, SPARSE_N, pyref.Rng(73))
    sb, _ = S.bases_array(C, pool)
    ss = S.random_scalars_np(SPARSE_N, seed=74, below=C.order)
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

    def mark(name):
        sys.stderr.flush()
        sys.stderr.write("== %s\n" % name)
        sys.stderr.flush()
    res = {}
    xy, _ = S.bases_array(C, [P0, H])
    rb = gl.ResidentBases.chain(curve, xy[0], xy[1], n)
    ds, dt = gl.DeviceBuffer(s.nbytes).upload(s), gl.DeviceBuffer(t.nbytes).upload(t)
    try:
        assert rb.precompute(TABLE_C) == TABLE_C
        mark("dense")
        res["dense"] = aff(rb.msm_dev(ds, n))
        tm = gl.msm_last_timing()
        res["dense_window"] = [int(tm["window_bits"]), int(tm["num_windows"])]
        if "batch" in what:
            mark("single_t")
            res["single_t"] = aff(rb.msm_dev(dt, n))
            mark("batch")
            res["batch"] = [aff(o) for o in gl.msm_batch_dev([(rb, ds, n), (rb, dt, n), (rb, ds, n)])]
    finally:
        ds.free(); dt.free()
        rb.free()
    if "sparse" in what:
        rs = gl.ResidentBases(curve, sb)
        try:
            mark("sparse")
            res["sparse"] = aff(rs.msm(ss))
            res["sparse_window"] = int(gl.msm_last_timing()["window_bits"])
            gl.msm_set_window(SPARSE_C)
            mark("sparse_c9")
            res["sparse_c9"] = aff(rs.msm(ss))
        finally:
            gl.msm_set_window(0)
            rs.free()
    gl.dev_trim()
    sys.stderr.flush()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ------------------------------------------------------------------------------ the tests
pytestmark = pytest.mark.gpu
_RUNS = {}


def _run(curve, what, **env_extra):
    """one child: -> (results, {section: [(programs, redone), ...]})"""
    key = (curve, what, tuple(sorted(env_extra.items())))
    if key in _RUNS:
        return _RUNS[key]
    env = dict(os.environ, GH_REDUCE_LEAN="1", GH_REDUCE_DEBUG="1")
    for k in ("GH_REDUCE_L", "GH_REDUCE_ASM", "GH_REDUCE_WAVES"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), curve, what], env=env, capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    dbg, section = {}, None
    for line in out.stderr.splitlines():
        if line.startswith("== "):
            section = line[3:].strip()
            dbg[section] = []
        elif line.startswith("reduce: programs "):
            w = line.split()
            assert w[3] == "redone", line
            dbg[section].append((int(w[2]), int(w[4])))
    _RUNS[key] = (res, dbg)
    return _RUNS[key]


def _expect(curve, P):
    import pyref
    import support as S
    xy, inf = S.affine_abi_of_point(pyref.CURVES[curve], P)
    return [int(inf), xy.tobytes().hex()]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("L,programs", [(None, 32), (16, 8)])
def test_dense_buckets_through_the_generated_kernel(gpu, curve, L, programs):
    import support as S
    C, P0, H, s, t, sb, ss = _inputs(curve)
    extra = {} if L is None else {"GH_REDUCE_L": str(L)}
    res, dbg = _run(curve, "dense,batch,sparse" if L is None else "dense", **extra)
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
    res, dbg = _run(curve, "dense,batch,sparse")
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
    res, dbg = _run(curve, "dense,batch,sparse")
    assert res["batch"] == [res["dense"], res["single_t"], res["dense"]]
    assert res["single_t"] != res["dense"]
    assert dbg["batch"] == [(32, 0)] * 3 and dbg["single_t"] == [(32, 0)]


def test_generated_reducer_resources(gpu):
    for which in ("g1_red_p4", "g1_red_p6"):
        r = gpu.kernel_resources(which)
        assert r["scratch_bytes_per_lane"] == 0 and 0 < r["registers"] <= 256 and r["lds_bytes"] == 0, (which, r)
