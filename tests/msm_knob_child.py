"""The one child runner of the MSM knob tests (tests/test_gpu_acc_persist.py, test_gpu_acc_lazy.py, test_gpu_reduce_asm.py).  The
GH_* knobs are read once per process, so every configuration is a child process: this module run as a script,

    python tests/msm_knob_child.py <profile> <curve> <sections>

which loads the package, builds the inputs of <profile>, runs the requested sections, writes `== <name>` on stderr before every
MSM call (so that the library's own stderr lines can be told apart) and prints one `RESULT <json>` line.  The sections:

  dense      2^14 pairs on a chain key with a shift table at c = 14 (always run; also gives dense_window)
  again      the same call a second time
  batch      the same key over the scalars t (single_t), then a batch of three: s, t, s
  long       2^13 pairs without a table whose scalars take 64 values
  sparse     100 explicit points without a table (also gives sparse_window)
  sparse_c9  the same 100 pairs at window c = 9
  dup        a key with repeated and negated bases under equal scalars

A profile is the seeds of one test file; a file's inputs are the same arrays in the child and in the test that checks it."""
import functools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, TABLE_C = 14, 14
LONG_LOG_N, LONG_VALUES = 13, 64
SPARSE_N, SPARSE_C = 100, 9
CURVES = ["mnt4753_g1", "mnt6753_g1"]
SECTIONS = ("dense", "again", "batch", "long", "sparse", "sparse_c9", "dup")
# chain: the seed of the chain key's two points; s, t: the dense scalars, with row `zero` = 0 and row `top` = order - 1;
# pool, ss: the sparse points and their scalars; long: the 64 values and the picks among them; dup: the 40 scalars of the dup key
PROFILES = {
    "persist": dict(chain=5200, s=81, t=82, zero=5, top=7, pool=83, ss=84),
    "lazy": dict(chain=7300, s=91, t=92, zero=3, top=9, pool=95, ss=96, long=(93, 94), dup=97),
    "reduce": dict(chain=4100, s=71, t=72, zero=5, top=7, pool=73, ss=74),
}


@functools.lru_cache(maxsize=None)
def inputs(profile, curve):
    """-> dict: C, P0, H (the chain key), s, t, sb, ss, and with the profile's extra seeds sl (long) and db, ds (dup).  Shared by
    every caller in the process: read only."""
    import pyref
    import support as S
    pf = PROFILES[profile]
    C = pyref.CURVES[curve]
    rng = pyref.Rng(pf["chain"] + len(curve) + (1 if "6" in curve else 0))
    I = dict(C=C, P0=C.mul(rng.next_u64() | 1, C.G), H=C.mul(rng.next_u64() | 1, C.G))
    n = 1 << LOG_N
    I["s"] = S.random_scalars_np(n, seed=pf["s"], below=C.order)
    I["t"] = S.random_scalars_np(n, seed=pf["t"], below=C.order)
    I["s"][pf["zero"]] = 0
    I["s"][pf["top"]] = np.array(pyref.int_to_limbs(C.order - 1), dtype=np.uint64)
    if "long" in pf:
        vals = S.random_scalars_np(LONG_VALUES, seed=pf["long"][0], below=C.order)
        I["sl"] = vals[np.random.default_rng(pf["long"][1]).integers(0, LONG_VALUES, size=1 << LONG_LOG_N)]
    pool = S.chain_points(C, SPARSE_N, pyref.Rng(pf["pool"]))
    I["sb"], _ = S.bases_array(C, pool)
    I["ss"] = S.random_scalars_np(SPARSE_N, seed=pf["ss"], below=C.order)
    if "dup" in pf:
        dup = pool[:40] + pool[:20] + [C.neg(P) for P in pool[20:40]]          # 20 bases twice, 20 bases with their negatives
        I["db"], _ = S.bases_array(C, dup)
        d40 = S.random_scalars_np(40, seed=pf["dup"], below=C.order)
        I["ds"] = np.concatenate([d40, d40[:20], d40[20:40]])                   # equal scalars: the pairs meet in every bucket
    return I


def expect(curve, P):
    """a point as the child reports one: [infinity, hex of the affine ABI words]"""
    import pyref
    import support as S
    xy, inf = S.affine_abi_of_point(pyref.CURVES[curve], P)
    return [int(inf), xy.tobytes().hex()]


# ------------------------------------------------------------------------------ the child process
def child(profile, curve, sections):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import support as S
    from __graft_entry__ import _load_pkg
    assert "dense" in sections and not set(sections) - set(SECTIONS), sections
    gl = _load_pkg()
    gl.load_library()
    gl.init()
    I = inputs(profile, curve)
    C, s, t = I["C"], I["s"], I["t"]
    n, nl = 1 << LOG_N, 1 << LONG_LOG_N
    res = {}

    def aff(xyz):
        xy, inf = gl.proj_to_affine(curve, xyz)
        return [int(inf), xy.tobytes().hex()]

    def mark(name):
        sys.stderr.flush()
        sys.stderr.write("== %s\n" % name)
        sys.stderr.flush()

    def explicit(key, bases, scalars, at_c9=False):
        r = gl.ResidentBases(curve, bases)
        try:
            if key in sections:
                mark(key)
                res[key] = aff(r.msm(scalars))
                res[key + "_window"] = int(gl.msm_last_timing()["window_bits"])
            if at_c9:
                try:
                    gl.msm_set_window(SPARSE_C)
                    mark("sparse_c9")
                    res["sparse_c9"] = aff(r.msm(scalars))
                finally:
                    gl.msm_set_window(0)
        finally:
            r.free()

    xy, _ = S.bases_array(C, [I["P0"], I["H"]])
    rb = gl.ResidentBases.chain(curve, xy[0], xy[1], n)
    ds, dt = gl.DeviceBuffer(s.nbytes).upload(s), gl.DeviceBuffer(t.nbytes).upload(t)
    try:
        assert rb.precompute(TABLE_C) == TABLE_C
        mark("dense")
        res["dense"] = aff(rb.msm_dev(ds, n))
        tm = gl.msm_last_timing()
        res["dense_window"] = [int(tm["window_bits"]), int(tm["num_windows"])]
        if "again" in sections:
            mark("again")
            res["again"] = aff(rb.msm_dev(ds, n))
        if "batch" in sections:
            mark("single_t")
            res["single_t"] = aff(rb.msm_dev(dt, n))
            mark("batch")
            res["batch"] = [aff(o) for o in gl.msm_batch_dev([(rb, ds, n), (rb, dt, n), (rb, ds, n)])]
    finally:
        ds.free(); dt.free()
        rb.free()
    if "long" in sections:
        rl = gl.ResidentBases.chain(curve, xy[0], xy[1], nl)
        dl = gl.DeviceBuffer(I["sl"].nbytes).upload(np.ascontiguousarray(I["sl"]))
        try:
            mark("long")
            res["long"] = aff(rl.msm_dev(dl, nl))
        finally:
            dl.free()
            rl.free()
    if "sparse" in sections or "sparse_c9" in sections:
        explicit("sparse", I["sb"], I["ss"], at_c9="sparse_c9" in sections)
    if "dup" in sections:
        explicit("dup", I["db"], I["ds"])
    gl.dev_trim()
    sys.stderr.flush()
    print("RESULT " + json.dumps(res))


# ------------------------------------------------------------------------------ the parent's side
_RUNS = {}
started = 0                     # children so far: a test file's configurations, no more (the cache key holds)


def run(profile, curve, sections, clear=(), base_env=None, **env):
    """one child with the knobs `clear` removed from the environment and base_env, then env, set -> (results, its stderr); run
    once per process for a given configuration"""
    key = (profile, curve, sections, tuple(clear), tuple(sorted((base_env or {}).items())), tuple(sorted(env.items())))
    if key in _RUNS:
        return _RUNS[key]
    e = dict(os.environ)
    for k in clear:
        e.pop(k, None)
    e.update(base_env or {})
    e.update(env)
    global started
    started += 1
    print("msm_knob_child: child %d: %s %s %s %s" % (started, profile, curve, sections, env))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), profile, curve, sections], env=e, capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    _RUNS[key] = (json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]), out.stderr)
    return _RUNS[key]


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2], sys.argv[3].split(","))
