"""One fixed, seeded sequence through every branch of the MSM's launch sequence (csrc/msm_impl.h), every result checked against
the closed form of a chain key or textbook multiples, for comparing the kernel dispatches of two trees
(profiles/msm_launch_parity.md):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/msm_dispatch_sequence.py TREE
    python tools/msm_dispatch_sequence.py --compare A_kernel_trace.csv B_kernel_trace.csv

TREE is the repository root whose built library is loaded.  --compare groups each trace by kernel name and compares, per name,
the sorted list of (grid size, workgroup size, LDS bytes, scratch bytes); exit status 1 if anything differs."""
import csv
import os
import sys
import time


def trace_shapes(path):
    shapes = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            def dims(prefix):
                return tuple(int(row[k]) for k in (prefix + "_X", prefix + "_Y", prefix + "_Z") if k in row) or (int(row[prefix]),)
            lds = int(row.get("LDS_Block_Size", row.get("LDS_Block_Size_v", 0)) or 0)
            scratch = int(row.get("Scratch_Size", row.get("Private_Segment_Size", 0)) or 0)
            shapes.setdefault(row["Kernel_Name"], []).append((dims("Grid_Size"), dims("Workgroup_Size"), lds, scratch))
    return {k: sorted(v) for k, v in shapes.items()}


def compare(a_path, b_path):
    a, b = trace_shapes(a_path), trace_shapes(b_path)
    bad = 0
    for name in sorted(set(a) | set(b)):
        la, lb = a.get(name, []), b.get(name, [])
        if la != lb:
            bad += 1
            only_a = [s for s in la if s not in lb][:3]
            only_b = [s for s in lb if s not in la][:3]
            print("DIFFERENT %s: %d dispatches against %d; first shapes only in A %s, only in B %s" % (name, len(la), len(lb), only_a, only_b))
    print("%d kernel names, %d dispatches in A, %d in B, %d names differ" % (len(set(a) | set(b)), sum(map(len, a.values())),
                                                                             sum(map(len, b.values())), bad))
    return 1 if bad else 0


def run(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import numpy as np
    import pyref
    import support as S
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    t_start = time.perf_counter()

    def chain(curve, n, seed):
        C = pyref.CURVES[curve]
        rng = pyref.Rng(seed)
        P0, H = C.mul(rng.next_u64() | 1, C.G), C.mul(rng.next_u64() | 1, C.G)
        xy, _ = S.bases_array(C, [P0, H])
        return gl.ResidentBases.chain(curve, xy[0], xy[1], n), P0, H

    def check(name, curve, xyz, want):
        got = S.affine_of_xyz(pyref.CURVES[curve], xyz)
        if got != want:
            raise SystemExit("WRONG RESULT: " + name)
        tm = gl.msm_last_timing()
        print("ok  %-62s c %2d  windows %2d" % (name, tm["window_bits"], tm["num_windows"]), flush=True)

    g1 = "mnt4753_g1"
    C = pyref.CURVES[g1]
    n = 1 << 20
    check("empty MSM", g1, gl.VariableBaseMSM.multi_scalar_mul(g1, np.zeros((0, 24), np.uint64), np.zeros((0, 12), np.uint64)), None)
    rb, P0, H = chain(g1, n, 1020)
    s = S.random_scalars_np(n, seed=620, below=C.order)
    s[5] = 0
    s[7] = np.array(pyref.int_to_limbs(C.order - 1), dtype=np.uint64)
    want = S.chain_msm_closed_form(C, P0, H, s)
    m = 1 << 12
    check("G1 2^12 from host buffers (atomic sort, per-window)", g1, gl.VariableBaseMSM.multi_scalar_mul(g1, rb.download(0, m), s[:m]),
          S.chain_msm_closed_form(C, P0, H, s[:m]))
    ds = gl.DeviceBuffer(s.nbytes).upload(s)
    check("G1 2^20 chain key, no table", g1, rb.msm_dev(ds, n), want)
    rb.precompute(0)
    check("G1 2^20 chain key, full table, one MSM alone", g1, rb.msm_dev(ds, n), want)
    short = n - 12345
    want_short = S.chain_msm_closed_form(C, P0, H, s[:short])
    outs = gl.msm_batch_dev([(rb, ds, n), (rb, ds, short), (rb, ds, n), (rb, ds, n)])
    for k, (o, w) in enumerate(zip(outs, (want, want_short, want, want))):
        check("G1 2^20 batch of four, MSM %d (lean for the first three)" % k, g1, o, w)
    rb.precompute(0, 8)
    check("G1 2^20 chain key, precompute(max_rows=8)", g1, rb.msm_dev(ds, n), want)
    gl.msm_set_affine(1)
    check("G1 2^18 with msm_set_affine(1)", g1, rb.msm_dev(ds, 1 << 18), S.chain_msm_closed_form(C, P0, H, s[:1 << 18]))
    gl.msm_set_affine(2)
    # a key with repeated bases (every base twice): the table build finds the groups, the merge kernels add their scalars up
    half = 1 << 14
    dup = np.repeat(rb.download(0, half), 2, axis=0)
    rb.free()
    rd = gl.ResidentBases(g1, dup)
    rd.precompute(0)
    sums = [S.chain_sums(s[par:2 * half:2], C.order) for par in (0, 1)]
    a, b = (sums[0][0] + sums[1][0]) % C.order, (sums[0][1] + sums[1][1]) % C.order
    check("G1 2^15 key of repeated bases (merge kernels)", g1, rd.msm_dev(ds, 2 * half), C.add(C.mul(a, P0), C.mul(b, H)))
    rd.free()
    ds.free()
    gl.dev_trim()
    for curve, log_n in (("mnt4753_g2", 20), ("mnt6753_g2", 19)):
        C2 = pyref.CURVES[curve]
        n2 = 1 << log_n
        rb2, Q0, H2 = chain(curve, n2, 1000 + log_n)
        s2 = S.random_scalars_np(n2, seed=600 + log_n, below=C2.order)
        d2 = gl.DeviceBuffer(s2.nbytes).upload(s2)
        rb2.precompute(0)
        check("%s 2^%d with a table (rounds, split halves)" % (curve, log_n), curve, rb2.msm_dev(d2, n2), S.chain_msm_closed_form(C2, Q0, H2, s2))
        d2.free()
        rb2.free()
        gl.dev_trim()
    for curve in (g1, "mnt4753_g2"):
        Cf = pyref.CURVES[curve]
        rng = pyref.Rng(77)
        base = Cf.mul(rng.next_u64() | 1, Cf.G)
        ks = S.random_scalars_np(1 << 16, seed=41, below=Cf.order)
        fb = gl.FixedBaseMSM(curve, S.proj_array(Cf, base), 753, num_scalars=1 << 16)
        out = fb.multi_scalar_mul(ks)
        fb.free()
        for i in (0, 1, 4097, (1 << 16) - 1):
            if S.affine_of_xyz(Cf, out[i]) != Cf.mul(S.to_int(ks[i]), base):
                raise SystemExit("WRONG RESULT: FixedBaseMSM %s scalar %d" % (curve, i))
        print("ok  FixedBaseMSM 2^16 scalars on %s (accumulate_lists)" % curve, flush=True)
    print("sequence done in %.1f s" % (time.perf_counter() - t_start), flush=True)
    gl.shutdown()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    run(os.path.abspath(sys.argv[1]))
