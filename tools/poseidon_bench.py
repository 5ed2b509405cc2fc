#!/usr/bin/env python3
"""Poseidon on the device: hashes/s of 2^20 pairs at every K, products per hash against the card's measured product rate,
the latency of one permutation, and a 2^20-leaf tree's total and per-level times with and without the host tail.
Prints one JSON document.  Usage: timeout 600 python tools/poseidon_bench.py [--log2n 20] [--reps 3] > out.json"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARAMS = os.path.join(ROOT, "tests", "golden", "poseidon_params.json")


def products_per_hash(r_f, r_p, k):
    """products a lane issues per 2-to-1 hash (one permutation) in the kernel as written: per S-box input 3 products of the
    Montgomery trick, per mixed round 3 fp_mul3 (2 products each), one inversion (~40 products, fp29.h) per K states"""
    full, part = 2 * r_f, r_p
    return full * 3 * 3 + part * 3 + (full + part - 1) * 6 + (full + part) * 40.0 / k


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tails", type=int, nargs="*", default=[0, 16, 64, 128, 256, 512, 1024, 4096])
    a = ap.parse_args()
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    from ginger_lib_amd import poseidon as pos
    lib = gl.load_library()
    peak = ctypes.c_double()
    gl._check(lib.gh_measure_fpmul_peak(ctypes.byref(peak)))
    n = 1 << a.log2n
    res = {"device": gl.device_name(), "fpmul_peak_per_s": peak.value, "n_pairs": n, "fields": {}}
    rng = np.random.default_rng(1)
    data = rng.integers(0, 1 << 63, size=(2 * n, 12), dtype=np.uint64)
    data[:, 11] &= (1 << 40) - 1
    d_in, d_out = gl.DeviceBuffer(data.nbytes), gl.DeviceBuffer(n * 96)
    d_in.upload(data)
    for tag in ("mnt4753", "mnt6753"):
        prm = pos.PoseidonParameters.from_json(PARAMS, tag)
        H = pos.PoseidonHash(prm)
        f = {"r_f": prm.r_f, "r_p": prm.r_p, "k": {}}
        for k in (1, 2, 4, 8):
            pos.set_tuning(k, None)
            H.evaluate_dev(d_in, n, 2, d_out)                     # warm-up (slab allocation, code load)
            best = 1e30
            for _ in range(a.reps):
                t0 = time.perf_counter()
                H.evaluate_dev(d_in, n, 2, d_out)
                best = min(best, time.perf_counter() - t0)
            pph = products_per_hash(prm.r_f, prm.r_p, k)
            f["k"][k] = {"ms": best * 1e3, "hashes_per_s": n / best, "products_per_hash_model": pph,
                         "product_rate_frac_of_peak": n / best * pph / peak.value}
        pos.set_tuning(1, None)
        lat = 1e30
        for _ in range(5):
            t0 = time.perf_counter()
            H.evaluate_dev(d_in, 1, 2, d_out)
            lat = min(lat, time.perf_counter() - t0)
        f["one_permutation_latency_ms_k1"] = lat * 1e3
        # K = 1 from registers against K = 1 from the slab (GH_POSEIDON_LAYOUT, read at every launch): latency and rate
        ab = {}
        for layout in ("registers", "slab"):
            if layout == "slab":
                os.environ["GH_POSEIDON_LAYOUT"] = "slab"
            try:
                H.evaluate_dev(d_in, 1, 2, d_out)
                l1 = min(_timed(lambda: H.evaluate_dev(d_in, 1, 2, d_out)) for _ in range(5))
                m = n // 4
                H.evaluate_dev(d_in, m, 2, d_out)
                tm = min(_timed(lambda: H.evaluate_dev(d_in, m, 2, d_out)) for _ in range(a.reps))
            finally:
                os.environ.pop("GH_POSEIDON_LAYOUT", None)
            ab[layout] = {"latency_ms_n1": l1 * 1e3, "hashes_per_s_n%d" % m: m / tm}
        f["k1_layout_ab"] = ab
        pos.set_tuning(0, None)
        leaves = data[:n]
        for label, tail in (("device_only", 0), ("host_tail_default", None)):
            pos.set_tuning(0, tail)
            pos.FieldBasedMerkleHashTree(prm, 21, leaves[:1024])
            t0 = time.perf_counter()
            pos.FieldBasedMerkleHashTree(prm, 24, leaves)
            wall = time.perf_counter() - t0
            lv, tot = pos.last_timing()
            f["tree_2p%d_height24_%s" % (a.log2n, label)] = {"wall_ms": wall * 1e3, "library_total_ms": tot,
                                                             "level_ms_bottom_up_then_padding": lv}
        # host-tail threshold sweep: the whole tree (device levels + host levels + padding) per threshold
        sweep = {}
        for tail in a.tails:
            pos.set_tuning(0, tail)
            times = []
            for _ in range(2):
                pos.FieldBasedMerkleHashTree(prm, 24, leaves)
                times.append(pos.last_timing()[1])
            sweep[tail] = min(times)
        f["tree_2p%d_height24_total_ms_by_host_tail_nodes" % a.log2n] = sweep
        pos.set_tuning(0, None)
        res["fields"][tag] = f
        prm.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
