#!/usr/bin/env python3
"""The polynomial unit on the device (include/ginger_hip_poly.h) over MNT4-753 Fr: evaluate at 2^24 coefficients for k = 1 and
k = 8 points, divide_by_linear at 2^24, divide_by_vanishing at n = 2^24 and N = 2^23, Mul at 2^23 x 2^23 (domain 2^24) and the
division of 2^24 evaluations.

Method: a warm-up call, then windows of at least 20 calls and at least 0.5 s; a window is timed by the device events of
gh_poly_last_timing summed over its calls and by the wall clock around them (every entry point waits for its stream before it
returns); three windows per shape, the median is the figure and (max - min) the spread.  Per line: the products and the bytes
counted from the shapes by the functions below, their share of the product peak gh_measure_fpmul_peak measures in the same run
and of the HBM bandwidth of the data sheet, and which of the two bounds the line.

Two comparisons in the same run, the two sides alternating window by window, by the wall clock of both sides:
  Mul against its parts through the existing entry points (two gh_fft_dev, gh_vec_mul_dev, an inverse gh_fft_dev);
  evaluate at k = 8 against eight calls at k = 1.
Writes profiles/poly_bench.json and prints it.  Usage: timeout -k 10 900 python tools/poly_bench.py [--log2n 24]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELD = "mnt4753_fr"
HBM_BYTES_PER_S = 8.0e12          # MI355X data sheet: 8 TB/s
RUN_LEN, FOLD_GROUP = 32, 4


def fold_counts(n, k):
    """(products, bytes) of evaluate: every level folds n_l coefficients into ceil(n_l / 32) sums, one product per coefficient
    but a lane's first; level 0 reads the rows once per group of four points"""
    prod, byts, first = 0, 0, True
    while n > RUN_LEN:
        g = -(-n // RUN_LEN)
        prod += k * (n - g)
        byts += (96 * n * -(-k // FOLD_GROUP) if first else 104 * n * k) + 104 * g * k
        n, first = g, False
    return prod + k * (n - 1), byts + 104 * n * k


def scan_counts(n):
    """division by x - z: two products per coefficient on every level; the rows are read twice and written once"""
    prod, byts, first = 0, 0, True
    while n > RUN_LEN:
        g = -(-n // RUN_LEN)
        prod += 2 * n
        byts += (288 if first else 312) * n + 208 * g
        n, first = g, False
    return prod + n, byts + 208 * n


def fft_counts(log_n):
    passes = -(-log_n // 8)
    ks = [log_n // passes + (1 if s < log_n % passes else 0) for s in range(passes)]
    return (1 << log_n) * sum(1 + (k - 1) / 2 for k in ks), (1 << log_n) * 192 * passes


def windows(fn, timing, min_calls=20, min_s=0.5, count=3):
    """-> [(device seconds per call, wall seconds per call)] of `count` windows"""
    fn()
    out = []
    for _ in range(count):
        dev = calls = 0
        t0 = time.perf_counter()
        while calls < min_calls or time.perf_counter() - t0 < min_s:
            fn()
            dev += timing() / 1e3
            calls += 1
        out.append((dev / calls, (time.perf_counter() - t0) / calls))
    return out


def figure(ws, idx):
    v = sorted(w[idx] for w in ws)
    return v[len(v) // 2], v[-1] - v[0]


def line(name, ws, products, byts, peak):
    dev, dev_spread = figure(ws, 0)
    wall, wall_spread = figure(ws, 1)
    fp, fb = products / dev / peak, byts / dev / HBM_BYTES_PER_S
    res = {"ms": dev * 1e3, "spread_ms": dev_spread * 1e3, "wall_ms": wall * 1e3, "wall_spread_ms": wall_spread * 1e3, "products": products, "bytes": byts,
           "share_of_product_peak": fp, "share_of_hbm_bandwidth": fb, "nearer_bound": "products" if fp > fb else "bandwidth"}
    print("%-24s %9.3f ms (+- %.3f)  products %.3f of peak, bytes %.3f of HBM" % (name, res["ms"], res["spread_ms"], fp, fb), file=sys.stderr, flush=True)
    return res


def alternate(fa, fb, min_calls=20, min_s=0.5, count=3):
    """wall seconds per call of the two sides, window by window in turn"""
    fa()
    fb()
    res = ([], [])
    for _ in range(count):
        for side, fn in enumerate((fa, fb)):
            calls, t0 = 0, time.perf_counter()
            while calls < min_calls or time.perf_counter() - t0 < min_s:
                fn()
                calls += 1
            res[side].append((time.perf_counter() - t0) / calls)
    return res


def compare(name, a_name, b_name, ta, tb):
    ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    res = {a_name + "_ms": ma * 1e3, b_name + "_ms": mb * 1e3, "larger_spread_ms": spread * 1e3, "difference_ms": (ma - mb) * 1e3,
           "difference_is_real": abs(ma - mb) > 3 * spread}
    print("%s: %s %.3f ms, %s %.3f ms, larger spread %.3f ms" % (name, a_name, ma * 1e3, b_name, mb * 1e3, spread * 1e3), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_bench.json"))
    a = ap.parse_args()
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    from ginger_lib_amd import poly
    lib, f = poly._lib(), gl.FIELDS[FIELD]
    peak = gl.measure_fpmul_peak()
    lg, n = a.log2n, 1 << a.log2n
    rs = np.random.default_rng(7)

    def rows(count):          # canonical rows: below 2^752
        r = rs.integers(0, 1 << 63, size=(count, 12), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        r[:, 11] &= np.uint64(0xFFFF)
        return r

    pts = np.ascontiguousarray(rows(8))
    out = np.zeros((8, 12), dtype=np.uint64)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    d_a = gl.DeviceBuffer(n * 96).upload(rows(n))
    d_b = gl.DeviceBuffer(n * 96)
    d_c = gl.DeviceBuffer(n * 96)
    d_half = gl.DeviceBuffer(n * 48).upload(rows(n // 2))
    size = ctypes.c_size_t()
    doc = {"device": gl.device_name(), "field": FIELD, "fpmul_peak_per_s": peak, "hbm_bytes_per_s": HBM_BYTES_PER_S, "log2n": lg, "lines": {}}
    L = doc["lines"]
    ok = lambda rc: gl._check(rc)
    for k in (1, 8):
        L["evaluate_k%d" % k] = line("evaluate k=%d" % k, windows(lambda: ok(lib.gh_poly_evaluate_dev(f, d_a.ptr, n, P(pts), k, P(out))), poly.last_timing),
                                     *fold_counts(n, k), peak)
    L["divide_by_linear"] = line("divide_by_linear", windows(lambda: ok(lib.gh_poly_divide_by_linear_dev(f, d_a.ptr, n, P(pts), d_b.ptr, P(out))), poly.last_timing),
                                 *scan_counts(n), peak)
    L["divide_by_vanishing"] = line("divide_by_vanishing", windows(lambda: ok(lib.gh_poly_divide_by_vanishing_dev(f, d_a.ptr, n, lg - 1, d_b.ptr, d_c.ptr)),
                                                                   poly.last_timing), 0, 192 * n, peak)
    fp, fb = fft_counts(lg)
    mul = lambda: ok(lib.gh_poly_mul_dev(f, d_a.ptr, n // 2, d_half.ptr, n // 2, d_c.ptr, n, ctypes.byref(size)))
    L["mul"] = line("mul", windows(mul, poly.last_timing), 3 * fp + 3 * n, 3 * fb + 96 * n * 2 + 288 * n, peak)
    # the division needs non-zero divisors: d_a's rows are odd.  It divides in place, so the quotient drifts; the time does not depend on it.
    ok(lib.gh_poly_resize_dev(f, d_a.ptr, n, d_c.ptr, n))
    L["evals_div"] = line("evals_div", windows(lambda: ok(lib.gh_evals_div_dev(f, d_c.ptr, d_a.ptr, n, ctypes.byref(size))), poly.last_timing),
                          8 * n, (192 + 496 + 288) * n, peak)
    assert size.value == 0

    def parts():
        ok(lib.gh_poly_resize_dev(f, d_a.ptr, n // 2, d_c.ptr, n))
        ok(lib.gh_poly_resize_dev(f, d_half.ptr, n // 2, d_b.ptr, n))
        ok(gl.load_library().gh_fft_dev(f, d_c.ptr, lg, 0))
        ok(gl.load_library().gh_fft_dev(f, d_b.ptr, lg, 0))
        ok(gl.load_library().gh_vec_mul_dev(f, d_c.ptr, d_b.ptr, n))
        ok(gl.load_library().gh_fft_dev(f, d_c.ptr, lg, gl.FFT_INVERSE))

    def transforms_only():
        ok(gl.load_library().gh_fft_dev(f, d_c.ptr, lg, 0))
        ok(gl.load_library().gh_fft_dev(f, d_b.ptr, lg, 0))
        ok(gl.load_library().gh_vec_mul_dev(f, d_c.ptr, d_b.ptr, n))
        ok(gl.load_library().gh_fft_dev(f, d_c.ptr, lg, gl.FFT_INVERSE))

    doc["mul_against_its_parts"] = compare("mul against its parts", "mul", "parts", *alternate(mul, transforms_only))
    doc["mul_against_its_parts"]["parts"] = "two gh_fft_dev, gh_vec_mul_dev, inverse gh_fft_dev over vectors already padded"
    doc["mul_against_padded_parts"] = compare("mul against its parts and two resizes", "mul", "parts", *alternate(mul, parts))
    one = [np.ascontiguousarray(pts[j:j + 1]) for j in range(8)]

    def eight():
        for j in range(8):
            ok(lib.gh_poly_evaluate_dev(f, d_a.ptr, n, P(one[j]), 1, P(out[j:j + 1])))

    doc["evaluate_k8_against_8_calls"] = compare("evaluate k=8 against eight calls", "grouped", "eight_calls",
                                                 *alternate(lambda: ok(lib.gh_poly_evaluate_dev(f, d_a.ptr, n, P(pts), 8, P(out))), eight))
    txt = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
