#!/usr/bin/env python3
"""Pedersen hash on the device: rows/s of gh_pedersen_hash_dev over 2^20 rows of 96 bytes (one serialised field element,
generators[128][6]) on both G1 groups at every table_bits, the hash kernel's products per row (the expected count of mixed
additions of random input, by the product count of proj_madd) over its kernel time as a fraction of the product peak
gh_measure_fpmul_peak measures in the same run, and in the same run gh_bh_hash over the same bytes (2.67 mixed additions
per byte against 1 at table_bits 8).  The generators are random points (sk G from a Schnorr handle's public keys): the cost
does not depend on them.
Writes profiles/pedersen_bench.json and prints it.  Usage: timeout -k 10 600 python tools/pedersen_bench.py [--log2n 20] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from schnorr_bench import MADD, TOP, _rand   # noqa: E402

PARAMS = os.path.join(ROOT, "tests", "golden", "poseidon_params.json")
GROUPS = {"mnt6753_g1": "mnt4753", "mnt4753_g1": "mnt6753"}    # group -> the Poseidon tag of its base field (for the key generator)
NUM_WINDOWS, WINDOW_SIZE, NBYTES = 128, 6, 96
BH_WINDOWS, BH_WINDOW_SIZE = 2, 128                              # 256 chunks of 3 bits: the same 96 bytes
TABLE_BITS = (1, 2, 4, 8)


def madds_per_row(t, bits=8 * NBYTES):
    """expected mixed additions of a random row: one per position whose digit is not zero"""
    return (bits // t) * (1.0 - 2.0 ** -t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pedersen_bench.json"))
    a = ap.parse_args()
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    from ginger_lib_amd import ecvrf, pedersen, poseidon, schnorr
    peak = gl.measure_fpmul_peak()
    n = 1 << a.log2n
    doc = {"device": gl.device_name(), "fpmul_peak_per_s": peak, "rows": n, "nbytes": NBYTES, "windows": [NUM_WINDOWS, WINDOW_SIZE],
           "bh_windows": [BH_WINDOWS, BH_WINDOW_SIZE], "products_per_madd": MADD, "groups": {}}
    for curve, tag in GROUPS.items():
        prm = poseidon.PoseidonParameters.from_json(PARAMS, tag)
        S = schnorr.FieldBasedSchnorrSignatureScheme(prm, curve)
        rs = np.random.default_rng(1)
        gxy, ginf = S.get_public_key(_rand(rs, NUM_WINDOWS * WINDOW_SIZE, TOP))
        data = rs.integers(0, 256, size=(n, NBYTES), dtype=np.uint8)
        d_in, d_xy, d_inf = gl.DeviceBuffer(n * NBYTES).upload(data), gl.DeviceBuffer(n * 192), gl.DeviceBuffer(n)
        res = {"table_bits": {}}
        ref_xy = None
        for t in TABLE_BITS:
            D = pedersen.PedersenCRH(curve, gxy, ginf, NUM_WINDOWS, WINDOW_SIZE, t)
            D.evaluate_dev(d_in, n, NBYTES, d_xy, d_inf)          # builds the table
            wall, kern = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                D.evaluate_dev(d_in, n, NBYTES, d_xy, d_inf)
                wall.append(time.perf_counter() - t0)
                kern.append(pedersen.last_timing()[0]["hash"] / 1e3)
            xy = d_xy.download()
            if ref_xy is None:
                ref_xy = xy
            assert np.array_equal(xy, ref_xy), "table_bits %d disagrees with table_bits %d" % (t, TABLE_BITS[0])
            prod = madds_per_row(t) * MADD
            res["table_bits"][str(t)] = {"call_s": min(wall), "rows_per_s": n / min(wall), "hash_kernel_s": min(kern),
                                         "kernel_rows_per_s": n / min(kern), "madds_per_row": madds_per_row(t), "products_per_row": prod,
                                         "fraction_of_peak": prod * n / min(kern) / peak}
            print("%s t=%d: %.2f M rows/s (kernel %.1f ms, %.3f of peak)" % (curve, t, n / min(wall) / 1e6, min(kern) * 1e3,
                                                                              prod * n / min(kern) / peak), file=sys.stderr, flush=True)
            D.close()
        B = ecvrf.BoweHopwoodPedersenCRH(curve, gxy[:BH_WINDOWS * BH_WINDOW_SIZE], ginf[:BH_WINDOWS * BH_WINDOW_SIZE], BH_WINDOWS, BH_WINDOW_SIZE)
        B.evaluate(data[:64])
        wall, kern = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            B.evaluate(data)
            wall.append(time.perf_counter() - t0)
            kern.append(ecvrf.last_timing()[0]["group_hash"] / 1e3)
        prod = 256 * MADD
        res["bowe_hopwood"] = {"call_s_from_host": min(wall), "hash_kernel_s": min(kern), "kernel_rows_per_s": n / min(kern), "madds_per_row": 256,
                               "products_per_row": prod, "fraction_of_peak": prod * n / min(kern) / peak}
        print("%s Bowe-Hopwood: kernel %.1f ms (%.3f of peak)" % (curve, min(kern) * 1e3, prod * n / min(kern) / peak), file=sys.stderr, flush=True)
        res["fastest_table_bits"] = int(min(res["table_bits"], key=lambda k: res["table_bits"][k]["hash_kernel_s"]))
        doc["groups"][curve] = res
        B.close()
        for b in (d_in, d_xy, d_inf):
            b.free()
        S.close()
        prm.close()
    txt = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
