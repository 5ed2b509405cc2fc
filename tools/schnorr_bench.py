#!/usr/bin/env python3
"""Field-based Schnorr on the device: verifications/s and signatures/s at 2^16 and 2^20 rows (L = 1) for both schemes, the
phase split of every call, and the gh_batch_mul kernel's products per row (counted from the window and the formulas as
written) over its kernel time as a fraction of the product peak gh_measure_fpmul_peak measures in the same run.
Prints one JSON document.  Usage: timeout -k 10 900 python tools/schnorr_bench.py [--log2n 16 20] [--reps 2] > out.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARAMS = os.path.join(ROOT, "tests", "golden", "poseidon_params.json")
SCHEMES = {"SchnorrMNT4": ("mnt4753", "mnt6753_g1"), "SchnorrMNT6": ("mnt6753", "mnt4753_g1")}   # (Poseidon tag, group)
TOP = 0x1c4c62d92c411     # the top u64 limb of both 753-bit primes: random limbs with a smaller top limb are below either
DBL, MADD, ADD = 11, 11, 14   # products of proj_dbl (dbl-2007-bl), proj_madd (madd-1998-cmo), proj_add (add-1998-cmo-2) in ec29.h
INV = 40                      # one safegcd inversion (fp_inv), as tools/poseidon_bench.py counts it


def vb_products_per_row(w, bits=753):
    """the kernels as written: table (2 from_abi, one doubling, 2^(w-1) - 1 additions, Montgomery trick 3 per entry + the
    inversion, 2 per entry for x, y), then w (m - 1) doublings, m - 1 mixed additions and on average half a correction"""
    m = -(-bits // w)
    e = 1 << (w - 1)
    table = 2 + DBL + (e - 1) * ADD + e * 1 + INV + e * 4
    main = w * (m - 1) * DBL + (m - 1) * MADD + 0.5 * MADD
    return table + main


def _rand(rs, n, top):
    a = rs.integers(0, 1 << 63, size=(n, 12), dtype=np.uint64) * 2 + rs.integers(0, 2, size=(n, 12), dtype=np.uint64)
    a[:, 11] = a[:, 11] % np.uint64(top)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    from ginger_lib_amd import poseidon, schnorr
    peak = gl.measure_fpmul_peak()
    # the library runs GH_SCHNORR_WINDOW when it is 4, 5 or 6 and its default, 4, otherwise: refuse what it would not run, so
    # that the window recorded (and the products counted from it) is the one that ran
    env = os.environ.get("GH_SCHNORR_WINDOW")
    if env is not None and env not in ("4", "5", "6"):
        sys.exit("GH_SCHNORR_WINDOW=%s: the library runs only 4, 5 or 6" % env)
    w = int(env or 4)
    doc = {"device": gl.device_name(), "fpmul_peak_per_s": peak, "window": w, "schemes": {}}
    prod = vb_products_per_row(w)
    doc["batch_mul_products_per_row"] = prod
    for name, (tag, curve) in SCHEMES.items():
        prm = poseidon.PoseidonParameters.from_json(PARAMS, tag)
        S = schnorr.FieldBasedSchnorrSignatureScheme(prm, curve)
        res = {}
        rs = np.random.default_rng(1)
        for lg in a.log2n:
            n = 1 << lg
            sk = _rand(rs, n, TOP)
            msg = _rand(rs, n, TOP).reshape(n, 1, 12)
            t0 = time.perf_counter()
            pk = S.get_public_key(sk)
            t_pk = time.perf_counter() - t0
            sig = np.zeros((n, 24), dtype=np.uint64)
            todo = np.arange(n)
            sign_s, sign_rows, sign_phases = [], 0, None
            for _ in range(64):                    # about 57 % of the nonces pass both range checks
                if not len(todo):
                    break
                k = _rand(rs, len(todo), TOP)
                t0 = time.perf_counter()
                s_, st = S.sign(sk[todo], (pk[0][todo], pk[1][todo]), msg[todo], k)
                dt = time.perf_counter() - t0
                if len(todo) == n:
                    sign_s.append(dt)
                    sign_phases = schnorr.last_timing()
                    sign_rows = int(st.sum())
                sig[todo[st == 1]] = s_[st == 1]
                todo = todo[st != 1]
            ver_s, ver_phases = [], None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                st = S.verify(pk, msg, sig)
                ver_s.append(time.perf_counter() - t0)
                ver_phases = schnorr.last_timing()
            assert (st == 1).all(), "a device signature did not verify"
            # the variable-base kernels alone
            k = _rand(rs, n, TOP)
            k[:, 11] &= np.uint64((1 << 49) - 1)
            bm = []
            for _ in range(a.reps):
                schnorr.batch_mul(curve, pk[0], k, pk[1])
                bm.append(schnorr.last_timing()[0]["variable_base"])
            best = min(bm) / 1e3
            res[str(lg)] = {
                "rows": n,
                "verify_s": min(ver_s), "verifications_per_s": n / min(ver_s), "verify_phases_ms": ver_phases[0],
                "verify_total_ms": ver_phases[1],
                "sign_s": min(sign_s), "signatures_per_s": sign_rows / min(sign_s), "sign_accepted": sign_rows,
                "sign_phases_ms": sign_phases[0], "public_keys_s": t_pk, "public_keys_per_s": n / t_pk,
                "batch_mul_kernel_s": best, "batch_mul_per_s": n / best,
                "batch_mul_fraction_of_peak": prod * n / best / peak,
            }
            print("%s 2^%d: %.0f verifications/s, %.0f signatures/s, batch_mul %.3f of peak" % (
                name, lg, n / min(ver_s), sign_rows / min(sign_s), prod * n / best / peak), file=sys.stderr, flush=True)
        doc["schemes"][name] = res
        S.close()
        prm.close()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
