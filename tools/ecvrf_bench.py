#!/usr/bin/env python3
"""Field-based EC-VRF on the device: proofs/s and proof_to_hash/s at 2^16 and 2^20 rows (L = 1) for both instances, the phase
split of every call, the joint double-scalar kernel's products per row (counted from the window and the formulas as written)
over its kernel time as a fraction of the product peak gh_measure_fpmul_peak measures in the same run, and the joint kernel
against two gh_batch_mul passes on the same rows.  The Bowe-Hopwood generators are random points (sk G from the Schnorr
handle's public keys): the hash's cost does not depend on them.
Prints one JSON document.  Usage: timeout -k 10 900 python tools/ecvrf_bench.py [--log2n 16 20] [--reps 2] > out.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from schnorr_bench import ADD, DBL, INV, MADD, TOP, _rand, vb_products_per_row   # noqa: E402

PARAMS = os.path.join(ROOT, "tests", "golden", "poseidon_params.json")
SCHEMES = {"EcVrfMNT4": ("mnt4753", "mnt6753_g1"), "EcVrfMNT6": ("mnt6753", "mnt4753_g1")}   # (Poseidon tag, group)
W, BITS = 4, 753
NUM_WINDOWS, WINDOW_SIZE = 2, 128                  # 256 chunks: one message element


def joint_products_per_row(w=W, bits=BITS):
    """two tables as vb_products_per_row counts them, then w (m - 1) doublings, 2 m mixed additions and on average one
    correction"""
    m = -(-bits // w)
    e = 1 << (w - 1)
    table = 2 + DBL + (e - 1) * ADD + e * 1 + INV + e * 4
    return 2 * table + w * (m - 1) * DBL + 2 * m * MADD + 1.0 * MADD


def bh_products_per_row(elements=1):
    return 256 * elements * MADD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    from ginger_lib_amd import ecvrf, poseidon, schnorr
    peak = gl.measure_fpmul_peak()
    joint, single = joint_products_per_row(), vb_products_per_row(W)
    doc = {"device": gl.device_name(), "fpmul_peak_per_s": peak, "window": W, "bh_windows": [NUM_WINDOWS, WINDOW_SIZE],
           "joint_products_per_row": joint, "two_batch_mul_products_per_row": 2 * single,
           "bh_products_per_row_L1": bh_products_per_row(), "schemes": {}}
    for name, (tag, curve) in SCHEMES.items():
        prm = poseidon.PoseidonParameters.from_json(PARAMS, tag)
        S = schnorr.FieldBasedSchnorrSignatureScheme(prm, curve)
        rs = np.random.default_rng(1)
        gxy, ginf = S.get_public_key(_rand(rs, NUM_WINDOWS * WINDOW_SIZE, TOP))
        B = ecvrf.BoweHopwoodPedersenCRH(curve, gxy, ginf, NUM_WINDOWS, WINDOW_SIZE)
        V = ecvrf.FieldBasedEcVrf(prm, B, curve)
        res = {}
        for lg in a.log2n:
            n = 1 << lg
            sk = _rand(rs, n, TOP)
            msg = _rand(rs, n, TOP).reshape(n, 1, 12)
            pk = V.get_public_key(sk)
            gam_xy, gam_inf = np.zeros((n, 24), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
            cs = np.zeros((n, 24), dtype=np.uint64)
            todo = np.arange(n)
            prove_s, prove_rows, prove_phases = [], 0, None
            for _ in range(64):                    # about 32 % of the nonces pass both range checks
                if not len(todo):
                    break
                k = _rand(rs, len(todo), TOP)
                t0 = time.perf_counter()
                (g_, gi_), c_, st = V.prove(sk[todo], (pk[0][todo], pk[1][todo]), msg[todo], k)
                dt = time.perf_counter() - t0
                if len(todo) == n:
                    prove_s.append(dt)
                    prove_phases = ecvrf.last_timing()
                    prove_rows = int(st.sum())
                ok = todo[st == 1]
                gam_xy[ok], gam_inf[ok], cs[ok] = g_[st == 1], gi_[st == 1], c_[st == 1]
                todo = todo[st != 1]
            assert not len(todo), "rows left unproved"
            ver_s, ver_phases = [], None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out, st = V.proof_to_hash(pk, msg, (gam_xy, gam_inf), cs)
                ver_s.append(time.perf_counter() - t0)
                ver_phases = ecvrf.last_timing()
            assert (st == 1).all(), "a device proof did not verify"
            # the joint kernel against two variable-base passes, same bases and scalars, same call
            k1, k2 = _rand(rs, n, TOP), _rand(rs, n, TOP)
            jt, tw = [], []
            for _ in range(a.reps):
                ecvrf.batch_double_mul(curve, pk[0], k1, gam_xy, k2, pk[1], gam_inf)
                jt.append(ecvrf.last_timing()[0]["variable_base"])
                schnorr.batch_mul(curve, pk[0], k1, pk[1])
                t1 = schnorr.last_timing()[0]["variable_base"]
                schnorr.batch_mul(curve, gam_xy, k2, gam_inf)
                tw.append(t1 + schnorr.last_timing()[0]["variable_base"])
            bj, bt = min(jt) / 1e3, min(tw) / 1e3
            res[str(lg)] = {
                "rows": n,
                "proof_to_hash_s": min(ver_s), "proof_to_hash_per_s": n / min(ver_s), "proof_to_hash_phases_ms": ver_phases[0],
                "proof_to_hash_total_ms": ver_phases[1],
                "prove_s": min(prove_s), "proofs_per_s": prove_rows / min(prove_s), "prove_accepted": prove_rows,
                "prove_phases_ms": prove_phases[0],
                "joint_kernel_s": bj, "two_batch_mul_s": bt, "joint_speedup": bt / bj,
                "joint_fraction_of_peak": joint * n / bj / peak, "two_batch_mul_fraction_of_peak": 2 * single * n / bt / peak,
            }
            print("%s 2^%d: %.0f proof_to_hash/s, %.0f proofs/s, joint %.3f s vs two passes %.3f s (%.3f of peak)" % (
                name, lg, n / min(ver_s), prove_rows / min(prove_s), bj, bt, joint * n / bj / peak), file=sys.stderr, flush=True)
        doc["schemes"][name] = res
        V.close()
        B.close()
        S.close()
        prm.close()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
