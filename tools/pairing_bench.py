#!/usr/bin/env python3
"""MNT4-753 (or, with --engine mnt6753, MNT6-753) pairings and Groth16 verification on the device: pairings/s (gh_pairing_product, k = 1) and verifications/s
(gh_groth16_verify, two public inputs) at 2^16 and 2^20 rows, warmed, best of 3, timed around the call (which synchronises
the device before it returns), the phase split of every call, and the Miller and final-exponentiation kernels' products per
row (counted from the formulas as written in the PairingTower of csrc/pairing29.h and the sparse products of its two engines, squarings as products)
over their kernel time as a fraction of
the product peak gh_measure_fpmul_peak measures in the same run.

The rows are valid proofs of a key made from random scalars, so that (A, B, C) is known in the exponent:
    a b = alpha beta + (k_0 + sum_j x_j k_j) gamma + c delta;
4096 distinct rows are tiled to the batch size (no kernel looks at another row).  Every status must be 1.
Prints one JSON document.

--scheme gm17 measures gh_gm17_verify instead of the pairing: valid proofs (a G, a H, c G) of a GM17 key known in the exponent,
    (a + alpha)(a + beta) = alpha beta + (k_0 + sum_j x_j k_j) gamma + c,
two public inputs, next to gh_groth16_verify in the same run (their ratio), with the product counts it divides by, and merges
the document into --out (profiles/pairing_bench.json) under "gm17" / the engine.
Usage: timeout -k 10 900 python tools/pairing_bench.py [--engine mnt4753|mnt6753] [--scheme groth16|gm17] [--log2n 16 20] [--reps 3] > out.json"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from schnorr_bench import INV, MADD, ADD   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DISTINCT = 4096
N_INPUTS = 2
# products of the steps of csrc/pairing29.h (its header counts them for both engines, MNT4-753 / MNT6-753)
FQ4_MUL, FQ4_SQR, MUL_023, CYC_SQR = 9, 6, 8, 4
DBL_STEP, ADD_STEP, PREPARED_LINE = 25 + 4, 28 + 8, 2
FQ3_MUL, FQ3_SQR = 6, 5
FQ6_MUL, FQ6_SQR, MUL_2345, CYC_SQR6 = 3 * FQ3_MUL, 2 * FQ3_MUL, 3 + 2 * FQ3_MUL, 2 * FQ3_SQR
DBL_STEP6, ADD_STEP6, PREPARED_LINE6 = 11 * FQ3_SQR + FQ3_MUL + 6, 7 * FQ3_MUL + 4 * FQ3_SQR + 15, 3


def products(consts, engine="mnt4753"):
    naf, w0 = consts["ate_naf"], consts["w0_naf"]
    dig, nz = len(naf), sum(1 for d in naf if d)
    g_ic = N_INPUTS * (2 + -(-753 // 8) * MADD + ADD) + (1 + 3 + INV / 16 + 2)
    if engine == "mnt4753":
        variable = dig * (DBL_STEP + FQ4_MUL) + nz * (ADD_STEP + FQ4_MUL)
        prepared = (dig + nz) * (PREPARED_LINE + MUL_023)
        squarings = dig * FQ4_SQR
        fq4_inv = 4 + (2 + INV + 2 + 2) + 6
        final_exp = fq4_inv + 2 * FQ4_MUL + 3 * 2 + (len(w0) - 1) * CYC_SQR + (sum(1 for d in w0 if d) - 1) * FQ4_MUL + FQ4_MUL + 4
        setup1, setup3, checks = 6, 10, 21
    else:
        variable = dig * (DBL_STEP6 + FQ6_MUL) + nz * (ADD_STEP6 + FQ6_MUL)
        prepared = (dig + nz) * (PREPARED_LINE6 + MUL_2345)
        squarings = dig * FQ6_SQR
        # inverse: two Fq3 squarings, the Fq3 inverse (9 + 3 products and one inversion), two Fq3 products
        fq6_inv = 2 * FQ3_SQR + (9 + INV + 3) + 2 * FQ3_MUL
        # Frobenius: power 3 costs 3 products (c1 times one coefficient), power 1 costs 4 + 3
        final_exp = fq6_inv + 3 + FQ6_MUL + 7 + FQ6_MUL + 7 + (len(w0) - 1) * CYC_SQR6 + (sum(1 for d in w0 if d) - 1) * FQ6_MUL + FQ6_MUL + 6
        # setup: the conversions of x_P, y_P (2) and of x_Q, y_Q (6) per pair; checks: the proof points' curve equations
        setup1, setup3, checks = 8, 12, 4 + 6 + (2 * FQ3_SQR + FQ3_MUL + 6)
    # GM17 (csrc/gm17_sum.h counts the sums): test1 is Groth16's Miller shape, test2 one variable and one prepared pair; the sums
    # kernel converts A, B and the two key points (2 + 2 D + 2 + 2 D), writes -S1, S2, -B (2 + 4 D) and adds in G1 and in G2
    d = 2 if engine == "mnt4753" else 3
    sum_g1, sum_g2 = 4 + INV + 2, (10 + 2 + INV + 2 + 2 if d == 2 else 22 + 9 + INV + 2 + 3)
    sums = sum_g1 + sum_g2 + 4 + 4 * d + 2 + 4 * d
    setup2 = setup3 - 2
    gm17 = {"gm17_sums": sums, "gm17_test1_miller": variable + 2 * prepared + squarings + setup3,
            "gm17_test2_miller": variable + prepared + squarings + setup2, "gm17_g_psi_and_checks": g_ic + checks,
            "gm17_total": 2 * variable + 3 * prepared + 2 * squarings + setup3 + setup2 + 2 * final_exp + sums + g_ic + checks}
    return {**gm17, "variable_pair": variable, "prepared_pair": prepared, "shared_squarings": squarings, "final_exponentiation": final_exp,
            "pairing_miller": variable + squarings + setup1, "groth16_miller": variable + 2 * prepared + squarings + setup3,
            "groth16_g_ic_and_checks": g_ic + checks,
            "pairing_total": variable + squarings + setup1 + final_exp,
            "groth16_total": variable + 2 * prepared + squarings + setup3 + final_exp + g_ic + checks}


def _rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(96, "little") for v in vals), dtype=np.uint64).reshape(-1, 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engine", choices=["mnt4753", "mnt6753"], default="mnt4753")
    ap.add_argument("--scheme", choices=["groth16", "gm17"], default="groth16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_bench.json"), help="--scheme gm17: the document to merge into")
    a = ap.parse_args()
    eng = a.engine
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    from ginger_lib_amd import limbs, pairing
    peak = gl.measure_fpmul_peak()
    C = json.load(open(os.path.join(GOLDEN, "constants.json")))
    consts = json.load(open(os.path.join(GOLDEN, "pairing_constants.json" if eng == "mnt4753" else "pairing6_constants.json")))
    prod = products(consts, eng)
    p, r = int(C["fields"]["p4"]["p"], 16), int(C["fields"]["p6"]["p"], 16)
    if eng == "mnt6753":
        p, r = r, p                                             # the cycle: MNT6-753's base field is MNT4-753's group order
    mont = lambda vals: limbs.mont_rows(vals, p).reshape(-1)
    c1, c2 = C["curves"][eng + "_g1"], C["curves"][eng + "_g2"]
    deg = len(c2["gx"])
    g1_xyz = mont([int(c1["gx"][0], 16), int(c1["gy"][0], 16), 1])
    g2_xyz = mont([int(v, 16) for v in c2["gx"] + c2["gy"]] + [1] + [0] * (deg - 1))
    t1, t2 = gl.FixedBaseMSM(eng + "_g1", g1_xyz, 753, 10), gl.FixedBaseMSM(eng + "_g2", g2_xyz, 753, 8)
    g1 = lambda ks: t1.multi_scalar_mul_affine(_rows(ks))
    g2 = lambda ks: t2.multi_scalar_mul_affine(_rows(ks))
    rng = random.Random(14)
    alpha, beta, gamma, delta = (rng.randrange(1, r) for _ in range(4))
    ks = [rng.randrange(1, r) for _ in range(N_INPUTS + 1)]
    av = [rng.randrange(1, r) for _ in range(DISTINCT)]
    bv = [rng.randrange(1, r) for _ in range(DISTINCT)]
    xv = [[rng.randrange(r) for _ in range(N_INPUTS)] for _ in range(DISTINCT)]
    di = pow(delta, -1, r)
    cv = [(x * y - alpha * beta - (ks[0] + sum(u * k for u, k in zip(xs, ks[1:]))) * gamma) * di % r for x, y, xs in zip(av, bv, xv)]
    A, B, Cc = g1(av), g2(bv), g1(cv)
    vk2 = g2([gamma, delta, beta])
    abc = g1(ks + [alpha])
    gt = pairing.pairing_product((abc[0][-1:], abc[1][-1:]), (vk2[0][2:], vk2[1][2:]), engine=eng)
    pvk = pairing.PreparedVerifyingKey(gt, vk2[0][0], vk2[0][1], abc[0][:-1], engine=eng)
    X = limbs.mont_rows([u for xs in xv for u in xs], r).reshape(DISTINCT, N_INPUTS * 12)
    if a.scheme == "gm17":
        from ginger_lib_amd import gm17_verify
        cg = [((x + alpha) * (x + beta) - alpha * beta - (ks[0] + sum(u * k for u, k in zip(xs, ks[1:]))) * gamma) % r for x, xs in zip(av, xv)]
        gB, gC = g2(av), g1(cg)
        k1, k2 = g1([alpha, gamma]), g2([beta, gamma, 1])
        gpvk = gm17_verify.PreparedVerifyingKey(k1[0][0], k2[0][0], k1[0][1], k2[0][1], k2[0][2], abc[0][:-1], engine=eng)
        print("products per row: %s" % json.dumps({k: v for k, v in prod.items() if k.startswith(("gm17", "groth16"))}), file=sys.stderr, flush=True)
    t1.free()
    t2.free()
    doc = {"device": gl.device_name(), "engine": eng, "fpmul_peak_per_s": peak, "public_inputs": N_INPUTS, "products_per_row": prod, "rows": {}}
    for lg in a.log2n:
        n = 1 << lg
        tile = lambda arr: np.ascontiguousarray(np.tile(arr, (-(-n // DISTINCT),) + (1,) * (arr.ndim - 1))[:n])
        pa, pb, pc, px = [(tile(q[0]), tile(q[1])) for q in (A, B, Cc)] + [tile(X)]
        res = {"rows": n}
        calls = [("pairing", lambda: pairing.pairing_product(pa, pb, engine=eng), None, prod["pairing_miller"], pairing),
                 ("groth16_verify", lambda: pvk.verify(pa, pb, pc, px), 1, prod["groth16_miller"], pairing)]
        if a.scheme == "gm17":
            qb, qc = [(tile(q[0]), tile(q[1])) for q in (gB, gC)]
            calls = calls[1:] + [("gm17_verify", lambda: gpvk.verify(pa, qb, qc, px), 1, None, gm17_verify)]
        for name, call, ok, miller, mod in calls:
            out = call()                                        # warm: tables, pooled buffers
            if ok is not None:
                assert (out == ok).all(), "a valid proof did not verify"
            best, phases = None, None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                dt = time.perf_counter() - t0
                if best is None or dt < best:
                    best, phases = dt, mod.last_timing()
            ms = phases[0]
            if name == "gm17_verify":
                mil = ms["test1_miller"] + ms["test2_miller"]
                fe = ms["test1_final_exp"] + ms["test2_final_exp"]
                res[name] = {"s": best, "per_s": n / best, "phases_ms": ms, "total_ms": phases[1],
                             "miller_fraction_of_peak": (prod["gm17_test1_miller"] + prod["gm17_test2_miller"]) * n / (mil / 1e3) / peak,
                             "final_exp_fraction_of_peak": 2 * prod["final_exponentiation"] * n / (fe / 1e3) / peak,
                             "ratio_to_groth16_verify": best / res["groth16_verify"]["s"],
                             "predicted_ratio": prod["gm17_total"] / prod["groth16_total"]}
                print("gm17_verify 2^%d: %.0f /s, Miller %.1f + %.1f ms (%.3f of peak), final exponentiation %.1f ms, %.2f x groth16_verify (products: %.2f)" % (
                    lg, n / best, ms["test1_miller"], ms["test2_miller"], res[name]["miller_fraction_of_peak"], fe,
                    res[name]["ratio_to_groth16_verify"], res[name]["predicted_ratio"]), file=sys.stderr, flush=True)
                continue
            res[name] = {"s": best, "per_s": n / best, "phases_ms": ms, "total_ms": phases[1],
                         "miller_fraction_of_peak": miller * n / (ms["miller"] / 1e3) / peak,
                         "final_exp_fraction_of_peak": prod["final_exponentiation"] * n / (ms["final_exp"] / 1e3) / peak}
            print("%s 2^%d: %.0f /s, Miller %.1f ms (%.3f of peak), final exponentiation %.1f ms (%.3f of peak)" % (
                name, lg, n / best, ms["miller"], res[name]["miller_fraction_of_peak"], ms["final_exp"],
                res[name]["final_exp_fraction_of_peak"]), file=sys.stderr, flush=True)
        doc["rows"][str(lg)] = res
    pvk.close()
    if a.scheme == "gm17":
        gpvk.close()
        merged = json.load(open(a.out)) if os.path.exists(a.out) else {}
        merged.setdefault("gm17", {})[eng] = doc
        with open(a.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
