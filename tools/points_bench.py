#!/usr/bin/env python3
"""Point validation on the device: rows/s of gh_group_membership on G2, of gh_points_decompress on G1 and G2 and of
gh_groth16_verify_checked next to gh_groth16_verify (two public inputs) for one engine, warmed, best of --reps, timed around the
call (which synchronises the device before it returns); each kernel's products per row (counted from the formulas as written in
csrc/sqrt29.h and csrc/ec29.h, squarings as products) over its kernel time as a fraction of the product peak
gh_measure_fpmul_peak measures in the same run; and the ratio verify_checked : verify next to the ratio of the product counts.

The rows are those of tools/pairing_bench.py: valid proofs of a key made from random scalars, 4096 distinct rows tiled to the
batch size.  Every point is a member and every proof verifies; a kernel's time does not depend on that (its loops have fixed
trip counts), only the few exceptional group steps of a point outside the subgroup would diverge.
One run covers one engine: its G2 for membership, its G1 and G2 for decompression; both G2s and all four curves take two runs.
Prints one JSON document and merges it into --out (profiles/points_bench.json) under the engine.
Usage: timeout -k 10 900 python tools/points_bench.py [--engine mnt4753|mnt6753] [--log2n 20] [--reps 2] > out.json"""
import argparse
import json
import os
import random
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pairing_bench import DISTINCT, GOLDEN, N_INPUTS, _rows, products as pairing_products   # noqa: E402
from schnorr_bench import INV   # noqa: E402

# products of a field product and squaring (fp29.h: Karatsuba Fq2 3 / complex squaring 2; Fq3 6 / CH-SQR2 5)
MUL = {1: 1, 2: 3, 3: 6}
SQR = {1: 1, 2: 2, 3: 5}


def _macro(hdr, name):
    return re.search(r"#define %s (.*)" % name, hdr).group(1).strip()


def sqrt_products(hdr, name, deg):
    """Tonelli-Shanks of sqrt29.h for a square: the power (EBITS - 1 squarings, one product per further set bit), x and b (2), the
    rounds ((S-1)(S-2)/2 squarings of b, S - 1 squarings of z, two products in every other round on average), the final check"""
    s, ebits = int(_macro(hdr, name + "_SQRT_S")), int(_macro(hdr, name + "_SQRT_EBITS"))
    ones = sum(bin(int(t.strip().rstrip("u"), 0)).count("1") for t in _macro(hdr, name + "_SQRT_E32").strip("{}").split(","))
    return (ebits - 1 + (s - 1) * (s - 2) // 2 + (s - 1) + 1) * SQR[deg] + (ones - 1 + 2 + (s - 1)) * MUL[deg]


def products(engine):
    hdr = open(os.path.join(ROOT, "ginger-lib_amd", "csrc", "sqrt_constants_gen.h")).read()
    fam = "GH_MNT4_R" if engine == "mnt4753" else "GH_MNT6_R"
    d = 2 if engine == "mnt4753" else 3
    digits, nonzero = int(_macro(hdr, fam + "_DIGITS")), int(_macro(hdr, fam + "_NONZERO"))
    m, s = MUL[d], SQR[d]
    dbl, madd = 5 * m + 6 * s, 9 * m + 2 * s                       # dbl-2007-bl, madd-1998-cmo as ec29.h writes them
    chain = (digits - 1) * dbl + (nonzero - 1) * madd
    curve_eq = lambda k: 2 * SQR[k] + MUL[k]                       # x^2, x^3, y^2 (or the right-hand side and the check of the root)
    member_g2 = 2 * d + curve_eq(d) + chain                        # the conversions of x and y, the curve equation, r P
    member_g1 = 2 + curve_eq(1)
    fq = "GH_P4" if engine == "mnt4753" else "GH_P6"
    root_g1 = sqrt_products(hdr, fq, 1)
    # Fq2: the norm (2), the root of the norm, one or two roots of delta (1.5 on average), 3 products and an inversion
    root_g2 = (2 + 2.5 * root_g1 + 3 + INV) if d == 2 else sqrt_products(hdr, "GH_P6Q3", 3)
    # decompression: x from its canonical words (d), x^2 and x^3 (the check of the root is counted with it), the root, the parity
    # (at most one product per coefficient), r P on G2, x and y back to the ABI's form (2 d)
    dec_g1 = 1 + SQR[1] + MUL[1] + root_g1 + 1 + 2
    dec_g2 = d + SQR[d] + MUL[d] + root_g2 + d + chain + 2 * d
    return {"fq_sqrt": root_g1, "g2_sqrt": root_g2, "r_chain": chain, "membership_g1": member_g1, "membership_g2": member_g2,
            "decompress_g1": dec_g1, "decompress_g2": dec_g2, "validate_checked": 2 * member_g1 + member_g2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--engine", choices=["mnt4753", "mnt6753"], default="mnt4753")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_bench.json"), help="the document to merge into")
    a = ap.parse_args()
    eng = a.engine
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    from ginger_lib_amd import limbs, pairing, points
    peak = gl.measure_fpmul_peak()
    C = json.load(open(os.path.join(GOLDEN, "constants.json")))
    consts = json.load(open(os.path.join(GOLDEN, "pairing_constants.json" if eng == "mnt4753" else "pairing6_constants.json")))
    prod = products(eng)
    prod["groth16_total"] = pairing_products(consts, eng)["groth16_total"]
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
    rng = random.Random(15)
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
    t1.free()
    t2.free()
    n1, n2 = eng + "_g1", eng + "_g2"
    ca, cb = points.compress_limbs(n1, A), points.compress_limbs(n2, B)
    doc = {"device": gl.device_name(), "engine": eng, "fpmul_peak_per_s": peak, "public_inputs": N_INPUTS, "products_per_row": prod, "rows": {}}
    print("products per row: %s" % json.dumps(prod), file=sys.stderr, flush=True)
    for lg in a.log2n:
        n = 1 << lg
        tile = lambda arr: np.ascontiguousarray(np.tile(arr, (-(-n // DISTINCT),) + (1,) * (arr.ndim - 1))[:n])
        pa, pb, pc, px = [(tile(q[0]), tile(q[1])) for q in (A, B, Cc)] + [tile(X)]
        xa, xb = [(tile(q[0]), tile(q[1])) for q in (ca, cb)]
        res = {"rows": n}
        # name, the call, what every row must give, the products of its validate kernel(s), whose timing record holds them
        calls = [("membership_g2", lambda: points.group_membership_test(n2, pb), lambda o: o.all(), prod["membership_g2"]),
                 ("decompress_g1", lambda: points.decompress_limbs(n1, *xa), lambda o: not o[1].any() and (o[0][0] == pa[0]).all(), prod["decompress_g1"]),
                 ("decompress_g2", lambda: points.decompress_limbs(n2, *xb), lambda o: not o[1].any() and (o[0][0] == pb[0]).all(), prod["decompress_g2"]),
                 ("groth16_verify", lambda: pvk.verify(pa, pb, pc, px), lambda o: (o == 1).all(), None),
                 ("groth16_verify_checked", lambda: pvk.verify_checked(pa, pb, pc, px), lambda o: (o[0] == 1).all() and not o[1].any(), prod["validate_checked"])]
        for name, call, good, kernel_products in calls:
            assert good(call()), name                             # warm: tables, pooled buffers
            best, tm, ptm = None, None, None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                dt = time.perf_counter() - t0
                if best is None or dt < best:
                    best, tm, ptm = dt, points.last_timing(), pairing.last_timing()
            res[name] = {"s": best, "per_s": n / best}
            if kernel_products is not None:
                res[name].update({"phases_ms": tm[0], "validate_fraction_of_peak": kernel_products * n / (tm[0]["validate"] / 1e3) / peak})
            if name.startswith("groth16"):
                res[name]["pairing_phases_ms"] = ptm[0]
            if name == "groth16_verify_checked":
                res[name].update({"ratio_to_groth16_verify": best / res["groth16_verify"]["s"],
                                  "predicted_ratio": (prod["groth16_total"] + prod["validate_checked"]) / prod["groth16_total"]})
            print("%s 2^%d: %.0f /s%s%s" % (name, lg, n / best,
                                            ", validate %.1f ms (%.3f of peak)" % (tm[0]["validate"], res[name]["validate_fraction_of_peak"]) if kernel_products else "",
                                            ", %.2f x groth16_verify (products: %.2f)" % (res[name]["ratio_to_groth16_verify"], res[name]["predicted_ratio"])
                                            if name == "groth16_verify_checked" else ""), file=sys.stderr, flush=True)
        doc["rows"][str(lg)] = res
    pvk.close()
    merged = json.load(open(a.out)) if os.path.exists(a.out) else {}
    merged[eng] = doc
    with open(a.out, "w") as f:
        f.write(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
