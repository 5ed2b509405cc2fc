#!/usr/bin/env python3
"""Constraint evaluation on the device, measured: create_proof of the `Benchmark` circuit with 2^k - 3 constraints over
MNT4-753, key resident with shift tables, in one warmed process, by two paths that are alternated:

  (a) prove_prepared on rows evaluated and converted outside the clock (three domain-sized uploads, gh_witness_map_dev, MSMs):
      rows_upload_ms + witness_map_ms + msm_stage_ms;
  (b) create_proof_r1cs from the Montgomery assignment already in host memory (one upload, gh_r1cs_witness_map_dev, MSMs).

The proof bytes of the two paths are compared.  Also reported: the device time of gh_r1cs_evaluate_dev and of
gh_r1cs_instance_map_dev alone (HIP events, gh_r1cs_last_timing), per-level times of one product over A (the closing row's
reduction chain: level 0 is the gather, the levels above sum its partials), terms per second and bytes gathered from the
shapes, and one timing of generate_parameters with and without the resident matrices (same bytes).  The spread of each path
(max - min over its proofs) is printed next to the difference of the means.

Prints one JSON document and writes it to --out.  --rehearse runs without a device: argument parsing, the circuit, the
flattening and the referee of tests/r1cs_ref.py on a small size.
Usage: timeout -k 10 900 python tools/r1cs_bench.py [--log-n 20] [--proofs 5] [--out profiles/r1cs_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shapes(lcs):
    """terms and the bytes a product moves, from the shapes alone: per term the index and the code (8 B) and one gathered
    operand in the internal form (104 B); per row one 96-byte result"""
    num_inputs, num_aux, at, bt, ct = lcs
    nnz = [sum(len(row) for row in rows) for rows in (at, bt, ct)]
    return {"nnz": dict(zip("ABC", nnz)), "terms": sum(nnz), "gathered_bytes": sum(nnz) * 104, "index_bytes": sum(nnz) * 8,
            "result_bytes": 3 * len(at) * 96, "longest_row": max(len(row) for row in at)}


def rehearse(args):
    import r1cs_ref as ref
    from __graft_entry__ import _load_pkg
    _load_pkg()
    groth16 = importlib.import_module("ginger_lib_amd.groth16")
    limbs = importlib.import_module("ginger_lib_amd.limbs")
    r1cs = importlib.import_module("ginger_lib_amd.r1cs")
    pairing, n = "mnt4753", 61
    r = limbs.MODULUS[pairing]
    lcs = groth16.benchmark_circuit_lcs(n)
    num_inputs, assignment, A, B, C = groth16.benchmark_circuit_rows(pairing, n)
    a, b, c = ref.evaluate(lcs, assignment, r)
    assert a[:n] == A and b[:n] == B and c[:n] == C
    flat = [r1cs.flatten(rows, r) for rows in lcs[2:]]
    assert all(int(f[0][-1]) == len(f[1]) == len(f[2]) for f in flat) and all(len(f[3]) == 1 for f in flat)
    out = {"rehearsal": True, "log_n": args.log_n, "proofs": args.proofs, "shapes_at_61": shapes(lcs), "measured": "not measured: no device"}
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log-n", type=int, default=20, help="the QAP domain: 2^k - 3 constraints")
    ap.add_argument("--proofs", type=int, default=5, help="timed proofs per path (at least 5 for the published numbers)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_bench.json"))
    ap.add_argument("--rehearse", action="store_true", help="no device: parse, build the circuit, run the referee on a small size")
    ap.add_argument("--no-generator", action="store_true", help="skip the second generate_parameters (with the resident matrices)")
    args = ap.parse_args()
    if args.rehearse:
        return rehearse(args)

    import pyref
    import support as S
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    groth16 = importlib.import_module("ginger_lib_amd.groth16")
    limbs = importlib.import_module("ginger_lib_amd.limbs")
    r1cs = importlib.import_module("ginger_lib_amd.r1cs")
    pairing = "mnt4753"
    field = gl.FIELDS["mnt4753_fr"]
    C1, C2 = pyref.CURVES[pairing + "_g1"], pyref.CURVES[pairing + "_g2"]
    rr = C1.order
    n_con = (1 << args.log_n) - 3
    prng = pyref.Rng(2026)
    alpha, beta, gamma, delta, tau, r_, s_ = (prng.field_elem(rr) for _ in range(7))
    g1, g2 = C1.mul(prng.next_u64() | 1, C1.G), C2.mul(prng.next_u64() | 1, C2.G)
    gen_args = (alpha, beta, gamma, delta, tau, S.proj_array(C1, g1), S.proj_array(C2, g2))
    out = {"device": gl.device_name(), "pairing": pairing, "log_n": args.log_n, "constraints": n_con}

    lcs = groth16.benchmark_circuit_lcs(n_con)
    out["shapes"] = shapes(lcs)
    t0 = time.perf_counter()
    res = r1cs.ResidentR1CS(gl, pairing, lcs)
    out["r1cs_upload_s"] = time.perf_counter() - t0          # flattening in Python, the host plan, the copies
    info = res.info()
    out["r1cs_info"] = info
    t0 = time.perf_counter()
    blob, _ = groth16.generate_parameters(gl, pairing, lcs, *gen_args)
    out["generate_parameters_s"] = time.perf_counter() - t0
    if not args.no_generator:
        t0 = time.perf_counter()
        blob_r, _ = groth16.generate_parameters(gl, pairing, lcs, *gen_args, r1cs=res)
        out["generate_parameters_r1cs_s"] = time.perf_counter() - t0
        out["generate_parameters_same_bytes"] = bool(blob_r == blob)
        del blob_r
    key = groth16.ResidentProvingKey.from_parameters(gl, pairing, blob, 3)
    del blob
    try:
        rows = groth16.benchmark_circuit_rows(pairing, n_con)
        t0 = time.perf_counter()
        prep = key.prepare_rows(rows, 0, 0, 0)                 # outside the clock of path (a)
        out["host_prepare_rows_s"] = time.perf_counter() - t0
        zm = limbs.mont_rows(rows[1], rr)                   # outside the clock of path (b)
        del rows
        proof_a = key.prove_prepared(prep, r_, s_)             # warm both paths: pools, pipeline slots, domain tables
        proof_b = key.create_proof_r1cs(res, zm, 0, 0, 0, r_, s_)
        out["same_proof_bytes"] = bool(proof_a == proof_b)
        ta, tb = [], []
        for _ in range(args.proofs):                           # alternated
            tm = {}
            pa = key.prove_prepared(prep, r_, s_, timing=tm)
            ta.append(tm["rows_upload_ms"] + tm["witness_map_ms"] + tm["msm_stage_ms"])
            last_a = tm
            tm = {}
            pb = key.create_proof_r1cs(res, zm, 0, 0, 0, r_, s_, timing=tm)
            tb.append(tm["assignment_upload_ms"] + tm["witness_map_ms"] + tm["msm_stage_ms"])
            last_b = tm
            out["same_proof_bytes"] = out["same_proof_bytes"] and pa == proof_a and pb == proof_a
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        diff = float(np.mean(ta) - np.mean(tb))
        out["paths"] = {"a_prove_prepared_ms": ta, "b_create_proof_r1cs_ms": tb, "a_mean_ms": float(np.mean(ta)), "b_mean_ms": float(np.mean(tb)),
                        "a_spread_ms": max(ta) - min(ta), "b_spread_ms": max(tb) - min(tb), "difference_ms": diff,
                        "difference_in_spreads": diff / spread if spread else None, "a_last_stages": last_a, "b_last_stages": last_b}
        # the device stages alone, by events
        nv, size = res.num_variables, res.size
        d_z = gl.DeviceBuffer(nv * 96).upload(zm)
        bufs = [gl.DeviceBuffer(size * 96) for _ in range(3)]
        d_u = gl.DeviceBuffer(size * 96)
        vouts = [gl.DeviceBuffer(nv * 96) for _ in range(3)]
        try:
            ev, im, lv = [], [], []
            for _ in range(3):
                res.evaluate_dev(d_z, *bufs)
                ev.append(r1cs.last_timing())
            tau_m = limbs.mont_rows([tau], rr)[0]
            gl._check(gl.load_library().gh_lagrange_coefficients_dev(field, args.log_n, gl._ptr(tau_m), d_u.ptr))
            for _ in range(3):
                res.instance_map_dev(d_u, *vouts)
                im.append(r1cs.last_timing())
            for _ in range(3):
                res.matvec_dev("A", d_z, bufs[0])
                lv.append(r1cs.last_timing())
        finally:
            for buf in [d_z, d_u] + bufs + vouts:
                buf.free()
        best = lambda runs: min(runs, key=lambda t: t[1])
        e_ph, e_tot = best(ev)
        i_ph, i_tot = best(im)
        l_ph, l_tot = best(lv)
        levels = info["levels"]["A"][0]
        terms = out["shapes"]["terms"]
        out["evaluate_dev"] = {"total_ms": e_tot, "phases_ms": e_ph[:info["levels"]["A"][0] + 2], "runs_total_ms": [t for _, t in ev],
                               "terms_per_s": terms / (e_tot * 1e-3) if e_tot else None,
                               "gathered_gb_per_s": out["shapes"]["gathered_bytes"] / (e_tot * 1e-3) / 1e9 if e_tot else None}
        out["instance_map_dev"] = {"total_ms": i_tot, "phases_ms": i_ph[:max(info["levels"][m][1] for m in "ABC") + 2],
                                   "runs_total_ms": [t for _, t in im], "terms_per_s": terms / (i_tot * 1e-3) if i_tot else None}
        out["matvec_A_levels_ms"] = {"convert": l_ph[0], "levels": l_ph[1:1 + levels], "total_ms": l_tot,
                                     "note": "level 0 gathers every row of A; levels 1 .. reduce the closing row's partials"}
    finally:
        key.free()
        res.free()
        gl.dev_trim()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
