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

--scheme gm17 measures GM17's create_proof the same way: (a) is gm17's prove_prepared on SAP rows
formed and converted outside the clock (sap_rows_from_r1cs and the conversions are timed separately), (b) its
create_proof_r1cs; next to them gh_sap_rows_dev and gh_sap_instance_map_dev alone by events and per phase, and
generate_parameters with and without the resident matrices.  --log-n is still the R1CS size 2^k - 3; the SAP domain is 2^(k+1).
Its default output is profiles/sap_bench.json.

Prints one JSON document and writes it to --out.  --rehearse runs without a device: argument parsing, the circuit, the
flattening and the referee of tests/r1cs_ref.py on a small size.
Usage: timeout -k 10 900 python tools/r1cs_bench.py [--scheme groth16|gm17] [--log-n 20] [--proofs 5] [--out profiles/r1cs_bench.json]"""
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
    if args.scheme == "gm17":
        import sap_ref
        gm17 = importlib.import_module("ginger_lib_amd.gm17")
        full, sa, sc, log_n = gm17.sap_rows_from_r1cs(pairing, num_inputs, assignment, A, B, C)
        assert (full, sa, sc) == sap_ref.rows(lcs, assignment, r) and 1 << log_n == sap_ref.domain_size(n, num_inputs)
    out = {"rehearsal": True, "scheme": args.scheme, "log_n": args.log_n, "proofs": args.proofs, "shapes_at_61": shapes(lcs), "measured": "not measured: no device"}
    print(json.dumps(out))
    return 0


def alternate(run_a, run_b, proofs, same):
    """the two paths alternated, `proofs` each: run_x(timing) -> proof; same(proof) -> bool.  -> (paths report, all proofs equal)"""
    ta, tb, ok = [], [], True
    for _ in range(proofs):
        last_a, last_b = {}, {}
        ok = same(run_a(last_a)) and ok
        ta.append(sum(last_a.values()))
        ok = same(run_b(last_b)) and ok
        tb.append(sum(last_b.values()))
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    diff = float(np.mean(ta) - np.mean(tb))
    return {"a_prove_prepared_ms": ta, "b_create_proof_r1cs_ms": tb, "a_mean_ms": float(np.mean(ta)), "b_mean_ms": float(np.mean(tb)),
            "a_spread_ms": max(ta) - min(ta), "b_spread_ms": max(tb) - min(tb), "difference_ms": diff,
            "difference_in_spreads": diff / spread if spread else None, "a_last_stages": last_a, "b_last_stages": last_b}, ok


def main_gm17(args):
    import pyref
    import support as S
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.init()
    groth16 = importlib.import_module("ginger_lib_amd.groth16")
    gm17 = importlib.import_module("ginger_lib_amd.gm17")
    limbs = importlib.import_module("ginger_lib_amd.limbs")
    r1cs = importlib.import_module("ginger_lib_amd.r1cs")
    sap = importlib.import_module("ginger_lib_amd.sap")
    pairing = "mnt4753"
    field = gl.FIELDS["mnt4753_fr"]
    C1, C2 = pyref.CURVES[pairing + "_g1"], pyref.CURVES[pairing + "_g2"]
    rr = C1.order
    n_con = (1 << args.log_n) - 3
    prng = pyref.Rng(2027)
    alpha, beta, gamma, tau, r_, d1, d2 = (prng.field_elem(rr) for _ in range(7))
    g1, g2 = C1.mul(prng.next_u64() | 1, C1.G), C2.mul(prng.next_u64() | 1, C2.G)
    gen_args = (alpha, beta, gamma, tau, S.proj_array(C1, g1), S.proj_array(C2, g2))
    out = {"device": gl.device_name(), "scheme": "gm17", "pairing": pairing, "log_n": args.log_n, "constraints": n_con}
    lcs = groth16.benchmark_circuit_lcs(n_con)
    out["shapes"] = shapes(lcs)
    t0 = time.perf_counter()
    res = r1cs.ResidentR1CS(gl, pairing, lcs)
    out["r1cs_upload_s"] = time.perf_counter() - t0
    info = res.info()
    out["r1cs_info"] = info
    out["sap_info"] = sinfo = sap.sap_info(res)
    t0 = time.perf_counter()
    pk, ginfo = gm17.generate_parameters(gl, pairing, lcs, *gen_args)
    out["generate_parameters_s"] = time.perf_counter() - t0
    if not args.no_generator:
        t0 = time.perf_counter()
        pk_r, ginfo_r = gm17.generate_parameters(gl, pairing, lcs, *gen_args, r1cs=res)
        out["generate_parameters_r1cs_s"] = time.perf_counter() - t0
        out["generate_parameters_same_key"] = bool(sorted(pk) == sorted(pk_r) and all((np.asarray(pk[k]) == np.asarray(pk_r[k])).all() for k in pk)
                                                   and ginfo == ginfo_r)
        del pk_r, ginfo_r
    del ginfo
    key = gm17.ResidentGm17Key(gl, pairing, pk, 3)
    del pk
    try:
        rows = groth16.benchmark_circuit_rows(pairing, n_con)          # outside every clock
        t0 = time.perf_counter()
        full, a, c, _ = gm17.sap_rows_from_r1cs(pairing, *rows)
        t1 = time.perf_counter()
        limbs.canon_rows(full), limbs.mont_rows(a, rr), limbs.mont_rows(c, rr)
        t2 = time.perf_counter()
        out["host_sap_rows_from_r1cs_s"], out["host_conversions_s"] = t1 - t0, t2 - t1      # what leaves the caller
        del full, a, c
        prep = key.prepare_rows(rows, d1, d2)                          # outside the clock of path (a)
        zm = limbs.mont_rows(rows[1], rr)                              # outside the clock of path (b)
        del rows
        pb = lambda proof: gm17.proof_bytes(pairing, proof)
        proof_a = pb(key.prove_prepared(prep, r_))                     # warm both paths: pools, pipeline slots, domain tables
        out["same_proof_bytes"] = bool(proof_a == pb(key.create_proof_r1cs(res, zm, d1, d2, r_)))
        out["paths"], same = alternate(lambda tm: key.prove_prepared(prep, r_, timing=tm), lambda tm: key.create_proof_r1cs(res, zm, d1, d2, r_, timing=tm),
                                       args.proofs, lambda proof: pb(proof) == proof_a)
        out["same_proof_bytes"] = out["same_proof_bytes"] and same
        # the device stages alone, by events
        nv, size, sap_nv = res.num_variables, sinfo["size"], sinfo["sap_num_variables"]
        d_z = gl.DeviceBuffer(nv * 96).upload(zm)
        bufs = [gl.DeviceBuffer(rows_ * 96) for rows_ in (size, size, sap_nv, sap_nv - 2, size, sap_nv + 1, sap_nv + 1)]
        d_a, d_c, d_s, d_x, d_u, v_a, v_c = bufs
        try:
            rw, rs, im = [], [], []
            for _ in range(3):
                sap.sap_rows_dev(res, d_z, d_a, d_c)
                rw.append(sap.last_timing())
            for _ in range(3):
                sap.sap_rows_dev(res, d_z, d_a, d_c, d_s, d_x)
                rs.append(sap.last_timing())
            tau_m = limbs.mont_rows([tau], rr)[0]
            gl._check(gl.load_library().gh_lagrange_coefficients_dev(field, sinfo["sap_log_n"], gl._ptr(tau_m), d_u.ptr))
            for _ in range(3):
                sap.sap_instance_map_dev(res, d_u, v_a, v_c)
                im.append(sap.last_timing())
        finally:
            for buf in [d_z] + bufs:
                buf.free()
        best = lambda runs: min(runs, key=lambda t: t[1])
        terms = out["shapes"]["terms"]
        n_ph = max(max(info["levels"][m]) for m in "ABC") + 2
        for name, runs in (("sap_rows_dev", rw), ("sap_rows_dev_with_scalars", rs), ("sap_instance_map_dev", im)):
            ph, tot = best(runs)
            out[name] = {"total_ms": tot, "phases_ms": ph[:n_ph], "runs_total_ms": [t for _, t in runs], "terms_per_s": terms / (tot * 1e-3) if tot else None,
                         "phases": "conversion or split, levels 0 .. of the three products, the SAP kernel (last entry)"}
    finally:
        key.free()
        res.free()
        gl.dev_trim()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scheme", choices=("groth16", "gm17"), default="groth16")
    ap.add_argument("--log-n", type=int, default=20, help="the QAP domain: 2^k - 3 constraints")
    ap.add_argument("--proofs", type=int, default=5, help="timed proofs per path (at least 5 for the published numbers)")
    ap.add_argument("--out", default=None, help="default: profiles/r1cs_bench.json, or profiles/sap_bench.json with --scheme gm17")
    ap.add_argument("--rehearse", action="store_true", help="no device: parse, build the circuit, run the referee on a small size")
    ap.add_argument("--no-generator", action="store_true", help="skip the second generate_parameters (with the resident matrices)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sap_bench.json" if args.scheme == "gm17" else "r1cs_bench.json")
    if args.rehearse:
        return rehearse(args)
    if args.scheme == "gm17":
        return report(main_gm17(args), args)

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
        out["paths"], same = alternate(lambda tm: key.prove_prepared(prep, r_, s_, timing=tm),
                                       lambda tm: key.create_proof_r1cs(res, zm, 0, 0, 0, r_, s_, timing=tm), args.proofs, lambda proof: proof == proof_a)
        out["same_proof_bytes"] = out["same_proof_bytes"] and same
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
    return report(out, args)


def report(out, args):
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
