"""The GM17 prover over a device-resident proving key.

Mirror of proof-systems/src/gm17/prover.rs:201-352 (create_proof): the R1CS -> SAP witness map
(gm17/r1cs_to_sap.rs:99-245; its transforms are gh_sap_witness_map_dev) followed by the MSM stage
(prover.rs:267-343): nine multi_scalar_mul calls over a_query, b_query, c_query_1, c_query_2 and
g_gamma2_z_t (gm17/mod.rs:136-147, getters :237-330), a dozen single scalar multiplications and additions,
then into_affine() of A, B, C.  Same restructuring as groth16.py: every query is ONE resident vector that
carries the single points the reference adds by hand, so a proof is five MSMs -- four on G1 as one pipelined
batch (gh_msm_resident_dev_batch), one on G2 -- and the sums are the same group elements:

  A = MSM(a_query[1..] || a_query[0] || g_gamma_z ; input || aux || 1 || r + d1)                       (:268-279)
  B = MSM(b_query[1..] || b_query[0] || h_gamma_z ; the same scalars)                                  (:284-296)
  C = MSM(c_query_1 || g_gamma2_z2 || g_ab_gamma_z ; aux || r^2 + 2 r d1 || r + d1)                   (:306-308, :327-331)
      + r * MSM(c_query_2[1..] || c_query_2[0] ; input || aux || 1)                                    (:313-317, :330, :332-333)
      + MSM(g_gamma2_z_t || g_gamma2_z_t[0] ; h || d2)                                                 (:322-325, :331)

GM17's Proof / Parameters have no byte format in the reference (gm17/mod.rs:59-69, :186-196: unimplemented), so the
proof is returned as three affine points in the C ABI's form; `proof_bytes` writes them the way GroupAffine::write
would (short_weierstrass_projective.rs:185-192), which is what the parity tests compare.
"""
import contextlib
import time

import numpy as np

from . import sap
from .limbs import FR_FIELD, MODULUS, affine_to_wire, canon_rows, domain_size, ints_from_canon_rows, ints_from_mont_rows, mont_rows
from .prover import ResidentQueries, into_repr, upload_rows


def sap_rows_from_r1cs(pairing, num_inputs, assignment, A, B, C):
    """The host part of R1CStoSAP::witness_map (r1cs_to_sap.rs:123-148, :159-184, :198-219): from the evaluated R1CS rows
    A_i = <at_i, x>, B_i, C_i and the assignment x (Python integers) to the extended assignment and the two vectors the
    transforms start from.  -> (full_assignment, a, c, log_n): a and c have 2^log_n entries."""
    r = MODULUS[pairing]
    n_con = len(A)
    ni = num_inputs
    full = list(assignment)
    n_var = len(full)                                            # num_inputs + num_aux
    extra = [(x - y) * (x - y) % r for x, y in zip(A, B)]        # :127-141
    full += extra
    for i in range(1, ni):                                       # :144-149
        full.append((full[i] - 1) * (full[i] - 1) % r)
    size = domain_size(2 * n_con + 2 * (ni - 1) + 1)             # :151-155
    off = 2 * n_con
    var_off, var_off2 = n_var, n_var + n_con - 1
    a = [0] * size
    c = [0] * size
    for i in range(n_con):
        a[2 * i] = (A[i] + B[i]) % r
        a[2 * i + 1] = (A[i] - B[i]) % r
        c[2 * i] = (4 * C[i] + full[var_off + i]) % r            # :200-212
        c[2 * i + 1] = full[var_off + i]
    a[off] = 1
    c[off] = 1
    for i in range(1, ni):
        a[off + 2 * i - 1] = (full[i] + 1) % r
        a[off + 2 * i] = (full[i] - 1) % r
        c[off + 2 * i - 1] = (4 * full[i] + full[var_off2 + i]) % r
        c[off + 2 * i] = full[var_off2 + i]
    return full, a, c, size.bit_length() - 1


class ResidentGm17Key(ResidentQueries):
    """pk: dict of numpy arrays in the ABI formats (Montgomery x || y rows, all points finite): a_query, c_query_2 (n x 24),
    c_query_1 (n - num_inputs rows), g_gamma2_z_t (m x 24), b_query (n x 24*deg), and the single points g_gamma_z,
    g_ab_gamma_z, g_gamma2_z2 (24 u64), h_gamma_z (24*deg u64)."""

    def __init__(self, gl, pairing, pk, num_inputs, precompute=True):
        super().__init__(gl, pairing, num_inputs)
        row = lambda v: np.asarray(v, dtype=np.uint64).reshape(1, -1)
        cat = lambda *parts: np.ascontiguousarray(np.concatenate(parts), dtype=np.uint64)
        # keys made by generate_parameters hold GroupAffine::zero() wherever a variable does not occur in A (the extra SAP
        # variables: r1cs_to_sap.rs:68, :85-91): pk["<query>_inf"] flags them (absent = all finite)
        def flags(q, head_last, tail):
            f = pk.get(q + "_inf")
            if f is None:
                return None
            f = np.asarray(f, dtype=np.uint8)
            f = np.concatenate([f[1:], f[:1]]) if head_last else f
            return np.ascontiguousarray(np.concatenate([f, np.zeros(tail, dtype=np.uint8)]))
        self._upload({
            "a": (self.g1, cat(pk["a_query"][1:], row(pk["a_query"][0]), row(pk["g_gamma_z"])), flags("a_query", True, 1)),
            "b": (self.g2, cat(pk["b_query"][1:], row(pk["b_query"][0]), row(pk["h_gamma_z"])), flags("b_query", True, 1)),
            "c1": (self.g1, cat(pk["c_query_1"], row(pk["g_gamma2_z2"]), row(pk["g_ab_gamma_z"])), flags("c_query_1", False, 2)),
            "c2": (self.g1, cat(pk["c_query_2"][1:], row(pk["c_query_2"][0])), flags("c_query_2", True, 0)),
            "g": (self.g1, cat(pk["g_gamma2_z_t"], row(pk["g_gamma2_z_t"][0])), None),
        }, precompute)

    def create_proof_msms(self, input_assignment, aux_assignment, h, d1, d2, r, h_dev=None, scalars_dev=None):
        """prover.rs:267-352 after the witness map.  input_assignment: num_inputs - 1 rows, aux_assignment: the rest of
        the EXTENDED assignment (aux, then the extra SAP variables), h: its coefficients -- all canonical 12-u64 rows
        (into_repr, :224-252); d1, d2, r: Python integers.  h_dev = (DeviceBuffer, rows): h already on the device as canonical
        scalars.  scalars_dev = (d_s, d_c1, n), with h_dev: the extended assignment already on the device as canonical scalars
        (gh_sap_r1cs_witness_map_dev's d_scalars and d_aux_scalars): d_s holds input || aux in its first n rows and has room for
        two more, d_c1 holds the aux part in its first n - (num_inputs - 1) rows and has room for two more; the tail rows are
        written here, the buffers stay the caller's, and input_assignment / aux_assignment are ignored.
        Returns (A, B, C) as (xy, is_infinity) pairs."""
        gl, ni = self.gl, self.num_inputs
        g1, g2 = self.g1, self.g2
        mod = MODULUS[self.pairing]
        k = self.keys
        n_var = k["a"].n - 2                                 # variables the a / b / c_2 queries pair with: input || aux
        assert k["b"].n - 2 == n_var and k["c2"].n - 1 == n_var and k["c1"].n - 2 == n_var - (ni - 1)
        n_aux = n_var - (ni - 1)
        s_tail = [canon_rows([1]), canon_rows([(r + d1) % mod])]
        c1_tail = [canon_rows([(r * r + 2 * r * d1) % mod, (r + d1) % mod])]
        row_d2 = canon_rows([d2 % mod])
        # ONE device vector  input || aux || 1 || (r + d1) || (r^2 + 2 r d1) || (r + d1):
        #   a / b keys take rows [0, n_var + 2), c_2 rows [0, n_var + 1), c_1 rows [ni - 1, n_var) followed by its own two
        # -- c_1's tail is not contiguous with the aux part, so c_1 gets the aux rows again behind the shared vector
        with contextlib.ExitStack() as stack:
            if scalars_dev is not None:
                d_s, d_c1, n = scalars_dev[0], scalars_dev[1], int(scalars_dev[2])
                if n != n_var or d_s.nbytes < (n + 2) * 96 or d_c1.nbytes < (n_aux + 2) * 96:
                    raise ValueError("the scalar vectors must hold one row per variable of the key's queries, and room for two more each")
                upload_rows(gl, d_s, s_tail, n_var)
                upload_rows(gl, d_c1, c1_tail, n_aux)
            else:
                inp = np.ascontiguousarray(input_assignment, dtype=np.uint64).reshape(-1, 12)
                aux = np.ascontiguousarray(aux_assignment, dtype=np.uint64).reshape(-1, 12)
                assert len(inp) == ni - 1
                aux_used = aux[:n_aux]                               # the reference's zip cuts a longer vector here (variable_base.rs:36)
                pad = np.zeros((n_aux - len(aux_used), 12), dtype=np.uint64)
                d_s = stack.enter_context(gl.DeviceBuffer((n_var + 2) * 96))
                d_c1 = stack.enter_context(gl.DeviceBuffer((n_aux + 2) * 96))
                assert upload_rows(gl, d_s, [inp, aux_used, pad] + s_tail) == n_var + 2
                assert upload_rows(gl, d_c1, [aux_used, pad] + c1_tail) == n_aux + 2
            if h_dev is None:
                h_all = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 12)
                n_h = min(len(h_all), k["g"].n - 1)
                hv = np.concatenate([h_all[:n_h], np.zeros((k["g"].n - 1 - n_h, 12), dtype=np.uint64), row_d2])
                d_h = stack.enter_context(gl.DeviceBuffer(hv.nbytes)).upload(hv)
            else:
                d_h, n_h = h_dev[0], int(h_dev[1])
                assert n_h == k["g"].n - 1                           # the caller left room for one more row behind h
                upload_rows(gl, d_h, [row_d2], n_h)
            g_a, c1, c2, g_acc = gl.msm_batch_dev([(k["a"], d_s, n_var + 2), (k["c1"], d_c1, n_var - (ni - 1) + 2),
                                                   (k["c2"], d_s, n_var + 1), (k["g"], d_h, k["g"].n)])
            g_b = k["b"].msm_dev(d_s, n_var + 2)
        g_c = gl.proj_add(g1, c1, gl.proj_mul(g1, c2, canon_rows([r % mod])[0]))
        g_c = gl.proj_add(g1, g_c, g_acc)
        return gl.proj_to_affine(g1, g_a), gl.proj_to_affine(g2, g_b), gl.proj_to_affine(g1, g_c)

    def prepare_rows(self, circuit_rows, d1, d2):
        """The host side of create_proof up to the device boundary: the host part of the SAP witness map on the evaluated
        constraint rows (Python integers) and its results as Montgomery / canonical limb arrays.  Separate from prove_prepared
        so that a caller (tools/r1cs_bench.py) can time the device stage alone."""
        mod = MODULUS[self.pairing]
        num_inputs, assignment, A, B, C = circuit_rows
        assert num_inputs == self.num_inputs
        full, a, c, log_n = sap_rows_from_r1cs(self.pairing, num_inputs, assignment, A, B, C)
        return {"size": 1 << log_n, "a": mont_rows(a, mod), "c": mont_rows(c, mod), "dd": mont_rows([d1, d2], mod), "scal": canon_rows(full),
                "d1": d1, "d2": d2}

    def prove_prepared(self, prep, r, timing=None):
        """create_proof (prover.rs:201-352) from prepare_rows' arrays: the two vectors to the device, their transforms
        (gh_sap_witness_map_dev), into_repr on the device, the MSM stage.  timing (a dict) receives wall-clock ms per stage."""
        gl, num_inputs = self.gl, self.num_inputs
        size, dd, scal = prep["size"], prep["dd"], prep["scal"]
        log_n = size.bit_length() - 1
        field = FR_FIELD[self.pairing]
        lib = gl.load_library()
        t0 = time.perf_counter()
        with contextlib.ExitStack() as stack:
            bufs = [stack.enter_context(gl.DeviceBuffer(size * 96 + 192)) for _ in range(3)]
            bufs[0].upload(prep["a"])
            bufs[1].upload(prep["c"])
            lib.gh_dev_sync()
            t1 = time.perf_counter()
            gl._check(lib.gh_sap_witness_map_dev(gl.FIELDS[field], bufs[0].ptr, bufs[1].ptr, log_n, gl._ptr(dd[0]), gl._ptr(dd[1]), bufs[2].ptr))
            into_repr(gl, field, bufs[2], size + 1)                                                             # h (:237-252)
            lib.gh_dev_sync()
            t2 = time.perf_counter()
            n_h = self.keys["g"].n - 1
            assert n_h <= size + 1
            proof = self.create_proof_msms(scal[1:num_inputs], scal[num_inputs:], None, prep["d1"], prep["d2"], r, h_dev=(bufs[2], n_h))
            t3 = time.perf_counter()
        if timing is not None:
            timing.update(rows_upload_ms=(t1 - t0) * 1e3, witness_map_ms=(t2 - t1) * 1e3, msm_stage_ms=(t3 - t2) * 1e3)
        return proof

    def create_proof(self, circuit_rows, d1, d2, r):
        """create_proof (prover.rs:201-352) for evaluated constraint rows (groth16.benchmark_circuit_rows form): the host part
        of the SAP witness map, its transforms on the device, into_repr on the device, the MSM stage."""
        return self.prove_prepared(self.prepare_rows(circuit_rows, d1, d2), r)

    def create_proof_r1cs(self, r1cs, assignment, d1, d2, r, timing=None):
        """create_proof (prover.rs:201-352) over resident constraint matrices (r1cs.ResidentR1CS): the assignment goes to the
        device once, as Montgomery rows ((n, 12) uint64, or Python integers that are converted first);
        gh_sap_r1cs_witness_map_dev forms the SAP rows there, runs the witness map and leaves the extended assignment as
        canonical scalars for the five MSMs, so the MSM stage uploads its few tail rows only.  Returns the (A, B, C) of
        create_proof on the same circuit.  timing (a dict) receives wall-clock ms per stage."""
        gl = self.gl
        mod = MODULUS[self.pairing]
        if r1cs.num_inputs != self.num_inputs:
            raise ValueError("the constraint system and the key disagree on the number of inputs")
        z = assignment if isinstance(assignment, np.ndarray) else mont_rows(list(assignment), mod)
        z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 12)
        nv = r1cs.num_variables
        if len(z) != nv:
            raise ValueError("the assignment must have one row per variable")
        info = sap.sap_info(r1cs)
        size, sap_nv = info["size"], info["sap_num_variables"]
        n_aux = sap_nv - (self.num_inputs - 1)
        n_h = self.keys["g"].n - 1
        if n_h > size + 1:
            raise ValueError("the key's g_gamma2_z_t query is longer than h")
        dd = mont_rows([d1, d2], mod)
        lib = gl.load_library()
        t0 = time.perf_counter()
        with contextlib.ExitStack() as stack:
            d_z, d_h, d_s, d_c1 = (stack.enter_context(gl.DeviceBuffer(rows * 96)) for rows in (nv, size + 2, sap_nv + 2, n_aux + 2))
            d_z.upload(z)
            lib.gh_dev_sync()
            t1 = time.perf_counter()
            sap.sap_witness_map_dev(r1cs, d_z, dd, d_h, d_s, d_c1)
            into_repr(gl, FR_FIELD[self.pairing], d_h, size + 1)                                                # h (:237-252)
            lib.gh_dev_sync()
            t2 = time.perf_counter()
            proof = self.create_proof_msms(None, None, None, d1, d2, r, h_dev=(d_h, n_h), scalars_dev=(d_s, d_c1, sap_nv))
            t3 = time.perf_counter()
        if timing is not None:
            timing.update(assignment_upload_ms=(t1 - t0) * 1e3, witness_map_ms=(t2 - t1) * 1e3, msm_stage_ms=(t3 - t2) * 1e3)
        return proof


def sap_instance_map_host(lcs, u, r):
    """The loops of R1CStoSAP::instance_map_with_evaluation (r1cs_to_sap.rs:37-94) on host integers, as in the reference: u, the
    Lagrange coefficients at t over the SAP domain -> (a, c), each with sap_num_variables + 1 entries"""
    num_inputs, num_aux, at, bt, ct = lcs
    n_con = len(at)
    ni1 = num_inputs - 1
    sap_nv = 2 * ni1 + num_aux + n_con                                             # :30-31
    xvo, xco, xvo2 = ni1 + num_aux + 1, 2 * n_con, ni1 + num_aux + n_con           # :32-35
    a, c = [0] * (sap_nv + 1), [0] * (sap_nv + 1)
    for i in range(n_con):                                                         # :40-73
        u0, u1 = u[2 * i], u[2 * i + 1]
        ua, us = (u0 + u1) % r, (u0 - u1) % r
        for cf, ix in at[i]:
            a[ix] = (a[ix] + ua * cf) % r
        for cf, ix in bt[i]:
            a[ix] = (a[ix] + us * cf) % r
        for cf, ix in ct[i]:
            c[ix] = (c[ix] + 4 * u0 * cf) % r
        c[xvo + i] = (c[xvo + i] + ua) % r
    a[0] = (a[0] + u[xco]) % r                                                     # :75-76
    c[0] = (c[0] + u[xco]) % r
    for i in range(1, ni1 + 1):                                                    # :78-94
        uo, ue = u[xco + 2 * i - 1], u[xco + 2 * i]
        a[i] = (a[i] + uo + ue) % r
        a[0] = (a[0] + uo - ue) % r
        c[i] = (c[i] + 4 * uo) % r
        c[xvo2 + i] = (c[xvo2 + i] + uo + ue) % r
    return a, c


def _instance_map_on_device(gl, field, r1cs, shape, tau):
    """the same with u left on the device (gh_lagrange_coefficients_dev) and the three transposed products there
    (gh_sap_instance_map_dev); into_repr on the device as well, so the host only reads limbs -> a, c as integers"""
    num_inputs, num_aux, n_con, log_n = shape
    if (r1cs.num_inputs, r1cs.num_aux, r1cs.num_constraints) != shape[:3] or sap.sap_info(r1cs)["sap_log_n"] != log_n:
        raise ValueError("the resident constraint system is not the one of lcs")
    rows = 2 * (num_inputs - 1) + num_aux + n_con + 1
    with contextlib.ExitStack() as stack:
        d_u = stack.enter_context(gl.DeviceBuffer(96 << log_n))
        outs = [stack.enter_context(gl.DeviceBuffer(rows * 96)) for _ in range(2)]
        gl._check(gl.load_library().gh_lagrange_coefficients_dev(gl.FIELDS[field], log_n, gl._ptr(tau), d_u.ptr))
        sap.sap_instance_map_dev(r1cs, d_u, *outs)
        res = []
        for o in outs:
            into_repr(gl, field, o, rows)
            res.append(ints_from_canon_rows(o.download()[:rows * 12]))
        return tuple(res)


def generate_parameters(gl, pairing, lcs, alpha, beta, gamma, t, g1_xyz, g2_xyz, r1cs=None):
    """generate_parameters (proof-systems/src/gm17/generator.rs:146-335) above the C ABI, for a constraint system given as linear
    combinations (groth16.benchmark_circuit_lcs form); the toxic waste alpha, beta, gamma, the evaluation point t
    (sample_element_outside_domain, :183) and the generators g, h (`rand`, :41-42) are arguments instead of RNG draws.
      * Lagrange coefficients at t on the device (gh_lagrange_coefficients = evaluate_all_lagrange_coefficients, domain.rs:183-219);
      * R1CStoSAP::instance_map_with_evaluation (r1cs_to_sap.rs:14-96): host integers, as in the reference
        (sap_instance_map_host);
      * the FIVE FixedBaseMSM::multi_scalar_mul calls (:222-229 a_query, :245-254 g_gamma2_z_t, :259-270 verifier query ||
        c_query_1, :274-285 c_query_2, :297-302 b_query on h^gamma) with the reference's window rule (:198-213, :290) followed
        by batch_normalization + into_affine (:323-333): gh_fixed_base_msm_affine;
      * the single points (:233-241) by host-side scalar multiplications (gh_proj_mul).
    Returns (pk, info): pk in ResidentGm17Key's form (Montgomery x || y rows + `<query>_inf` flags; GM17's Parameters::write is
    unimplemented upstream, gm17/mod.rs:186-196), info = the SAP evaluations a, c, Z(t) for a check in the exponent.
      * r1cs (an r1cs.ResidentR1CS of the same lcs): the Lagrange coefficients stay on the device
        (gh_lagrange_coefficients_dev) and gh_sap_instance_map_dev takes the place of the host loops -- same pk and info."""
    r = MODULUS[pairing]
    field = FR_FIELD[pairing]
    g1c, g2c = pairing + "_g1", pairing + "_g2"
    num_inputs, num_aux, at, bt, ct = lcs
    n_con = len(at)
    ni1 = num_inputs - 1
    size = domain_size(2 * n_con + 2 * ni1 + 1)                                    # r1cs_to_sap.rs:18-21
    log_n = size.bit_length() - 1
    zt = (pow(t, size, r) - 1) % r
    tau = mont_rows([t], r)[0]
    sap_nv = 2 * ni1 + num_aux + n_con                                             # :30-31
    if r1cs is not None:
        a, c = _instance_map_on_device(gl, field, r1cs, (num_inputs, num_aux, n_con, log_n), tau)
    else:
        u_rows = np.zeros((size, 12), dtype=np.uint64)
        gl._check(gl.load_library().gh_lagrange_coefficients(gl.FIELDS[field], log_n, gl._ptr(tau), gl._ptr(u_rows)))
        a, c = sap_instance_map_host(lcs, ints_from_mont_rows(u_rows, r), r)
    non_zero_a = sum(1 for v in a[:sap_nv] if v)                                   # generator.rs:191-195
    m_raw = size
    FB = gl.FixedBaseMSM
    g_window = FB.get_mul_window_size(num_inputs + non_zero_a + (sap_nv - ni1) + sap_nv + 1 + m_raw + 1)      # :198-211
    h_window = FB.get_mul_window_size(non_zero_a)                                  # :290
    ab = (alpha + beta) % r
    gz = gamma * zt % r
    stats = {"fixed_base_scalars": 0, "fixed_base_calls": 0}

    def rows(table, vals):
        xy, inf = table.multi_scalar_mul_affine(canon_rows(vals), canonical=False)
        stats["fixed_base_scalars"] += len(vals)
        stats["fixed_base_calls"] += 1
        return np.ascontiguousarray(xy, dtype=np.uint64), np.asarray(inf, dtype=np.uint8)

    def point(curve, xyz, k):
        xy, inf = gl.proj_to_affine(curve, gl.proj_mul(curve, xyz, canon_rows([k % r])[0]))
        assert not inf
        return np.asarray(xy, dtype=np.uint64).reshape(-1)

    pk = {}
    tg = FB(g1c, g1_xyz, 753, g_window)
    try:
        pk["a_query"], pk["a_query_inf"] = rows(tg, [v * gamma % r for v in a])
        g2zt = gz * gamma % r
        pw, cur = [], g2zt
        for _ in range(m_raw + 1):
            pw.append(cur)
            cur = cur * t % r
        pk["g_gamma2_z_t"], ginf = rows(tg, pw)
        assert not ginf.any()
        res, rinf = rows(tg, [(cv * gamma + av * ab) % r for av, cv in zip(a, c)])
        pk["verifier_query"], pk["c_query_1"], pk["c_query_1_inf"] = res[:num_inputs], res[num_inputs:], rinf[num_inputs:]
        pk["c_query_2"], pk["c_query_2_inf"] = rows(tg, [v * (2 * gamma * gamma % r) % r * zt % r for v in a])
    finally:
        tg.free()
    h_gamma = gl.proj_mul(g2c, g2_xyz, canon_rows([gamma % r])[0])
    th = FB(g2c, h_gamma, 753, h_window)
    try:
        pk["b_query"], pk["b_query_inf"] = rows(th, a)
    finally:
        th.free()
    pk["g_gamma_z"] = point(g1c, g1_xyz, gz)
    pk["h_gamma_z"] = point(g2c, h_gamma, zt)
    pk["g_ab_gamma_z"] = point(g1c, g1_xyz, ab * gz)
    pk["g_gamma2_z2"] = point(g1c, g1_xyz, gz * gz)
    info = {"num_inputs": num_inputs, "log_n": log_n, "sap": (a, c, zt), "sap_num_variables": sap_nv, "g_window": g_window,
            "h_window": h_window, "non_zero_a": non_zero_a, "fixed_base": stats}
    return pk, info


def verifying_key(gl, pairing, pk, alpha, beta, gamma, g1_xyz, g2_xyz):
    """The VerifyingKey of generate_parameters' `pk` (generator.rs:305-321) for the same toxic waste and generators: the five
    single points h_g2 = h, g_alpha_g1 = alpha g, h_beta_g2 = beta h, g_gamma_g1 = gamma g, h_gamma_g2 = gamma h by host-side
    scalar multiplications (gh_proj_mul) and into_affine, and query = pk["verifier_query"].  Returns a dict of Montgomery limb
    rows (G1 24, G2 24 * deg u64; query: num_inputs x 24) plus "pairing": what gm17_verify.PreparedVerifyingKey.from_key takes.
    As in the reference, proofs of `pk` satisfy the verifier's first equation for gamma = 1 only, the value
    generate_random_parameters fixes (generator.rs:27): the C queries carry gamma c_i + (alpha + beta) a_i for the public inputs
    and for the auxiliary variables alike, and the two differ by (gamma - 1)((alpha + beta) sum a_i x_i + gamma sum c_i x_i)
    over the auxiliary variables."""
    r = MODULUS[pairing]
    g1c, g2c = pairing + "_g1", pairing + "_g2"

    def point(curve, xyz, k):
        xy, inf = gl.proj_to_affine(curve, gl.proj_mul(curve, xyz, canon_rows([k % r])[0]))
        if inf:
            raise ValueError("a point of the verifying key is the point at infinity")
        return np.asarray(xy, dtype=np.uint64).reshape(-1)

    query = np.ascontiguousarray(pk["verifier_query"], dtype=np.uint64).reshape(-1, 24)
    if not query.any(axis=1).all():                                                # GroupAffine::zero() written as zeros: an input no constraint uses
        raise ValueError("a point of the verifying key is the point at infinity")
    return {"pairing": pairing, "h_g2": point(g2c, g2_xyz, 1), "g_alpha_g1": point(g1c, g1_xyz, alpha), "h_beta_g2": point(g2c, g2_xyz, beta),
            "g_gamma_g1": point(g1c, g1_xyz, gamma), "h_gamma_g2": point(g2c, g2_xyz, gamma),
            "query": query}


def proof_bytes(pairing, proof):
    """A || B || C as GroupAffine::write records (GM17's own Proof::write is unimplemented upstream: gm17/mod.rs:59-69)"""
    (a, ai), (b, bi), (c, ci) = proof
    return affine_to_wire(pairing, "g1", a, ai) + affine_to_wire(pairing, "g2", b, bi) + affine_to_wire(pairing, "g1", c, ci)
