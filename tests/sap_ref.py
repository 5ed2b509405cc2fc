"""Referee of the device's R1CS -> SAP maps: proof-systems/src/gm17/r1cs_to_sap.rs restated on Python integers from the
constraint system's linear combinations and an assignment.  A constraint system is r1cs_ref's (num_inputs, num_aux, at, bt,
ct).  Test infrastructure: nothing here is shipped, and nothing here calls the code under test."""
import r1cs_ref


def domain_size(num_constraints, num_inputs):
    """EvaluationDomain::new(2 * num_constraints + 2 * (num_inputs - 1) + 1).size()  (:18-21, :151-155)"""
    size = 1
    while size < 2 * num_constraints + 2 * (num_inputs - 1) + 1:
        size <<= 1
    return size


def sap_num_variables(lcs):
    """:30-31"""
    num_inputs, num_aux, at = lcs[:3]
    return 2 * (num_inputs - 1) + num_aux + len(at)


def rows(lcs, assignment, r):
    """witness_map up to the transforms (:99-189, :206-232): -> (full_input_assignment, a, c), a and c of domain size"""
    num_inputs, num_aux, at, bt, ct = lcs
    num_constraints = len(at)
    full = list(assignment)
    assert len(full) == num_inputs + num_aux
    az = [r1cs_ref.evaluate_constraint(row, full, r) for row in at]
    bz = [r1cs_ref.evaluate_constraint(row, full, r) for row in bt]
    cz = [r1cs_ref.evaluate_constraint(row, full, r) for row in ct]
    extra_var_offset = num_inputs + num_aux
    for i in range(num_constraints):                       # :125-141
        full.append(pow(az[i] - bz[i], 2, r))
    for i in range(1, num_inputs):                         # :143-149
        full.append(pow(full[i] - 1, 2, r))
    size = domain_size(num_constraints, num_inputs)
    extra_constr_offset = 2 * num_constraints
    extra_var_offset2 = num_inputs + num_aux + num_constraints - 1
    a, c = [0] * size, [0] * size
    for i in range(num_constraints):                       # :159-166, :207-216
        a[2 * i] = (az[i] + bz[i]) % r
        a[2 * i + 1] = (az[i] - bz[i]) % r
        c[2 * i] = (4 * cz[i] + full[extra_var_offset + i]) % r
        c[2 * i + 1] = full[extra_var_offset + i]
    a[extra_constr_offset] = 1                             # :168, :218
    c[extra_constr_offset] = 1
    for i in range(1, num_inputs):                         # :170-189, :220-232
        a[extra_constr_offset + 2 * i - 1] = (full[i] + 1) % r
        a[extra_constr_offset + 2 * i] = (full[i] - 1) % r
        c[extra_constr_offset + 2 * i - 1] = (4 * full[i] + full[extra_var_offset2 + i]) % r
        c[extra_constr_offset + 2 * i] = full[extra_var_offset2 + i]
    return full, a, c


def instance_map(lcs, u, r):
    """instance_map_with_evaluation after the Lagrange coefficients (:30-94): u has domain size -> (a, c), each with
    sap_num_variables + 1 entries"""
    num_inputs, num_aux, at, bt, ct = lcs
    num_constraints = len(at)
    nv = num_inputs + num_aux
    n = sap_num_variables(lcs) + 1
    a, c = [0] * n, [0] * n
    p = [(u[2 * i] + u[2 * i + 1]) % r for i in range(num_constraints)]
    m = [(u[2 * i] - u[2 * i + 1]) % r for i in range(num_constraints)]
    q = [u[2 * i] for i in range(num_constraints)]
    at_p = r1cs_ref.matvec(at, p, r, num_out=nv, transpose=True)
    bt_m = r1cs_ref.matvec(bt, m, r, num_out=nv, transpose=True)
    ct_q = r1cs_ref.matvec(ct, q, r, num_out=nv, transpose=True)
    for j in range(nv):
        a[j] = (at_p[j] + bt_m[j]) % r
        c[j] = 4 * ct_q[j] % r
    for i in range(num_constraints):
        c[nv + i] = p[i]
    off = 2 * num_constraints
    a[0] = (a[0] + u[off]) % r
    c[0] = (c[0] + u[off]) % r
    for i in range(1, num_inputs):
        odd, even = u[off + 2 * i - 1], u[off + 2 * i]
        a[0] = (a[0] + odd - even) % r
        a[i] = (a[i] + odd + even) % r
        c[i] = (c[i] + 4 * odd) % r
        c[nv + num_constraints - 1 + i] = (odd + even) % r
    return a, c


def cases(r):
    """(name, lcs) of the shapes the host lanes and the device are run on: the domain at 63 and 65 (one padding row, then 63);
    the wave and block edges of one lane per constraint; no input rows; input rows beyond one block; the hand-built system of
    the R1CS tests with its empty rows and long column"""
    out = [("domain_%d" % (2 * nc + 5), r1cs_ref.random_system(nc, 12, r, seed=40 + nc, max_terms=9, num_inputs=3)) for nc in (29, 30)]
    out += [("edges_%d" % nc, r1cs_ref.random_system(nc, 9, r, seed=nc)) for nc in (1, 63, 64, 65, 128, 129)]
    out.append(("one_input", r1cs_ref.random_system(20, 9, r, seed=5, num_inputs=1)))
    out.append(("inputs_130", r1cs_ref.random_system(11, 140, r, seed=6, num_inputs=130)))
    out.append(("hand_built", r1cs_ref.hand_built_system(r)))
    return out


def satisfying_system(nc, nv, r, seed, num_inputs=2, max_terms=3):
    """a random system made satisfiable for a random assignment: A and B as r1cs_ref.random_system draws them, and every row
    of C one term on an aux variable of its own choosing a coefficient that makes <A_i, z> <B_i, z> = <C_i, z>
    -> (lcs, assignment)"""
    import random
    rng = random.Random(seed)
    num_inputs, num_aux, at, bt, _ = r1cs_ref.random_system(nc, nv, r, seed, max_terms=max_terms, num_inputs=num_inputs)
    z = [1] + [rng.randrange(1, r) for _ in range(nv - 1)]
    ct = []
    for i in range(nc):
        want = r1cs_ref.evaluate_constraint(at[i], z, r) * r1cs_ref.evaluate_constraint(bt[i], z, r) % r
        ix = rng.randrange(nv)
        ct.append([(want * pow(z[ix], -1, r) % r, ix)])
    return (num_inputs, num_aux, at, bt, ct), z
