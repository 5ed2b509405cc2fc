"""Referee of the device's sparse R1CS products: proof-systems/src/groth16/r1cs_to_qap.rs restated on Python integers,
statement by statement.  A constraint system is (num_inputs, num_aux, at, bt, ct): rows of (coefficient, index) where the
index is already the reference's `match index { Input(i) => i, Aux(i) => num_inputs + i }`.  Test infrastructure: nothing
here is shipped, and nothing here calls the code under test."""


def domain_size(num_constraints, num_inputs):
    """EvaluationDomain::new(num_constraints + (num_inputs - 1) + 1).size()  (:100-103, :18-21)"""
    size = 1
    while size < num_constraints + (num_inputs - 1) + 1:
        size <<= 1
    return size


def evaluate_constraint(terms, assignment, r):
    """:78-92"""
    acc = 0
    for coeff, index in terms:
        val = assignment[index]
        acc = (acc + val * coeff) % r
    return acc


def evaluate(lcs, assignment, r):
    """witness_map up to the transforms (:94-119, :141-151): -> (a, b, c), each of domain size"""
    num_inputs, num_aux, at, bt, ct = lcs
    num_constraints = len(at)
    full = list(assignment)
    assert len(full) == num_inputs + num_aux
    size = domain_size(num_constraints, num_inputs)
    a, b = [0] * size, [0] * size
    for i in range(num_constraints):                       # :107-115
        a[i] = evaluate_constraint(at[i], full, r)
        b[i] = evaluate_constraint(bt[i], full, r)
    for i in range(num_inputs):                            # :117-119
        a[num_constraints + i] = full[i] if i > 0 else 1
    c = [0] * size                                         # :141-151
    for i in range(num_constraints):
        c[i] = evaluate_constraint(ct[i], full, r)
    return a, b, c


def instance_map(lcs, u, r):
    """instance_map_with_evaluation after the Lagrange coefficients (:30-65): u has domain size -> (a, b, c), each with
    (num_inputs - 1) + num_aux + 1 entries"""
    num_inputs, num_aux, at, bt, ct = lcs
    num_constraints = len(at)
    qap_num_variables = (num_inputs - 1) + num_aux
    a = [0] * (qap_num_variables + 1)
    b = [0] * (qap_num_variables + 1)
    c = [0] * (qap_num_variables + 1)
    for i in range(num_inputs):                            # :36-38
        a[i] = u[num_constraints + i]
    for i in range(num_constraints):                       # :40-65
        for coeff, index in at[i]:
            a[index] = (a[index] + u[i] * coeff) % r
        for coeff, index in bt[i]:
            b[index] = (b[index] + u[i] * coeff) % r
        for coeff, index in ct[i]:
            c[index] = (c[index] + u[i] * coeff) % r
    return a, b, c


def matvec(rows, x, r, num_out=None, transpose=False):
    """y = M x for M given as rows of (coefficient, index); with transpose y = M^T x over num_out entries"""
    if not transpose:
        return [evaluate_constraint(row, x, r) for row in rows]
    y = [0] * num_out
    for i, row in enumerate(rows):
        for coeff, index in row:
            y[index] = (y[index] + x[i] * coeff) % r
    return y


# ---- the cases the host executor and the device are run on
def hand_built_system(r, seed=7):
    """130 constraints over 70 variables (3 inputs) with, in every one of A, B, C: empty rows; an unused variable (69); rows of
    1, 4, 5, 16, 17 and 65 terms (at a segment length of 4 the last takes three levels); variable 2 in every non-empty row of A
    (a long column); a repeated index inside a row; the coefficients 0, 1, r - 1, 2, r - 2 and random full-width values mixed
    within one row, and so within one wave.  -> (num_inputs, num_aux, at, bt, ct)"""
    import random
    rng = random.Random(seed)
    nv, nc = 70, 130
    special = [0, 1, r - 1, 2, r - 2]

    def coeff(k):
        return special[k % 5] if k % 3 else rng.randrange(r)

    def matrix(shift, long_column):
        rows = []
        lengths = {0: 1, 1: 4, 2: 5, 3: 16, 4: 17, 5: 65, 70: 17, 129: 5}
        for i in range(nc):
            t = lengths.get(i, 0 if i % 7 == 6 else 1 + (i * 5 + shift) % 6)
            row = [(coeff(i + j + shift), (i * 3 + j * 7 + shift) % 69) for j in range(t)]     # never variable 69
            if t >= 2:
                row[1] = (row[1][0], row[0][1])                                                # a repeated index, both count
            if long_column and t:
                row[-1] = (coeff(i) or 1, 2)
            rows.append(row)
        return rows
    return 3, nv - 3, matrix(0, True), matrix(11, False), matrix(23, False)


def hand_built_vector(n, r, seed=3):
    """0, 1 and r - 1 among random values"""
    import random
    rng = random.Random(seed)
    x = [rng.randrange(r) for _ in range(n)]
    for k, v in ((0, 1), (1, 0), (n // 2, r - 1), (n - 1, 1), (n - 2, 0)):
        if 0 <= k < n:
            x[k] = v
    return x


def random_system(nc, nv, r, seed, max_terms=3, num_inputs=2):
    """nc constraints of 0 .. max_terms terms with mostly +-1 and a few general coefficients"""
    import random
    rng = random.Random(seed)

    def matrix():
        rows = []
        for _ in range(nc):
            rows.append([(rng.choice([1, 1, 1, r - 1, 3, rng.randrange(r)]), rng.randrange(nv)) for _ in range(rng.randrange(max_terms + 1))])
        return rows
    return num_inputs, nv - num_inputs, matrix(), matrix(), matrix()
