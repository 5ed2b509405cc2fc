"""The referee of the polynomial unit on Python integers: for every function the reference's own loop as written
(algebra/src/fft/polynomial/dense.rs, mod.rs, sparse.rs), the closed forms the device kernels compute, checked against those
loops, and cases(): the shapes the host and the GPU tests share."""
import random

MODULUS = {
    "mnt4753_fr": 0x1c4c62d92c41110229022eee2cdadb7f997505b8fafed5eb7e8f96c97d87307fdb925e8a0ed8d99d124d9a15af79db26c5c28c859a99b3eebca9429212636b9dff97634993aa4d6c381bc3f0057974ea099170fa13a4fd90776e240000001,
    "mnt6753_fr": 0x1c4c62d92c41110229022eee2cdadb7f997505b8fafed5eb7e8f96c97d87307fdb925e8a0ed8d99d124d9a15af79db117e776f218059db80f0da5cb537e38685acce9767254a4638810719ac425f0e39d54522cdd119f5e9063de245e8001,
}
TWO_ADICITY = {"mnt4753_fr": 30, "mnt6753_fr": 15}
FIELDS = ["mnt4753_fr", "mnt6753_fr"]


# ---------------------------------------------------------------------------------------------------- the reference's loops
def trim(c):
    """from_coefficients_vec (dense.rs:64-73)"""
    c = list(c)
    while c and c[-1] == 0:
        c.pop()
    return c


def evaluate(c, z, p):
    """dense.rs:86-103: the powers of the point, then the sum of the products"""
    c = trim(c)
    if not c:
        return 0
    powers, cur = [1], z % p
    for _ in range(len(c) - 1):
        powers.append(cur)
        cur = cur * z % p
    acc = 0
    for pw, co in zip(powers, c):
        acc = (acc + pw * co) % p
    return acc


def naive_mul(a, b, p):
    """dense.rs:106-118"""
    a, b = trim(a), trim(b)
    if not a or not b:
        return []
    res = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            res[i + j] = (res[i + j] + x * y) % p
    return trim(res)


def divide_with_q_and_r(a, divisor_terms, p):
    """polynomial/mod.rs:105-132; the divisor as iter_with_index gives it: [(index, coefficient)], the leading term last"""
    a = trim(a)
    divisor_terms = [(i, c % p) for i, c in divisor_terms if c % p]
    if not a:
        return [], []
    if not divisor_terms:
        raise ZeroDivisionError("Dividing by zero polynomial")
    ddeg = divisor_terms[-1][0]
    if len(a) - 1 < ddeg:
        return [], a
    quotient = [0] * (len(a) - 1 - ddeg + 1)
    rem = list(a)
    lead_inv = pow(divisor_terms[-1][1], -1, p)
    while rem and len(rem) - 1 >= ddeg:
        cur_q = rem[-1] * lead_inv % p
        cur_deg = len(rem) - 1 - ddeg
        quotient[cur_deg] = cur_q
        for i, dc in divisor_terms:
            rem[cur_deg + i] = (rem[cur_deg + i] - cur_q * dc) % p
        while rem and rem[-1] == 0:
            rem.pop()
    return trim(quotient), rem


def vanishing_terms(N, p):
    """domain.rs:222-225"""
    return [(0, p - 1), (N, 1)]


def mul_by_vanishing(c, N, p):
    """dense.rs:134-139"""
    shifted = [0] * N + list(c)
    for i, x in enumerate(c):
        shifted[i] = (shifted[i] - x) % p
    return trim(shifted)


def sparse_evaluate(terms, z, p):
    """sparse.rs evaluate: the sum of coeff * point.pow(degree)"""
    return sum(c * pow(z, e, p) for e, c in terms) % p


def add_ref(a, b, p, sign=1, f=1):
    """Add / Sub / AddAssign((f, b)) of trimmed operands with the reference's lengths (dense.rs:150-328)"""
    if not trim(a):
        return [sign * f * x % p for x in b]
    if not trim(b):
        return list(a)
    res = [((a[i] if i < len(a) else 0) + sign * f * (b[i] if i < len(b) else 0)) % p for i in range(max(len(a), len(b)))]
    return res if len(a) >= len(b) else trim(res)


# ---------------------------------------------------------------------------------------------------- the kernels' closed forms
def divide_by_vanishing_closed(c, N, p):
    """q = sum_k x^(kN) sum_(j > k) P_j, r = sum_k P_k over the chunks P_k of N coefficients: (q, r) in full, max(n, N) - N and
    N rows"""
    n = len(c)
    q = [sum(c[i + N::N]) % p for i in range(max(n, N) - N)]
    r = [sum(c[i::N]) % p for i in range(N)]
    return q, r


def divide_by_linear_closed(c, z, p):
    """q_(n - 2) = c_(n - 1), q_(i - 1) = c_i + z q_i, rem = c_0 + z q_0: (q in full, max(n, 1) - 1 rows; rem)"""
    acc, out = 0, []
    for x in reversed(c):
        acc = (acc * z + x) % p
        out.append(acc)
    out.reverse()
    return out[1:], (out[0] if out else 0)


def fold_closed(c, G, z, p):
    """one level of the Horner fold: s_g = sum_j c_(g + j G) (z^G)^j; evaluate(s, z) = evaluate(c, z)"""
    w = pow(z, G, p)
    return [evaluate(c[g::G], w, p) for g in range(G)]


# ---------------------------------------------------------------------------------------------------- shapes and data
def coeffs(field, n, seed, kind="random"):
    """n coefficients with 0 and r - 1 among them; kind: random, zero (all zero), zero_top (zero top rows)"""
    p = MODULUS[field]
    rng = random.Random("%s/%d/%s" % (field, n, seed))
    if kind == "zero":
        return [0] * n
    c = [rng.randrange(p) for _ in range(n)]
    if n >= 3:
        c[rng.randrange(n - 1)] = 0
        c[rng.randrange(n - 1)] = p - 1
    if n:
        c[-1] = c[-1] or 1
    if kind == "zero_top":
        for i in range(n - (n + 2) // 3, n):
            c[i] = 0
    return c


def points(field):
    """0, 1, r - 1, an element of order 64, two random"""
    p = MODULUS[field]
    rng = random.Random("points/" + field)
    return [0, 1, p - 1, pow(17, (p - 1) >> 6, p), rng.randrange(p), rng.randrange(p)]


def cases():
    return {
        "tuning": (4, 4, 4),
        "evaluate_tuned": [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 300, 1000],
        "evaluate_default": [31, 32, 33, 1023, 1025, 32769],
        "evaluate_k": [1, 3, 5],
        "trimmed_len": [0, 1, 255, 256, 257, 5000],
        "axpy": [0, 1, 5, 257],
        "vanishing_log_n": [0, 1, 2, 6],
        "vanishing_n": lambda N: sorted({0, 1, max(N - 1, 0), N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 3 * N + 5}),
        "vanishing_two_pass": (0, 5000),               # N = 1 at seg_max = 4
        "vanishing_large": (15, (1 << 16) + 3),
        "linear_tuned": [0, 1, 2, 3, 4, 5, 16, 17, 300, 1000],
        "linear_default": [32769],
        "mul": [(0, 3), (1, 1), (1, 5), (3, 4), (4, 4), (5, 4), (255, 257), (256, 256), (257, 256)],
        "evals_div": [1, 31, 32, 33, 100],
        "domain_log_n": [0, 1, 6, 10],
        "plan_n": list(range(71)) + [300, 1000, 1023, 1025, 5000, 32769, (1 << 16) + 3, 1 << 24],
    }


def check_closed_forms(field):
    """the closed forms against the reference's loops at the test shapes (the small ones: the loops are quadratic)"""
    p = MODULUS[field]
    cs = cases()
    for n in [n for n in cs["linear_tuned"] if n <= 300]:
        c = coeffs(field, n, "lin")
        for z in points(field)[:5]:
            q, rem = divide_by_linear_closed(c, z, p)
            rq, rr = divide_with_q_and_r(c, [(0, -z % p), (1, 1)], p)
            assert trim(q) == rq and ([rem] if rem else []) == rr, (n, z)
            assert rem == evaluate(c, z, p)
    for log_n in cs["vanishing_log_n"]:
        N = 1 << log_n
        for n in cs["vanishing_n"](N):
            for kind in ("random", "zero_top"):
                c = coeffs(field, n, "van", kind)
                q, r = divide_by_vanishing_closed(c, N, p)
                assert (trim(q), trim(r)) == divide_with_q_and_r(c, vanishing_terms(N, p), p), (N, n)
                assert mul_by_vanishing(c, N, p) == naive_mul(c, [p - 1] + [0] * (N - 1) + [1], p)
    for n in (5, 17, 65):
        c = coeffs(field, n, "fold")
        for G in (1, 2, 5, 17):
            for z in points(field):
                assert evaluate(fold_closed(c, G, z, p), z, p) == evaluate(c, z, p)
