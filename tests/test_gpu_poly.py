"""The polynomial unit on the device (include/ginger_hip_poly.h, ginger-lib_amd/poly.py) against the referee on Python integers
(tests/poly_ref.py).  Every comparison is exact and covers every row; an output buffer holds 0xFF before a call and one row more
than the call may write, which must still hold 0xFF after it.  The shapes are poly_ref.cases(): the smallest at which the
kernels can still go wrong, at tuning (4, 4, 4) so that small inputs reach the upper levels of the fold and the scans, and the
sizes around a run at the defaults."""
import ctypes
import importlib

import numpy as np
import pytest

import poly_ref as ref

pytestmark = pytest.mark.gpu

GH_E_BAD_ARG, GH_E_UNSUPPORTED = -1, -2
FIELD_ID = {"mnt4753_fr": 0, "mnt6753_fr": 1}
CASES = ref.cases()
FF = 0xFFFFFFFFFFFFFFFF
_memo = {}


@pytest.fixture(scope="module")
def poly(gpu):
    return importlib.import_module("ginger_lib_amd.poly")


@pytest.fixture
def tuned(poly):
    poly.set_tuning(*CASES["tuning"])
    yield
    poly.set_tuning(0, 0, 0)


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def mont(vals, p):
    R = (1 << 768) % p
    raw = b"".join((v % p * R % p).to_bytes(96, "little") for v in vals)
    return np.frombuffer(raw + b"\0" * (0 if vals else 96), dtype=np.uint64).reshape(-1, 12).copy()


def ints(rows, n, p):
    rinv = pow(1 << 768, -1, p)
    raw = np.ascontiguousarray(rows, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[96 * i:96 * i + 96], "little") * rinv % p for i in range(n)]


class Dev:
    """an input vector on the device, or an output of n rows and a guard row, all 0xFF"""

    def __init__(self, gpu, vals=None, p=None, rows=None):
        self.n = len(vals) if vals is not None else rows
        self.buf = gpu.DeviceBuffer((self.n + 1) * 96)
        host = np.full((self.n + 1, 12), FF, dtype=np.uint64)
        if vals:
            host[:self.n] = mont(vals, p)
        self.buf.upload(host)
        self.ptr = self.buf.ptr

    def rows(self):
        return self.buf.download().reshape(-1, 12)

    def ints(self, p, n=None):
        """the first n rows (all of them by default); the guard row, and every row from n on, still holds 0xFF"""
        n = self.n if n is None else n
        r = self.rows()
        assert (r[n:] == FF).all(), "rows beyond the output were written"
        return ints(r[:n], n, p)

    def free(self):
        self.buf.free()


def data(field, n, seed, kind="random"):
    return memo(("c", field, n, seed, kind), lambda: ref.coeffs(field, n, seed, kind))


# ---------------------------------------------------------------------------------------------------- evaluate
def _evaluate_cases(gpu, poly, field, sizes):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    pts = ref.points(field)
    for n in sizes:
        for kind in ("random", "zero", "zero_top"):
            c = data(field, n, "ev", kind)
            want = memo(("ev", field, n, kind), lambda: [ref.evaluate(c, z, p) for z in pts])
            d = Dev(gpu, c, p)
            for k, first in ((1, 3), (3, 3), (5, 0)):           # the element of order 64 alone, the last three, the first five
                out = np.full((k, 12), FF, dtype=np.uint64)
                assert lib.gh_poly_evaluate_dev(f, d.ptr, n, P(mont(pts[first:first + k], p)), k, P(out)) == 0, lib.gh_last_error()
                assert ints(out, k, p) == want[first:first + k], (field, n, kind, k)
            d.free()
    c = data(field, sizes[-1], "ev")
    out = np.full((2, 12), FF, dtype=np.uint64)
    assert lib.gh_poly_evaluate(f, P(mont(c, p)), len(c), P(mont(pts[4:], p)), 2, P(out)) == 0       # the host-buffer form
    assert ints(out, 2, p) == [ref.evaluate(c, z, p) for z in pts[4:]]


@pytest.mark.parametrize("field", ref.FIELDS)
def test_evaluate_through_every_level(gpu, poly, tuned, field):
    _evaluate_cases(gpu, poly, field, CASES["evaluate_tuned"])


@pytest.mark.parametrize("field", ref.FIELDS)
def test_evaluate_at_the_default_run_length(gpu, poly, field):
    _evaluate_cases(gpu, poly, field, CASES["evaluate_default"])


# ---------------------------------------------------------------------------------------------------- trimmed_len, elementwise
@pytest.mark.parametrize("field", ref.FIELDS)
def test_trimmed_len(gpu, poly, field):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    for n in CASES["trimmed_len"]:
        for last in sorted({-1, 0, n - 1, 255, 256, 2047, 2048}):
            if last >= n:
                continue
            c = [0] * n
            if last >= 0:
                c[0], c[last] = 5, p - 1
            d = Dev(gpu, c, p)
            out = ctypes.c_size_t(77)
            assert lib.gh_poly_trimmed_len_dev(f, d.ptr, n, ctypes.byref(out)) == 0
            assert out.value == len(ref.trim(c)), (n, last)
            d.free()


@pytest.mark.parametrize("field", ref.FIELDS)
def test_add_sub_add_scaled_neg(gpu, poly, field):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    scale = ref.points(field)[4]
    s12 = mont([scale], p)
    for na in CASES["axpy"]:
        for nb in CASES["axpy"]:
            a, b = data(field, na, "a"), data(field, nb, "b", "zero_top" if nb == 5 else "random")
            rows = max(na, nb)
            pa, pb = a + [0] * (rows - na), b + [0] * (rows - nb)
            da, db = Dev(gpu, a, p), Dev(gpu, b, p)
            for fn, want in (("gh_poly_add_dev", [(x + y) % p for x, y in zip(pa, pb)]), ("gh_poly_sub_dev", [(x - y) % p for x, y in zip(pa, pb)]),
                             ("gh_poly_add_scaled_dev", [(x + scale * y) % p for x, y in zip(pa, pb)])):
                out = Dev(gpu, rows=rows)
                extra = (P(s12),) if "scaled" in fn else ()
                assert getattr(lib, fn)(f, da.ptr, na, db.ptr, nb, *extra, out.ptr) == 0, lib.gh_last_error()
                assert out.ints(p) == want, (fn, na, nb)
                out.free()
            da.free()
            db.free()
        out = Dev(gpu, rows=na)
        da = Dev(gpu, a, p)
        assert lib.gh_poly_neg_dev(f, da.ptr, na, out.ptr) == 0
        assert out.ints(p) == [-x % p for x in a]
        out.free()
        da.free()


# ---------------------------------------------------------------------------------------------------- the vanishing polynomial
def _vanishing_case(gpu, poly, field, log_n, n, kinds=("random", "zero_top")):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    N = 1 << log_n
    for kind in kinds:
        c = data(field, n, "van", kind)
        d, prod = Dev(gpu, c, p), Dev(gpu, rows=n + N)
        assert lib.gh_poly_mul_by_vanishing_dev(f, d.ptr, n, log_n, prod.ptr) == 0, lib.gh_last_error()
        got = prod.ints(p)
        assert ref.trim(got) == ref.mul_by_vanishing(c, N, p), (N, n)
        q, r = Dev(gpu, rows=max(n, N) - N), Dev(gpu, rows=N)
        assert lib.gh_poly_divide_by_vanishing_dev(f, d.ptr, n, log_n, q.ptr, r.ptr) == 0, lib.gh_last_error()
        assert (q.ints(p), r.ints(p)) == ref.divide_by_vanishing_closed(c, N, p), (N, n)
        rr = data(field, N, "rem")                              # divide(mul_by_vanishing(p) + r) = (p, r)
        full = Dev(gpu, [(got[i] + (rr[i] if i < N else 0)) % p for i in range(n + N)], p)
        q2, r2 = Dev(gpu, rows=n), Dev(gpu, rows=N)
        assert lib.gh_poly_divide_by_vanishing_dev(f, full.ptr, n + N, log_n, q2.ptr, r2.ptr) == 0
        assert (q2.ints(p), r2.ints(p)) == (c, rr), (N, n)
        for x in (d, prod, q, r, full, q2, r2):
            x.free()


@pytest.mark.parametrize("field", ref.FIELDS)
def test_vanishing_small_domains(gpu, poly, tuned, field):
    for log_n in CASES["vanishing_log_n"]:
        for n in CASES["vanishing_n"](1 << log_n):
            _vanishing_case(gpu, poly, field, log_n, n)


@pytest.mark.parametrize("field", ref.FIELDS)
def test_vanishing_two_pass_form(gpu, poly, tuned, field):
    """N = 1, n = 5000 at seg_max = 4: six levels of segment sums, no lane with more than four additions"""
    _vanishing_case(gpu, poly, field, *CASES["vanishing_two_pass"], kinds=("random",))


@pytest.mark.parametrize("field", ref.FIELDS)
def test_vanishing_large_domain(gpu, poly, field):
    log_n, n = CASES["vanishing_large"]
    if field == "mnt6753_fr":                                   # no domain above 2^14 there
        log_n, n = 14, (1 << 15) + 3
    _vanishing_case(gpu, poly, field, log_n, n, kinds=("random",))
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    c = data(field, 300, "van")
    q, r = np.full((300 - 64, 12), FF, dtype=np.uint64), np.full((64, 12), FF, dtype=np.uint64)
    assert lib.gh_poly_divide_by_vanishing(f, P(mont(c, p)), 300, 6, P(q), P(r)) == 0            # the host-buffer form
    assert (ints(q, 236, p), ints(r, 64, p)) == ref.divide_by_vanishing_closed(c, 64, p)


# ---------------------------------------------------------------------------------------------------- division by x - z
def _linear_cases(gpu, poly, field, sizes):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    pts = ref.points(field)
    for n in sizes:
        c = data(field, n, "lin")
        jobs = [(z, c) for z in (pts[0], pts[1], pts[2], pts[4])]
        if n >= 2:                                              # a root planted by construction: p = q0 (x - root)
            root, q0 = pts[5], data(field, n - 1, "root")
            jobs.append((root, [((q0[i - 1] if i else 0) - root * (q0[i] if i < n - 1 else 0)) % p for i in range(n)]))
        for z, cc in jobs:
            d, q = Dev(gpu, cc, p), Dev(gpu, rows=max(n, 1) - 1)
            rem = np.full((1, 12), FF, dtype=np.uint64)
            assert lib.gh_poly_divide_by_linear_dev(f, d.ptr, n, P(mont([z], p)), q.ptr, P(rem)) == 0, lib.gh_last_error()
            wq, wr = ref.divide_by_linear_closed(cc, z, p)
            assert q.ints(p) == wq and ints(rem, 1, p) == [wr], (field, n, z)
            if cc is not c:
                assert wr == 0 and wq == q0
            d.free()
            q.free()
    c = data(field, sizes[-1], "lin")
    q, rem = np.full((len(c) - 1, 12), FF, dtype=np.uint64), np.full((1, 12), FF, dtype=np.uint64)
    assert lib.gh_poly_divide_by_linear(f, P(mont(c, p)), len(c), P(mont([pts[4]], p)), P(q), P(rem)) == 0      # the host-buffer form
    wq, wr = ref.divide_by_linear_closed(c, pts[4], p)
    assert ints(q, len(wq), p) == wq and ints(rem, 1, p) == [wr]


@pytest.mark.parametrize("field", ref.FIELDS)
def test_divide_by_linear_through_every_level(gpu, poly, tuned, field):
    _linear_cases(gpu, poly, field, CASES["linear_tuned"])


@pytest.mark.parametrize("field", ref.FIELDS)
def test_divide_by_linear_at_the_default_run_length(gpu, poly, field):
    _linear_cases(gpu, poly, field, CASES["linear_default"])


# ---------------------------------------------------------------------------------------------------- Mul
@pytest.mark.parametrize("field", ref.FIELDS)
def test_mul_against_naive_mul(gpu, poly, field):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    for na, nb in CASES["mul"]:
        for kind in ("random", "zero_top"):
            a, b = data(field, na, "ma"), data(field, nb, "mb", kind)
            want = memo(("mul", field, na, nb, kind), lambda: ref.naive_mul(a, b, p))
            cap = 1 << max(0, na + nb - 1).bit_length()
            da, db, out = Dev(gpu, a, p), Dev(gpu, b, p), Dev(gpu, rows=cap)
            n_out = ctypes.c_size_t(77)
            assert lib.gh_poly_mul_dev(f, da.ptr, na, db.ptr, nb, out.ptr, cap, ctypes.byref(n_out)) == 0, lib.gh_last_error()
            assert n_out.value == len(want), (na, nb, kind)
            if want:
                got = out.ints(p)
                assert got[:len(want)] == want and not any(got[len(want):]), (na, nb, kind)
                n_small = ctypes.c_size_t(77)
                assert lib.gh_poly_mul_dev(f, da.ptr, na, db.ptr, nb, out.ptr, cap - 1, ctypes.byref(n_small)) == GH_E_BAD_ARG
                assert out.ints(p) == got
            else:
                out.ints(p, 0)                                  # untouched
            for x in (da, db, out):
                x.free()
    a, b = data(field, 5, "ma"), data(field, 4, "mb")
    out = np.full((16, 12), FF, dtype=np.uint64)
    n_out = ctypes.c_size_t(77)
    assert lib.gh_poly_mul(f, P(mont(a, p)), 5, P(mont(b, p)), 4, P(out), 16, ctypes.byref(n_out)) == 0     # the host-buffer form
    assert n_out.value == 8 and ints(out, 8, p) == ref.naive_mul(a, b, p) and (out[8:] == FF).all()


def test_mul_beyond_the_two_adicity_is_unsupported(gpu, poly):
    field = "mnt6753_fr"
    p, lib = ref.MODULUS[field], poly._lib()
    na, nb = (1 << 14) + 1, 1 << 14
    da, db, out = Dev(gpu, [1] * na, p), Dev(gpu, [2] * nb, p), Dev(gpu, rows=8)
    n_out = ctypes.c_size_t(77)
    assert lib.gh_poly_mul_dev(1, da.ptr, na, db.ptr, nb, out.ptr, 1 << 16, ctypes.byref(n_out)) == GH_E_UNSUPPORTED
    out.ints(p, 0)
    a, b = poly.DensePolynomial.from_coefficients(field, [1] * na), poly.DensePolynomial.from_coefficients(field, [2] * nb)
    with pytest.raises(poly.GingerHipError):
        a * b
    for x in (da, db, out):
        x.free()


# ---------------------------------------------------------------------------------------------------- evaluations, domains
@pytest.mark.parametrize("field", ref.FIELDS)
def test_evals_div(gpu, poly, field):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    for n in CASES["evals_div"]:
        a = data(field, n, "da")
        b = [x or 3 for x in data(field, n, "db")]
        da, db = Dev(gpu, a, p), Dev(gpu, b, p)
        zeros = ctypes.c_size_t(77)
        assert lib.gh_evals_div_dev(f, da.ptr, db.ptr, n, ctypes.byref(zeros)) == 0, lib.gh_last_error()
        assert zeros.value == 0 and da.ints(p) == [x * pow(y, -1, p) % p for x, y in zip(a, b)], n
        assert db.ints(p) == b
        b[n // 2] = 0
        da2, db2 = Dev(gpu, a, p), Dev(gpu, b, p)
        assert lib.gh_evals_div_dev(f, da2.ptr, db2.ptr, n, ctypes.byref(zeros)) == 0
        assert zeros.value == 1 and da2.ints(p) == a
        for x in (da, db, da2, db2):
            x.free()
    dom = poly.EvaluationDomain(field, 32)
    ea, eb = poly.Evaluations.from_ints(data(field, 32, "da"), dom), poly.Evaluations.from_ints([0] + [1] * 31, dom)
    with pytest.raises(ZeroDivisionError):
        ea / eb
    assert ea.evals() == data(field, 32, "da")


@pytest.mark.parametrize("field", ref.FIELDS)
def test_domain_elements_and_sparse_evaluation(gpu, poly, field):
    p, f, lib = ref.MODULUS[field], FIELD_ID[field], poly._lib()
    for log_n in CASES["domain_log_n"]:
        N = 1 << log_n
        dom = poly.EvaluationDomain(field, N)
        out = Dev(gpu, rows=N)
        assert lib.gh_domain_elements_dev(f, log_n, out.ptr) == 0, lib.gh_last_error()
        el = out.ints(p)
        g = el[1] if N > 1 else 1
        assert el == [pow(g, i, p) for i in range(N)] and pow(g, N, p) == 1 and (N == 1 or pow(g, N // 2, p) == p - 1)
        assert el == ints(dom.fft(mont([0, 1] if N > 1 else [1], p)), N, p)          # the group generator of the transforms
        assert dom.elements() == el
        out.free()
        assert poly.SparsePolynomial.from_coefficients(field, [(0, -1), (N, 1)]).evaluate_over_domain(dom).evals() == [0] * N
        assert dom.vanishing_polynomial().evaluate_over_domain(dom).evals() == [0] * N
        for terms in ([(0, 2), (1, 2)], [(3, 7), (N + 5, p - 2), (3 * N, 9)], []):      # 2 + 2x: sparse.rs's own test
            sp = poly.SparsePolynomial.from_coefficients(field, terms)
            assert sp.evaluate_over_domain(dom).evals() == [ref.sparse_evaluate(terms, x, p) for x in el], (log_n, terms)
            assert sp.evaluate_over_domain(dom).evals() == [sp.evaluate(x) for x in el]


# ---------------------------------------------------------------------------------------------------- the wrappers end to end
@pytest.mark.parametrize("field", ref.FIELDS)
def test_wrappers_follow_the_reference(gpu, poly, field):
    p = ref.MODULUS[field]
    D = poly.DensePolynomial
    mk = lambda c: D.from_coefficients(field, c)
    # dense.rs:366-494 at small sizes
    for deg in (0, 1, 2, 5, 17, 33):
        c = data(field, deg + 1, "w")
        a = mk(c)
        assert (a + a).coeffs() == [2 * x % p for x in c] and a.degree() == deg                    # double_polynomials_random
        for deg_b in (0, 1, 5, 20):
            cb = data(field, deg_b + 1, "wb")
            b = mk(cb)
            assert (a + b).coeffs() == ref.add_ref(c, cb, p) == (b + a).coeffs()                    # add_polynomials
            assert (a - b).coeffs() == ref.add_ref(c, cb, p, -1)                                    # sub_polynomials
            assert (b - a).coeffs() == [-x % p for x in (a - b).coeffs()]
            assert a.add_scaled(7, b).coeffs() == ref.add_ref(c, cb, p, 1, 7)                       # add_polynomials_with_mul
            assert (a * b).coeffs() == ref.naive_mul(c, cb, p)                                      # mul_polynomials_random
            if deg_b <= 1:                                                                          # divide_polynomials_random
                q, r = ref.divide_with_q_and_r(c, list(enumerate(cb)), p)
                assert (a / b).coeffs() == q
        assert (-a).coeffs() == [-x % p for x in c]
        z = ref.points(field)[4]
        assert a.evaluate(z) == ref.evaluate(c, z, p) and a.evaluate_many([0, z]) == [c[0], ref.evaluate(c, z, p)]
        assert (a - a).coeffs() == [0] * len(c) and (a - a).is_zero() and len(a - a) == len(c)      # the reference does not trim here
        assert (a + (-a)).coeffs() == [0] * len(c) and (mk([]) + a).coeffs() == c and (a - mk([])).coeffs() == c
        assert (mk([]) - a).coeffs() == [-x % p for x in c] and (a * mk([])).coeffs() == [] and mk([0, 0]).is_zero()
    c = data(field, 20, "w")
    a = mk(c)
    # a non-monic linear divisor, a root, the vanishing polynomial, the refusals
    lin = [5, 3]
    q, r = ref.divide_with_q_and_r(c, list(enumerate(lin)), p)
    assert (a / mk(lin)).coeffs() == q and ((a / mk(lin)) * mk(lin) + mk(r)).coeffs() == c
    assert (a * mk([-9 % p, 1]) / mk([-9 % p, 1])).coeffs() == c
    assert (a / mk([4])).coeffs() == [x * pow(4, -1, p) % p for x in c]
    dom = poly.EvaluationDomain(field, 8)
    van = mk([p - 1] + [0] * 7 + [1])
    q, r = ref.divide_with_q_and_r(c, ref.vanishing_terms(8, p), p)
    assert (a / van).coeffs() == q == (a / dom.vanishing_polynomial()).coeffs()
    assert [x.coeffs() for x in a.divide_by_vanishing_poly(dom)] == [q, r]
    assert a.mul_by_vanishing_poly(dom).coeffs() == (a * van).coeffs() == ref.mul_by_vanishing(c, 8, p)
    assert [x.coeffs() for x in a.mul_by_vanishing_poly(dom).divide_by_vanishing_poly(dom)] == [c, []]
    with pytest.raises(ZeroDivisionError):
        a / mk([0, 0])
    with pytest.raises(ValueError):
        a / mk([1, 2, 3])
    assert (mk([1, 2]) / mk([1, 2, 3])).coeffs() == []
    # evaluations: interpolate(evaluate_over_domain(p)) == p, and the pointwise operators
    for n in (1, 2, 7, 32, 33):
        cc = data(field, n, "w")
        pp = mk(cc)
        dom = poly.EvaluationDomain(field, n)
        ev = pp.evaluate_over_domain(dom)
        el = dom.elements()
        assert ev.evals() == [ref.evaluate(cc, x, p) for x in el]
        assert ev.interpolate().coeffs() == cc
        other = mk(data(field, max(n - 1, 1), "wb")).evaluate_over_domain(dom)
        assert (ev + other).evals() == [(x + y) % p for x, y in zip(ev.evals(), other.evals())]
        assert (ev - other).evals() == [(x - y) % p for x, y in zip(ev.evals(), other.evals())]
        assert (ev * other).evals() == [x * y % p for x, y in zip(ev.evals(), other.evals())] == dom.mul_polynomials_in_evaluation_domain(ev, other).evals()
        shifted = poly.Evaluations.from_ints([y or 1 for y in other.evals()], dom)
        assert (ev / shifted).evals() == [x * pow(y, -1, p) % p for x, y in zip(ev.evals(), shifted.evals())]
    small = poly.EvaluationDomain(field, 4)
    assert mk(data(field, 7, "w")).evaluate_over_domain(small).interpolate().coeffs() == ref.trim(data(field, 7, "w")[:4])     # Vec::resize truncates
    big, sub = poly.EvaluationDomain(field, 16), poly.EvaluationDomain(field, 4)
    assert sorted(big.reindex_by_subdomain(sub, i) for i in range(16)) == list(range(16))
    assert [big.elements()[big.reindex_by_subdomain(sub, i)] for i in range(4)] == sub.elements()
    assert big.evaluate_vanishing_polynomial(3) == (pow(3, 16, p) - 1) % p
    ev = mk(data(field, 16, "w")).evaluate_over_domain(big)
    before = ev.evals()
    big.divide_by_vanishing_poly_on_coset_in_place(ev)
    assert ev.evals() == [x * pow(pow(17, 16, p) - 1, -1, p) % p for x in before]
