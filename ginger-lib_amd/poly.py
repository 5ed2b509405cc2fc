"""DensePolynomial, SparsePolynomial and Evaluations of algebra::fft on the device (include/ginger_hip_poly.h), with the
reference's names (algebra/src/fft/polynomial/dense.rs, sparse.rs, mod.rs, evaluations.rs, domain.rs:222-302):

    EvaluationDomain(field, num_coeffs)      the transforms of the package's EvaluationDomain, and vanishing_polynomial,
                                             evaluate_vanishing_polynomial, elements, reindex_by_subdomain,
                                             divide_by_vanishing_poly_on_coset_in_place, mul_polynomials_in_evaluation_domain
    DensePolynomial.from_coefficients(field, ints)     + - unary - * /, add_scaled, evaluate, evaluate_many, degree, is_zero,
                                             mul_by_vanishing_poly, divide_by_vanishing_poly, evaluate_over_domain
    SparsePolynomial.from_coefficients(field, [(exponent, int)])     evaluate, evaluate_over_domain, to_dense
    Evaluations.from_ints(ints, domain)      + - * /, interpolate

field is "mnt4753_fr" or "mnt6753_fr".  The objects are built from and return Python integers; between operations their rows
stay in a DeviceBuffer (Montgomery rows of 12 u64), so a chain of operations never crosses PCIe.  Everything is exact.

`/` takes a divisor of degree 0, of degree 1 (a x + b: the quotient by x + b / a, scaled by 1 / a), or the vanishing polynomial
x^N - 1 of a domain; an all-zero divisor raises ZeroDivisionError as the reference panics, any other ValueError: dense long
division is serial in the quotient and is not on the device."""
import ctypes

import numpy as np

from . import EvaluationDomain as _Domain
from . import FFT_INVERSE, FIELDS, DeviceBuffer, GingerHipError, _check, _ptr, load_library    # noqa: F401 (GingerHipError: re-exported)
from . import _handles, limbs
from ._handles import ci, sz, u32, vp

_OUT_SIZE = ctypes.POINTER(sz)
_ARGTYPES = {"gh_poly_evaluate_dev": [ci, vp, sz, vp, sz, vp], "gh_poly_evaluate": [ci, vp, sz, vp, sz, vp],
             "gh_poly_resize_dev": [ci, vp, sz, vp, sz], "gh_poly_trimmed_len_dev": [ci, vp, sz, _OUT_SIZE],
             "gh_poly_add_dev": [ci, vp, sz, vp, sz, vp], "gh_poly_sub_dev": [ci, vp, sz, vp, sz, vp],
             "gh_poly_add_scaled_dev": [ci, vp, sz, vp, sz, vp, vp], "gh_poly_neg_dev": [ci, vp, sz, vp],
             "gh_poly_mul_by_vanishing_dev": [ci, vp, sz, u32, vp],
             "gh_poly_divide_by_vanishing_dev": [ci, vp, sz, u32, vp, vp], "gh_poly_divide_by_vanishing": [ci, vp, sz, u32, vp, vp],
             "gh_poly_divide_by_linear_dev": [ci, vp, sz, vp, vp, vp], "gh_poly_divide_by_linear": [ci, vp, sz, vp, vp, vp],
             "gh_poly_mul_dev": [ci, vp, sz, vp, sz, vp, sz, _OUT_SIZE], "gh_poly_mul": [ci, vp, sz, vp, sz, vp, sz, _OUT_SIZE],
             "gh_evals_div_dev": [ci, vp, vp, sz, _OUT_SIZE], "gh_domain_elements_dev": [ci, u32, vp],
             "gh_poly_sparse_evaluate_over_domain_dev": [ci, vp, vp, sz, u32, vp],
             "gh_poly_set_tuning": [u32, u32, u32], "gh_poly_last_timing": [ctypes.POINTER(ctypes.c_float)]}
# every symbol include/ginger_hip_poly.h declares
POLY_SYMBOLS = list(_ARGTYPES)
_lib = _handles.binder("polynomial", _ARGTYPES)

MODULUS = {limbs.FR_FIELD[k]: v for k, v in limbs.MODULUS.items()}
GENERATOR = 17      # F::multiplicative_generator of both fields: the coset of the coset transforms


def set_tuning(run_len=0, direct_max=0, seg_max=0):
    """elements per lane of a fold or scan, the longest vector one lane finishes, additions per lane of
    divide_by_vanishing_poly; 0 = the library's default"""
    _check(_lib().gh_poly_set_tuning(run_len, direct_max, seg_max))


def last_timing():
    """device milliseconds of the last call"""
    ms = ctypes.c_float()
    _check(_lib().gh_poly_last_timing(ctypes.byref(ms)))
    return ms.value


def _scalar(field, x):
    p = MODULUS[field]
    return np.ascontiguousarray(limbs.mont_rows([int(x) % p], p)[0])


def _alloc(rows):
    return DeviceBuffer(max(int(rows), 1) * 96)


def _upload(field, ints):
    p = MODULUS[field]
    ints = [int(v) % p for v in ints]
    buf = _alloc(len(ints))
    if ints:
        buf.upload(limbs.mont_rows(ints, p))
    return buf


def _download(field, buf, n):
    if not n:
        return []
    return limbs.ints_from_mont_rows(buf.download()[:12 * n], MODULUS[field])


def _trimmed_len(field, buf, n):
    out = sz()
    _check(_lib().gh_poly_trimmed_len_dev(FIELDS[field], buf.ptr, n, ctypes.byref(out)))
    return out.value


def _resized(field, buf, n, n_out):
    out = _alloc(n_out)
    _check(_lib().gh_poly_resize_dev(FIELDS[field], buf.ptr, n, out.ptr, n_out))
    return out


class EvaluationDomain(_Domain):
    """algebra::fft::EvaluationDomain with the helpers of domain.rs:222-302"""

    def vanishing_polynomial(self):
        return SparsePolynomial.from_coefficients(self.field, [(0, -1), (self.size, 1)])

    def evaluate_vanishing_polynomial(self, tau):
        p = MODULUS[self.field]
        return (pow(int(tau), self.size, p) - 1) % p

    def elements_dev(self):
        out = _alloc(self.size)
        _check(_lib().gh_domain_elements_dev(FIELDS[self.field], self.log_size_of_group, out.ptr))
        return out

    def elements(self):
        """group_gen^i, i < size"""
        return _download(self.field, self.elements_dev(), self.size)

    def divide_by_vanishing_poly_on_coset_in_place(self, evals):
        """evals *= 1 / (g^size - 1), g the multiplicative generator of the coset transforms"""
        p = MODULUS[self.field]
        inv = pow(self.evaluate_vanishing_polynomial(GENERATOR), -1, p)
        _check(load_library().gh_vec_scale_dev(FIELDS[self.field], evals.buf.ptr, _ptr(_scalar(self.field, inv)), evals.n))

    def mul_polynomials_in_evaluation_domain(self, a, b):
        """Evaluations x Evaluations -> Evaluations; arrays of limbs go the package's host path"""
        if isinstance(a, Evaluations):
            return a * b
        return super().mul_polynomials_in_evaluation_domain(a, b)

    def reindex_by_subdomain(self, other, index):
        assert self.size >= other.size
        period = self.size // other.size
        if index < other.size:
            return index * period
        i = index - other.size
        return i + i // (period - 1) + 1


class DensePolynomial:
    """coefficients c_0 .. c_(n - 1) on the device; n = len(self) is the reference's coeffs.len()"""

    def __init__(self, field, buf, n):
        self.field, self.buf, self.n = field, buf, int(n)

    @classmethod
    def from_coefficients(cls, field, coeffs):
        """from_coefficients_vec: trailing zeros are popped"""
        coeffs = list(coeffs)
        buf = _upload(field, coeffs)
        return cls(field, buf, _trimmed_len(field, buf, len(coeffs)))

    @classmethod
    def zero(cls, field):
        return cls(field, _alloc(0), 0)

    def __len__(self):
        return self.n

    def coeffs(self):
        return _download(self.field, self.buf, self.n)

    def _trimmed(self):
        return _trimmed_len(self.field, self.buf, self.n)

    def _trim(self):
        self.n = self._trimmed()
        return self

    def is_zero(self):
        return self.n == 0 or self._trimmed() == 0

    def degree(self):
        if self.is_zero():
            return 0
        assert self._trimmed() == self.n, "the leading coefficient is zero"
        return self.n - 1

    def clone(self):
        return DensePolynomial(self.field, _resized(self.field, self.buf, self.n, self.n), self.n)

    def _same(self, other):
        if not isinstance(other, DensePolynomial) or other.field != self.field:
            raise TypeError("a DensePolynomial over %s" % self.field)

    def evaluate_many(self, points):
        points = list(points)
        p = MODULUS[self.field]
        pts = np.ascontiguousarray(limbs.mont_rows([int(z) % p for z in points], p))
        out = np.zeros((len(points), 12), dtype=np.uint64)
        _check(_lib().gh_poly_evaluate_dev(FIELDS[self.field], self.buf.ptr, self.n, _ptr(pts), len(points), _ptr(out)))
        return limbs.ints_from_mont_rows(out, p)

    def evaluate(self, point):
        return self.evaluate_many([point])[0]

    def _axpy(self, fn, other, f=None):
        rows = max(self.n, other.n)
        out = _alloc(rows)
        args = [FIELDS[self.field], self.buf.ptr, self.n, other.buf.ptr, other.n]
        if f is not None:
            args.append(_ptr(_scalar(self.field, f)))
        _check(getattr(_lib(), fn)(*args, out.ptr))
        return DensePolynomial(self.field, out, rows)

    # Add, Sub and AddAssign((f, other)) keep the reference's lengths: where self.degree() >= other.degree() the reference
    # does not pop, so a cancellation of equal degrees leaves trailing zeros (dense.rs:159-165, :216-219, :275-280); only the
    # other branch trims.
    def _combine(self, fn, other, f=None):
        self._same(other)
        res = self._axpy(fn, other, f)
        return res if self.n >= other.n else res._trim()

    def __add__(self, other):
        self._same(other)
        if self.is_zero():
            return other.clone()
        if other.is_zero():
            return self.clone()
        return self._combine("gh_poly_add_dev", other)

    def __sub__(self, other):
        self._same(other)
        if self.is_zero():
            return -other
        if other.is_zero():
            return self.clone()
        return self._combine("gh_poly_sub_dev", other)

    def __neg__(self):
        out = _alloc(self.n)
        _check(_lib().gh_poly_neg_dev(FIELDS[self.field], self.buf.ptr, self.n, out.ptr))
        return DensePolynomial(self.field, out, self.n)

    def add_scaled(self, f, other):
        """self + f other: AddAssign<(F, &DensePolynomial)> (dense.rs:207-233)"""
        self._same(other)
        if self.is_zero():
            return DensePolynomial.zero(self.field)._axpy("gh_poly_add_scaled_dev", other, f)
        if other.is_zero():
            return self.clone()
        return self._combine("gh_poly_add_scaled_dev", other, f)

    def __mul__(self, other):
        self._same(other)
        cap = limbs.domain_size(self.n + other.n)
        out = _alloc(cap)
        n_out = sz()
        _check(_lib().gh_poly_mul_dev(FIELDS[self.field], self.buf.ptr, self.n, other.buf.ptr, other.n, out.ptr, cap, ctypes.byref(n_out)))
        return DensePolynomial(self.field, out, n_out.value)

    def mul_by_vanishing_poly(self, domain):
        out = _alloc(self.n + domain.size)
        _check(_lib().gh_poly_mul_by_vanishing_dev(FIELDS[self.field], self.buf.ptr, self.n, domain.log_size_of_group, out.ptr))
        return DensePolynomial(self.field, out, self.n + domain.size)._trim()

    def divide_by_vanishing_poly(self, domain):
        """-> (quotient, remainder), both trimmed"""
        nq = max(self.n, domain.size) - domain.size
        q, r = _alloc(nq), _alloc(domain.size)
        _check(_lib().gh_poly_divide_by_vanishing_dev(FIELDS[self.field], self.buf.ptr, self.n, domain.log_size_of_group, q.ptr, r.ptr))
        return DensePolynomial(self.field, q, nq)._trim(), DensePolynomial(self.field, r, domain.size)._trim()

    def divide_by_linear(self, z):
        """-> (quotient by x - z, remainder = self(z))"""
        nq = max(self.n, 1) - 1
        q = _alloc(nq)
        rem = np.zeros(12, dtype=np.uint64)
        _check(_lib().gh_poly_divide_by_linear_dev(FIELDS[self.field], self.buf.ptr, self.n, _ptr(_scalar(self.field, z)), q.ptr, _ptr(rem)))
        return DensePolynomial(self.field, q, nq)._trim(), limbs.ints_from_mont_rows(rem, MODULUS[self.field])[0]

    def __truediv__(self, divisor):
        p = MODULUS[self.field]
        if isinstance(divisor, SparsePolynomial):
            divisor = divisor.to_dense()
        self._same(divisor)
        nd = divisor._trimmed()
        if nd == 0:
            raise ZeroDivisionError("dividing by the zero polynomial")
        ns = self._trimmed()
        if ns < nd:
            return DensePolynomial.zero(self.field)
        me = DensePolynomial(self.field, self.buf, ns)
        if nd <= 2:
            c = _download(self.field, divisor.buf, nd)
            lead_inv = pow(c[-1], -1, p)
            quotient = me if nd == 1 else me.divide_by_linear(-c[0] * lead_inv % p)[0]
            return DensePolynomial.zero(self.field)._axpy("gh_poly_add_scaled_dev", quotient, lead_inv)._trim()
        N = nd - 1
        if N & (N - 1) == 0:
            c = _download(self.field, divisor.buf, nd)
            if c[0] == p - 1 and c[-1] == 1 and not any(c[1:-1]):
                return me.divide_by_vanishing_poly(EvaluationDomain(self.field, N))[0]
        raise ValueError("the divisor must have degree 0 or 1 or be the vanishing polynomial x^N - 1 of a domain")

    def evaluate_over_domain(self, domain):
        """the coefficient vector resized to the domain as Vec::resize does, then its transform"""
        buf = _resized(self.field, self.buf, self.n, domain.size)
        domain.fft_dev(buf)
        return Evaluations(self.field, buf, domain)


class SparsePolynomial:
    """[(exponent, coefficient)], sorted by exponent, zero coefficients dropped (sparse.rs)"""

    def __init__(self, field, terms):
        self.field, self.terms = field, terms

    @classmethod
    def from_coefficients(cls, field, terms):
        p = MODULUS[field]
        terms = sorted((int(e), int(c) % p) for e, c in terms)
        return cls(field, [(e, c) for e, c in terms if c])

    def is_zero(self):
        return not self.terms

    def degree(self):
        return self.terms[-1][0] if self.terms else 0

    def evaluate(self, point):
        p = MODULUS[self.field]
        return sum(c * pow(int(point), e, p) for e, c in self.terms) % p

    def to_dense(self):
        c = [0] * (self.degree() + 1 if self.terms else 0)
        for e, v in self.terms:
            c[e] = (c[e] + v) % MODULUS[self.field]
        return DensePolynomial.from_coefficients(self.field, c)

    def evaluate_over_domain(self, domain):
        p = MODULUS[self.field]
        t = len(self.terms)
        exps = np.array([e for e, _ in self.terms], dtype=np.uint64)
        co = np.ascontiguousarray(limbs.mont_rows([c for _, c in self.terms], p)) if t else np.zeros((0, 12), dtype=np.uint64)
        out = _alloc(domain.size)
        _check(_lib().gh_poly_sparse_evaluate_over_domain_dev(FIELDS[self.field], _ptr(exps), _ptr(co), t, domain.log_size_of_group, out.ptr))
        return Evaluations(self.field, out, domain)


class Evaluations:
    """the values of a polynomial over a domain, on the device (evaluations.rs)"""

    def __init__(self, field, buf, domain):
        self.field, self.buf, self.domain, self.n = field, buf, domain, domain.size

    @classmethod
    def from_ints(cls, evals, domain):
        evals = list(evals)
        if len(evals) != domain.size:
            raise ValueError("one value per element of the domain")
        return cls(domain.field, _upload(domain.field, evals), domain)

    def evals(self):
        return _download(self.field, self.buf, self.n)

    def clone(self):
        return Evaluations(self.field, _resized(self.field, self.buf, self.n, self.n), self.domain)

    def interpolate(self):
        buf = _resized(self.field, self.buf, self.n, self.n)
        self.domain.fft_dev(buf, FFT_INVERSE)
        return DensePolynomial(self.field, buf, self.n)._trim()

    def _same(self, other):
        if not isinstance(other, Evaluations) or other.field != self.field or other.n != self.n:
            raise TypeError("domains are unequal")

    def _axpy(self, fn, other):
        self._same(other)
        out = _alloc(self.n)
        _check(getattr(_lib(), fn)(FIELDS[self.field], self.buf.ptr, self.n, other.buf.ptr, other.n, out.ptr))
        return Evaluations(self.field, out, self.domain)

    def __add__(self, other):
        return self._axpy("gh_poly_add_dev", other)

    def __sub__(self, other):
        return self._axpy("gh_poly_sub_dev", other)

    def __mul__(self, other):
        self._same(other)
        res = self.clone()
        _check(load_library().gh_vec_mul_dev(FIELDS[self.field], res.buf.ptr, other.buf.ptr, self.n))
        return res

    def __truediv__(self, other):
        self._same(other)
        res = self.clone()
        zeros = sz()
        _check(_lib().gh_evals_div_dev(FIELDS[self.field], res.buf.ptr, other.buf.ptr, self.n, ctypes.byref(zeros)))
        if zeros.value:
            raise ZeroDivisionError("%d of the divisor's evaluations are zero" % zeros.value)
        return res
