"""Python restatement of point compression, decompression and group membership (test infrastructure), on pyref.Ext /
pyref.Curve: the reference's GroupAffine::compress / decompress / group_membership_test
(algebra/src/curves/models/short_weierstrass_projective.rs:82-121, :205-268) with its square roots -- Tonelli-Shanks
(fields/macros.rs:52-105) in Fq and Fq3, the complex method with its c1 = 0 branch (fields/models/fp2.rs:186-214) in Fq2."""
import pyref

OK, INVALID_FIELD_ELEMENT, INVALID_FLAGS, NOT_ON_CURVE, NOT_PRIME_ORDER = 0, 1, 2, 3, 4
FLAG_INFINITY, FLAG_PARITY = 1, 2
MODULUS_BITS = 753

_ts_cache = {}


def _ts_params(E):
    """q^k - 1 = 2^s t and c^t for a non-residue c of the field"""
    key = (E.p, E.k)
    if key not in _ts_cache:
        q = E.p ** E.k
        s, t = 0, q - 1
        while t % 2 == 0:
            t //= 2
            s += 1
        k = 1
        while True:
            c = (k,) if E.k == 1 else (k, 1) + (0,) * (E.k - 2)
            if E.pow(c, (q - 1) // 2) != E.one():
                break
            k += 1
        _ts_cache[key] = (s, t, E.pow(c, t))
    return _ts_cache[key]


def is_square(E, a):
    """Euler's criterion (zero counts as a square, as sqrt gives Some(0))"""
    return E.is_zero(a) or E.pow(a, (E.p ** E.k - 1) // 2) == E.one()


def sqrt_ts(E, a):
    """a root of a in Fq^k or None: textbook Tonelli-Shanks"""
    if E.is_zero(a):
        return a
    if not is_square(E, a):
        return None
    s, t, z = _ts_params(E)
    w = E.pow(a, (t - 1) // 2)
    x = E.mul(a, w)
    b = E.mul(x, w)
    v = s
    while b != E.one():
        k, b2k = 0, b
        while b2k != E.one():
            b2k = E.mul(b2k, b2k)
            k += 1
        w = z
        for _ in range(v - k - 1):
            w = E.mul(w, w)
        z = E.mul(w, w)
        b = E.mul(b, z)
        x = E.mul(x, w)
        v = k
    return x


def ts_rounds(E, a):
    """how many correction rounds Tonelli-Shanks takes for the square a (0 = a^t is already 1)"""
    s, t, _ = _ts_params(E)
    b, k = E.pow(a, t), 0
    while b != E.one():
        b = E.mul(b, b)
        k += 1
    return k


def fp2_sqrt(E, a):
    """fp2.rs:186-214: the complex method; an element with c1 = 0 is rooted in Fq only (None for a non-residue c0, although
    it has a root in Fq2)"""
    F1 = pyref.Ext(E.F, 1, 0)
    p = E.p
    if a[1] == 0:
        r = sqrt_ts(F1, (a[0],))
        return None if r is None else (r[0], 0)
    norm = (a[0] * a[0] - E.nr * a[1] * a[1]) % p
    alpha = sqrt_ts(F1, (norm,))
    if alpha is None:
        return None
    half = pow(2, -1, p)
    delta = (alpha[0] + a[0]) * half % p
    if not is_square(F1, (delta,)):
        delta = (delta - alpha[0]) % p
    c0 = sqrt_ts(F1, (delta,))[0]
    return (c0, a[1] * half * pow(c0, -1, p) % p)


def field_sqrt(C, a):
    return fp2_sqrt(C.E, a) if C.deg == 2 else sqrt_ts(C.E, a)


def is_odd(a):
    """fp2.rs:101-103, fp3.rs:135-139: the parity of the highest non-zero coefficient"""
    for c in reversed(a):
        if c:
            return bool(c & 1)
    return False


def rhs(C, x):
    E = C.E
    return E.add(E.add(E.mul(E.mul(x, x), x), E.mul(C.a, x)), C.b)


def membership(C, P):
    """group_membership_test: on the curve and r P = infinity"""
    return P is None or (C.on_curve(P) and C.mul(C.order, P) is None)


def compress(C, P):
    """-> (x coefficients, flags)"""
    if P is None:
        return C.E.zero(), FLAG_INFINITY
    return P[0], FLAG_PARITY if is_odd(P[1]) else 0


def decompress(C, x, flags, check_subgroup=True):
    """x: canonical coefficients as read (any non-negative integers) -> (status, point); the point is None at infinity and
    for a failed row"""
    if any(c >= C.E.p for c in x):
        return INVALID_FIELD_ELEMENT, None
    inf, parity = bool(flags & FLAG_INFINITY), bool(flags & FLAG_PARITY)
    if flags & ~3 or (inf and (parity or any(x))):
        return INVALID_FLAGS, None
    if inf:
        return OK, None
    y = field_sqrt(C, rhs(C, tuple(x)))
    if y is None:
        return NOT_ON_CURVE, None
    if is_odd(y) != parity:
        y = C.E.neg(y)
    P = (tuple(x), y)
    if check_subgroup and C.mul(C.order, P) is not None:
        return NOT_PRIME_ORDER, None
    return OK, P


def to_bits(x, flags):
    """the reference's Vec<bool>: per coefficient 753 bits, most significant first, then the infinity and the parity bit"""
    out = []
    for c in x:
        out += [(c >> i) & 1 for i in range(MODULUS_BITS - 1, -1, -1)]
    return out + [flags & 1, (flags >> 1) & 1]


def from_bits(bits, deg):
    body = bits[:-2]
    assert len(body) == deg * MODULUS_BITS
    x = tuple(int("".join(str(int(b)) for b in body[MODULUS_BITS * c:MODULUS_BITS * (c + 1)]), 2) for c in range(deg))
    return x, int(bits[-2]) | int(bits[-1]) << 1
