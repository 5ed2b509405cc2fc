"""Python restatement of the MNT6-753 reduced ate pairing: the textbook form, which shares nothing with the device code but
the curve.  Fq6 = Fq[w]/(w^6 - 11), a G2 point (x', y') of the twist is untwisted to (x' w^-2, y' w^-3), the Miller loop runs
affine over the plain bits of T = p - r (positive: f is not inverted) and f is raised to (p^6 - 1)/r by square and multiply.
The reduced pairing is unique, so this equals the reference's value word for word (algebra/src/curves/mnt6753/tests.rs:319-590).

An Fq6 element is the list [a0 .. a5] of the coefficients of 1, w .. w^5; the reference's tower order (Fp6::write: c0.c0, c0.c1,
c0.c2, c1.c0, c1.c1, c1.c2 with c0, c1 in Fq3 = Fq[u]/(u^3 - 11), u = w^2) is [a0, a2, a4, a1, a3, a5]: tower().
Points are pyref's: None for infinity, G1 ((x,), (y,)), G2 ((x0, x1, x2), (y0, y1, y2)).  Test infrastructure."""
import functools
import json
import os

import numpy as np

import pyref

C1, C2 = pyref.CURVES["mnt6753_g1"], pyref.CURVES["mnt6753_g2"]
E3 = C2.E
p, r = C1.F.p, C1.order
NR = 11
T = p - r
FINAL_EXPONENT = (p ** 6 - 1) // r
ONE = [1, 0, 0, 0, 0, 0]
ZERO = [0] * 6
_I11 = pow(NR, -1, p)
KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairing6_kats.json")))


def mul(a, b):
    o = [0] * 11
    for i in range(6):
        for j in range(6):
            o[i + j] += a[i] * b[j]
    for i in range(10, 5, -1):
        o[i - 6] += NR * o[i]
    return [v % p for v in o[:6]]


def add(a, b):
    return [(x + y) % p for x, y in zip(a, b)]


def sub(a, b):
    return [(x - y) % p for x, y in zip(a, b)]


def fpow(a, e):
    if e < 0:
        a, e = inv(a), -e
    res = ONE
    for bit in bin(e)[2:]:
        res = mul(res, res)
        if bit == "1":
            res = mul(res, a)
    return res


def inv(a):
    """1 / (A + B w) = (A - B w) / (A^2 - u B^2) with A = (a0, a2, a4), B = (a1, a3, a5) in Fq3; zero gives zero"""
    A, B = (a[0], a[2], a[4]), (a[1], a[3], a[5])
    n = E3.sub(E3.mul(A, A), E3.mul((0, 1, 0), E3.mul(B, B)))
    if E3.is_zero(n):
        return list(ZERO)
    ni = E3.inv(n)
    c0, c1 = E3.mul(A, ni), E3.neg(E3.mul(B, ni))
    return [c0[0], c1[0], c0[1], c1[1], c0[2], c1[2]]


def frobenius(a, k):
    return fpow(a, p ** k)


def tower(a):
    return [a[0], a[2], a[4], a[1], a[3], a[5]]


def from_tower(t):
    return [t[0], t[3], t[1], t[4], t[2], t[5]]


@functools.lru_cache(maxsize=64)
def miller(P, Q):
    """the Miller value f_{T,Q}(P); P, Q not infinity"""
    Px, Py = [P[0][0], 0, 0, 0, 0, 0], [P[1][0], 0, 0, 0, 0, 0]
    Qx = mul([Q[0][0], 0, Q[0][1], 0, Q[0][2], 0], [0, 0, 0, 0, _I11, 0])       # w^-2 = w^4 / 11
    Qy = mul([Q[1][0], 0, Q[1][1], 0, Q[1][2], 0], [0, 0, 0, _I11, 0, 0])       # w^-3 = w^3 / 11
    a6 = [C1.a[0], 0, 0, 0, 0, 0]

    def line(R, S):
        if R == S:
            lam = mul(add(mul([3, 0, 0, 0, 0, 0], mul(R[0], R[0])), a6), inv(add(R[1], R[1])))
        else:
            lam = mul(sub(S[1], R[1]), inv(sub(S[0], R[0])))
        x3 = sub(sub(mul(lam, lam), R[0]), S[0])
        y3 = sub(mul(lam, sub(R[0], x3)), R[1])
        return sub(sub(Py, R[1]), mul(lam, sub(Px, R[0]))), (x3, y3)

    f, R = ONE, (Qx, Qy)
    for bit in bin(T)[3:]:
        l, R = line(R, R)
        f = mul(mul(f, f), l)
        if bit == "1":
            l, R = line(R, (Qx, Qy))
            f = mul(f, l)
    return tuple(f)


def final_exponentiation(f):
    return fpow(f, FINAL_EXPONENT)


def product(pairs):
    """final_exp(prod miller(P, Q)); a pair with either point at infinity contributes one"""
    f = ONE
    for P, Q in pairs:
        if P is None or Q is None:
            continue
        f = mul(f, list(miller(P, Q)))
    return final_exponentiation(f)


def pairing(P, Q):
    return product([(P, Q)])


def groth16_verify(vk, proof, inputs):
    """proof-systems/src/groth16/verifier.rs:18-44.  vk: dict alpha_g1_beta_g2 (Fq6), gamma_g2, delta_g2, gamma_abc_g1;
    proof (A, B, C).  None = MalformedVerifyingKey."""
    abc = vk["gamma_abc_g1"]
    if len(inputs) + 1 != len(abc):
        return None
    g_ic = abc[0]
    for x, b in zip(inputs, abc[1:]):
        g_ic = C1.add(g_ic, C1.mul(x % r, b))
    A, B, C = proof
    neg2 = lambda Q: None if Q is None else C2.neg(Q)
    return product([(A, B), (g_ic, neg2(vk["gamma_g2"])), (C, neg2(vk["delta_g2"]))]) == vk["alpha_g1_beta_g2"]


def kat():
    """the reference's known answer: (P, Q, expected Fq6 in this module's coefficient order)"""
    v = [int(x, 16) for x in KATS["test_bilinearity"]["from_repr"]]
    zi = pow(v[2], -1, p)
    P = ((v[0] * zi % p,), (v[1] * zi % p,))
    zi3 = E3.inv(tuple(v[9:12]))
    Q = (E3.mul(tuple(v[3:6]), zi3), E3.mul(tuple(v[6:9]), zi3))
    return P, Q, from_tower(v[12:18])


# ---- the C ABI's layouts (12 u64 Montgomery limbs per Fq element)
def limbs(x):
    return pyref.int_to_limbs(C1.F.to_mont(x))


def g1_row(P):
    return np.array(limbs(P[0][0]) + limbs(P[1][0]) if P is not None else [0] * 24, dtype=np.uint64)


def g2_row(Q):
    if Q is None:
        return np.zeros(72, dtype=np.uint64)
    return np.array(sum((limbs(v) for v in tuple(Q[0]) + tuple(Q[1])), []), dtype=np.uint64)


def g1_batch(points):
    """-> (xy (n, 24), inf (n,)) as the package takes a batch of G1 points"""
    return np.stack([g1_row(P) for P in points]), np.array([P is None for P in points], dtype=np.uint8)


def g2_batch(points):
    return np.stack([g2_row(Q) for Q in points]), np.array([Q is None for Q in points], dtype=np.uint8)


def fq6_row(a):
    """this module's coefficient order -> 72 limbs in the order of Fp6::write"""
    return np.array(sum((limbs(v) for v in tower(a)), []), dtype=np.uint64)


def fq6_of(row):
    row = [int(v) for v in row]
    return from_tower([C1.F.from_mont(pyref.limbs_to_int(row[12 * i:12 * i + 12])) for i in range(6)])
