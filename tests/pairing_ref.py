"""Python restatement of the MNT4-753 and MNT6-753 reduced ate pairings: the textbook form, which shares nothing with the
device code but the curves.  One class, Engine, parametrised by the embedding degree k (4 or 6, d = k / 2); reach the two
instances as engine("mnt4753") / engine("mnt6753").  Fq^k = Fq[w]/(w^k - NR), a G2 point (x', y') of the twist is untwisted to
(x' w^-2, y' w^-3), the Miller loop runs affine over the plain bits of T = |p - r|, f is inverted where the trace is negative
and raised to (p^k - 1)/r by square and multiply.  The reduced pairing is unique, so this equals the reference's value word for
word.

                                  mnt4753 (id 0)                        mnt6753 (id 2)
    k, NR                         4, 13                                 6, 11
    T                             r - p: negative trace, f inverted     p - r: positive, f as it is
    Fr (input_rows)               pyref.P6                              pyref.P4
    the reference's test          algebra/src/curves/mnt4753/           algebra/src/curves/mnt6753/
                                  tests.rs:266-467                      tests.rs:319-590
    tower order (gt_row)          Fp4::write: c0.c0, c0.c1, c1.c0,      Fp6::write: c0.c0, c0.c1, c0.c2, c1.c0, c1.c1,
                                  c1.c1 with c0, c1 in                  c1.c2 with c0, c1 in
                                  Fq2 = Fq[u]/(u^2 - 13), u = w^2       Fq3 = Fq[u]/(u^3 - 11), u = w^2

An Fq^k element is the list [a0 .. a(k-1)] of the coefficients of 1, w .. w^(k-1); the reference's tower order is the even
coefficients followed by the odd ones ([a0, a2, a1, a3] / [a0, a2, a4, a1, a3, a5]): tower().  Points are pyref's: None for
infinity, G1 ((x,), (y,)), G2 ((x0 .. x(d-1)), (y0 .. y(d-1))).  Test infrastructure."""
import functools
import json
import os

import numpy as np

import pyref

ENGINES = ("mnt4753", "mnt6753")
_PARAMS = {"mnt4753": (0, 4, 13, pyref.P6, "pairing_kats.json"), "mnt6753": (2, 6, 11, pyref.P4, "pairing6_kats.json")}


class Engine:
    def __init__(self, name):
        self.name = name
        self.id, self.k, self.NR, self.fr, kats = _PARAMS[name]
        self.d = self.k // 2
        self.C1, self.C2 = pyref.CURVES[name + "_g1"], pyref.CURVES[name + "_g2"]
        self.p, self.r = self.C1.F.p, self.C1.order
        assert self.fr.p == self.r
        self.T = abs(self.r - self.p)
        self.FINAL_EXPONENT = (self.p ** self.k - 1) // self.r
        self.ONE, self.ZERO = [1] + [0] * (self.k - 1), [0] * self.k
        self.gt_words = 12 * self.k
        self.KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", kats)))
        self.miller = functools.lru_cache(maxsize=64)(self._miller)

    def mul(self, a, b):
        k = self.k
        o = [0] * (2 * k - 1)
        for i in range(k):
            for j in range(k):
                o[i + j] += a[i] * b[j]
        for i in range(2 * k - 2, k - 1, -1):
            o[i - k] += self.NR * o[i]
        return [v % self.p for v in o[:k]]

    def add(self, a, b):
        return [(x + y) % self.p for x, y in zip(a, b)]

    def sub(self, a, b):
        return [(x - y) % self.p for x, y in zip(a, b)]

    def fpow(self, a, e):
        if e < 0:
            a, e = self.inv(a), -e
        res = self.ONE
        for bit in bin(e)[2:]:
            res = self.mul(res, res)
            if bit == "1":
                res = self.mul(res, a)
        return res

    def inv(self, a):
        """1 / (A + B w) = (A - B w) / (A^2 - u B^2) with A the even and B the odd coefficients, in Fq^d; zero gives zero"""
        E = self.C2.E
        A, B = tuple(a[0::2]), tuple(a[1::2])
        n = E.sub(E.mul(A, A), E.mul((0, 1) + (0,) * (self.d - 2), E.mul(B, B)))
        if E.is_zero(n):
            return list(self.ZERO)
        ni = E.inv(n)
        out = [0] * self.k
        out[0::2], out[1::2] = E.mul(A, ni), E.neg(E.mul(B, ni))
        return out

    def frobenius(self, a, j):
        return self.fpow(a, self.p ** j)

    def tower(self, a):
        return list(a[0::2]) + list(a[1::2])

    def from_tower(self, t):
        out = [0] * self.k
        out[0::2], out[1::2] = t[:self.d], t[self.d:]
        return out

    def _embed(self, c, shift=0):
        """c in Fq^d -> c(u = w^2) w^shift / NR^(shift > 0), shift < k"""
        out = [0] * self.k
        out[0:2 * len(c):2] = c
        if shift:
            s = [0] * self.k
            s[shift] = pow(self.NR, -1, self.p)
            out = self.mul(out, s)
        return out

    def _miller(self, P, Q):
        """the Miller value f_{T,Q}(P), inverted where the trace is negative; P, Q not infinity"""
        mul, add, sub, inv = self.mul, self.add, self.sub, self.inv
        Px, Py = self._embed(P[0]), self._embed(P[1])
        Qx = self._embed(Q[0], self.k - 2)                                           # w^-2 = w^(k-2) / NR
        Qy = self._embed(Q[1], self.k - 3)                                           # w^-3 = w^(k-3) / NR
        a, three = self._embed(self.C1.a), self._embed((3,))

        def line(R, S):
            if R == S:
                lam = mul(add(mul(three, mul(R[0], R[0])), a), inv(add(R[1], R[1])))
            else:
                lam = mul(sub(S[1], R[1]), inv(sub(S[0], R[0])))
            x3 = sub(sub(mul(lam, lam), R[0]), S[0])
            y3 = sub(mul(lam, sub(R[0], x3)), R[1])
            return sub(sub(Py, R[1]), mul(lam, sub(Px, R[0]))), (x3, y3)

        f, R = self.ONE, (Qx, Qy)
        for bit in bin(self.T)[3:]:
            l, R = line(R, R)
            f = mul(mul(f, f), l)
            if bit == "1":
                l, R = line(R, (Qx, Qy))
                f = mul(f, l)
        return tuple(inv(f) if self.r > self.p else f)

    def final_exponentiation(self, f):
        return self.fpow(f, self.FINAL_EXPONENT)

    def product(self, pairs):
        """final_exp(prod miller(P, Q)); a pair with either point at infinity contributes one"""
        f = self.ONE
        for P, Q in pairs:
            if P is None or Q is None:
                continue
            f = self.mul(f, self.miller(P, Q))
        return self.final_exponentiation(f)

    def pairing(self, P, Q):
        return self.product([(P, Q)])

    @functools.cached_property
    def e0(self):
        """e(G1, G2): the one Python pairing that every key known in the exponent and every bilinearity test share"""
        return self.pairing(self.C1.G, self.C2.G)

    def groth16_verify(self, vk, proof, inputs):
        """proof-systems/src/groth16/verifier.rs:18-44.  vk: dict alpha_g1_beta_g2 (Fq^k), gamma_g2, delta_g2, gamma_abc_g1;
        proof (A, B, C).  None = MalformedVerifyingKey."""
        C1, C2 = self.C1, self.C2
        abc = vk["gamma_abc_g1"]
        if len(inputs) + 1 != len(abc):
            return None
        g_ic = abc[0]
        for x, b in zip(inputs, abc[1:]):
            g_ic = C1.add(g_ic, C1.mul(x % self.r, b))
        A, B, C = proof
        neg2 = lambda Q: None if Q is None else C2.neg(Q)
        return self.product([(A, B), (g_ic, neg2(vk["gamma_g2"])), (C, neg2(vk["delta_g2"]))]) == vk["alpha_g1_beta_g2"]

    def kat(self):
        """the reference's known answer: (P, Q, expected Fq^k in this module's coefficient order).  The golden list is G1
        (x, y, z), G2 (x, y, z) of d words each, then the k words of the value in tower order."""
        E, d, p = self.C2.E, self.d, self.p
        v = [int(x, 16) for x in self.KATS["test_bilinearity"]["from_repr"]]
        zi = pow(v[2], -1, p)
        P = ((v[0] * zi % p,), (v[1] * zi % p,))
        zi2 = E.inv(tuple(v[3 + 2 * d:3 + 3 * d]))
        Q = (E.mul(tuple(v[3:3 + d]), zi2), E.mul(tuple(v[3 + d:3 + 2 * d]), zi2))
        return P, Q, self.from_tower(v[3 + 3 * d:3 + 3 * d + self.k])

    # ---- the C ABI's layouts (12 u64 Montgomery limbs per Fq element)
    def limbs(self, x):
        return pyref.int_to_limbs(self.C1.F.to_mont(x))

    def g1_row(self, P):
        return np.array(self.limbs(P[0][0]) + self.limbs(P[1][0]) if P is not None else [0] * 24, dtype=np.uint64)

    def g2_row(self, Q):
        if Q is None:
            return np.zeros(self.gt_words, dtype=np.uint64)
        return np.array(sum((self.limbs(v) for v in tuple(Q[0]) + tuple(Q[1])), []), dtype=np.uint64)

    def g1_batch(self, points):
        """-> (xy (n, 24), inf (n,)) as the package takes a batch of G1 points"""
        return np.stack([self.g1_row(P) for P in points]), np.array([P is None for P in points], dtype=np.uint8)

    def g2_batch(self, points):
        return np.stack([self.g2_row(Q) for Q in points]), np.array([Q is None for Q in points], dtype=np.uint8)

    def gt_row(self, a):
        """this module's coefficient order -> gt_words limbs in the order of Fp4::write / Fp6::write"""
        return np.array(sum((self.limbs(v) for v in self.tower(a)), []), dtype=np.uint64)

    def gt_of(self, row):
        row = [int(v) for v in row]
        return self.from_tower([self.C1.F.from_mont(pyref.limbs_to_int(row[12 * i:12 * i + 12])) for i in range(self.k)])

    def input_rows(self, inputs):
        """lists of integers -> (n, n_inputs, 12) Montgomery rows of the engine's Fr"""
        rows = [[pyref.int_to_limbs(self.fr.to_mont(v % self.r)) for v in row] for row in inputs]
        return np.array(rows, dtype=np.uint64).reshape(len(inputs), -1, 12)


@functools.lru_cache(maxsize=None)
def engine(name):
    return Engine(name)
