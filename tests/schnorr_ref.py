"""Python restatement of the field-based Schnorr signature over MNT4-753 / MNT6-753 (test infrastructure), on top of pyref
and poseidon_ref.

Written from the scheme's definition: pk = sk G; sign with nonce k != 0: R = k G, e = H(m || R.x || R.y || pk.x), rejected if
e >= 2^752, s = k + e sk mod r, rejected if s >= 2^752; verify: Err if e or s >= 2^752, else R' = s G - e pk and
Ok(e == H(m || R'.x || R'.y || pk.x)); the point at infinity hashes as (0, 1); keyverify is the on-curve test (cofactor 1).
Scalar multiplication is Jacobian double-and-add with one inversion at the end (pyref.Curve.mul inverts at every step).
"""
import random

import poseidon_ref
import pyref

BOUND = 1 << 752
# scheme -> (poseidon tag = data field, group curve)
SCHEMES = {"SchnorrMNT4": ("mnt4753", "mnt6753_g1"), "SchnorrMNT6": ("mnt6753", "mnt4753_g1")}


def _jac_dbl(P, p, a):
    X, Y, Z = P
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    YY = Y * Y % p
    S = 4 * X * YY % p
    M = (3 * X * X + a * pow(Z, 4, p)) % p
    X3 = (M * M - 2 * S) % p
    return (X3, (M * (S - X3) - 8 * YY * YY) % p, 2 * Y * Z % p)


def _jac_add(P, Q, p, a):
    if P[2] == 0:
        return Q
    if Q[2] == 0:
        return P
    X1, Y1, Z1 = P
    X2, Y2, Z2 = Q
    Z1Z1, Z2Z2 = Z1 * Z1 % p, Z2 * Z2 % p
    U1, U2 = X1 * Z2Z2 % p, X2 * Z1Z1 % p
    S1, S2 = Y1 * Z2 * Z2Z2 % p, Y2 * Z1 * Z1Z1 % p
    if U1 == U2:
        return _jac_dbl(P, p, a) if S1 == S2 else (1, 1, 0)
    H, R = (U2 - U1) % p, (S2 - S1) % p
    HH = H * H % p
    HHH = H * HH % p
    V = U1 * HH % p
    X3 = (R * R - HHH - 2 * V) % p
    return (X3, (R * (V - X3) - S1 * HHH) % p, Z1 * Z2 * H % p)


def mul(curve, k, P):
    """k * P for an affine point P (tuple of ints, or None) and any k >= 0 -> affine or None"""
    if P is None or k == 0:
        return None
    p, a = curve.F.p, curve.a[0]
    base = (P[0][0], P[1][0], 1)
    acc = (1, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jac_dbl(acc, p, a)
        if bit == "1":
            acc = _jac_add(acc, base, p, a)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, p)
    return ((acc[0] * zi * zi % p,), (acc[1] * zi * zi * zi % p,))


def add(curve, P, Q):
    return curve.add(P, Q)


def coords(P):
    """affine coordinates as the hash sees them: GroupAffine::zero() = (0, 1) for infinity"""
    return (0, 1) if P is None else (P[0][0], P[1][0])


class Schnorr:
    def __init__(self, scheme):
        tag, cname = SCHEMES[scheme]
        self.name = scheme
        self.H = poseidon_ref.Poseidon(tag)
        self.C = pyref.CURVES[cname]
        self.F = self.H.F                    # data field
        self.p = self.F.p
        self.r = self.C.order                # the group's scalar field
        self.R = pyref.FIELDS["p4" if self.C.F is pyref.P6 else "p6"]   # scalar field as a pyref.Field (Montgomery conversions)
        assert self.R.p == self.r and self.C.F.p == self.p
        self.G = self.C.G

    def pk(self, sk):
        return mul(self.C, sk % self.r, self.G)

    def hash(self, msg, R, pk):
        x, y = coords(R)
        return self.H.evaluate(list(msg) + [x, y, coords(pk)[0]])

    def sign_with(self, sk, pk, msg, k):
        """one attempt with nonce k: (e, s), or None where the reference draws again"""
        if k % self.r == 0:
            return None
        e = self.hash(msg, mul(self.C, k, self.G), pk)
        if e >= BOUND:
            return None
        s = (k + e * sk) % self.r
        if s >= BOUND:
            return None
        return e, s

    def sign(self, sk, pk, msg, rng):
        while True:
            sig = self.sign_with(sk, pk, msg, rng.randrange(self.r))
            if sig:
                return sig

    def verify(self, pk, msg, sig):
        """True / False, or None for the reference's Err"""
        e, s = sig
        if e >= BOUND or s >= BOUND:
            return None
        R = self.C.add(mul(self.C, s, self.G), self.C.neg(mul(self.C, e, pk)))
        return self.hash(msg, R, pk) == e

    def keyverify(self, pk):
        return self.C.on_curve(pk)

    def keygen(self, rng):
        sk = rng.randrange(self.r)
        return self.pk(sk), sk

    # ABI conversions
    def fe(self, x):
        return pyref.int_to_limbs(self.F.to_mont(x % self.p))

    def sc(self, x):
        return pyref.int_to_limbs(self.R.to_mont(x % self.r))

    def pk_abi(self, P):
        """(24 limbs, infinity byte); infinity as zeros"""
        if P is None:
            return [0] * 24, 1
        return self.fe(P[0][0]) + self.fe(P[1][0]), 0

    def from_fe(self, limbs):
        return self.F.from_mont(pyref.limbs_to_int([int(v) for v in limbs]))


def rng(seed):
    return random.Random(seed)
