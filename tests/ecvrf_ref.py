"""Python restatement of the Bowe-Hopwood Pedersen hash and of the field-based EC-VRF over MNT4-753 / MNT6-753 (test
infrastructure), on top of pyref, poseidon_ref and schnorr_ref.mul.

Written from the definitions.  Bowe-Hopwood: the input bytes as bits, least significant bit of each byte first, zero-padded
to a multiple of 3; chunk t = (c0, c1, c2) adds (1 - 2 c2)(1 + c0 + 2 c1) generators[t / W][t % W]; the empty input hashes to
infinity.  The reference's generator recipe: per segment a base, then 16 base, 256 base, ...  EC-VRF with nonce r != 0:
mh = BH(to_bytes(m_0) || ...) with every element as its canonical integer in 96 little-endian bytes; gamma = sk mh;
c = H(m || pk.x || (r G).x || (r mh).x), rejected if c >= 2^752; s = r + sk c mod r_G, rejected if s >= 2^752.
proof_to_hash: Err if c or s >= 2^752, Err if gamma is off the curve, u = s G - c pk, v = s mh - c gamma, FailedVerification
unless H(m || pk.x || u.x || v.x) == c, else the output H(m || gamma.x || gamma.y).  Infinity hashes as (0, 1).
"""
import random

import poseidon_ref
import pyref
from schnorr_ref import BOUND, coords, mul

# scheme -> (poseidon tag = data field, group curve)
SCHEMES = {"EcVrfMNT4": ("mnt4753", "mnt6753_g1"), "EcVrfMNT6": ("mnt6753", "mnt4753_g1")}
# proof_to_hash outcomes, as the device's status codes
OK, FAILED, RANGE, GAMMA = 1, 0, 2, 3


def bytes_to_bits(data):
    return [(b >> i) & 1 for b in data for i in range(8)]


def recipe_generators(curve, bases, window_size):
    """generators[seg][k] = 16^k bases[seg] (the reference's create_generators with the caller's segment bases)"""
    gens = []
    for base in bases:
        seg, P = [], base
        for _ in range(window_size):
            seg.append(P)
            P = mul(curve, 16, P)
        gens.append(seg)
    return gens


class BoweHopwood:
    def __init__(self, curve, generators):
        """generators: num_windows lists of window_size affine points (None = infinity)"""
        self.C = curve
        self.gens = generators
        self.num_windows, self.window_size = len(generators), len(generators[0])

    def capacity_bits(self):
        return 3 * self.num_windows * self.window_size

    def chunks(self, data):
        """the signed digits (1 - 2 c2)(1 + c0 + 2 c1), one per chunk present"""
        bits = bytes_to_bits(data)
        bits += [0] * (-len(bits) % 3)
        return [(1 - 2 * bits[i + 2]) * (1 + bits[i] + 2 * bits[i + 1]) for i in range(0, len(bits), 3)]

    def evaluate(self, data):
        if 8 * len(data) > self.capacity_bits():
            raise ValueError("input longer than the parameters take")
        acc = None
        for t, d in enumerate(self.chunks(data)):
            g = self.gens[t // self.window_size][t % self.window_size]
            P = mul(self.C, abs(d), g)
            acc = self.C.add(acc, P if d > 0 else self.C.neg(P))
        return acc

    def flat(self):
        return [g for seg in self.gens for g in seg]


class EcVrf:
    def __init__(self, scheme, bh):
        tag, cname = SCHEMES[scheme]
        self.name = scheme
        self.H = poseidon_ref.Poseidon(tag)
        self.C = pyref.CURVES[cname]
        self.F = self.H.F                    # data field
        self.p = self.F.p
        self.r = self.C.order                # the group's scalar field
        self.R = pyref.FIELDS["p4" if self.C.F is pyref.P6 else "p6"]
        assert self.R.p == self.r and self.C.F.p == self.p
        self.G = self.C.G
        self.bh = bh

    def pk(self, sk):
        return mul(self.C, sk % self.r, self.G)

    def keygen(self, rng):
        sk = rng.randrange(self.r)
        return self.pk(sk), sk

    def message_on_curve(self, msg):
        data = b"".join(int(m).to_bytes(96, "little") for m in msg)
        return self.bh.evaluate(data)

    def prove_with(self, sk, pk, msg, r):
        """one attempt with nonce r: (gamma, c, s), or None where the reference draws again"""
        if r % self.r == 0:
            return None
        mh = self.message_on_curve(msg)
        gamma = mul(self.C, sk, mh)
        a, b = mul(self.C, r, self.G), mul(self.C, r, mh)
        c = self.H.evaluate(list(msg) + [coords(pk)[0], coords(a)[0], coords(b)[0]])
        if c >= BOUND:
            return None
        s = (r + sk * c) % self.r
        if s >= BOUND:
            return None
        return gamma, c, s

    def gamma_of(self, sk, msg):
        return mul(self.C, sk, self.message_on_curve(msg))

    def prove(self, sk, pk, msg, rng):
        while True:
            pr = self.prove_with(sk, pk, msg, rng.randrange(self.r))
            if pr:
                return pr

    def proof_to_hash(self, pk, msg, proof):
        """(status, output): status OK with the output, or FAILED / RANGE / GAMMA with None"""
        gamma, c, s = proof
        if c >= BOUND or s >= BOUND:
            return RANGE, None
        if not self.C.on_curve(gamma):
            return GAMMA, None
        mh = self.message_on_curve(msg)
        u = self.C.add(mul(self.C, s, self.G), self.C.neg(mul(self.C, c, pk)))
        v = self.C.add(mul(self.C, s, mh), self.C.neg(mul(self.C, c, gamma)))
        if self.H.evaluate(list(msg) + [coords(pk)[0], coords(u)[0], coords(v)[0]]) != c:
            return FAILED, None
        return OK, self.H.evaluate(list(msg) + list(coords(gamma)))

    def keyverify(self, pk):
        return self.C.on_curve(pk)

    # ABI conversions
    def fe(self, x):
        return pyref.int_to_limbs(self.F.to_mont(x % self.p))

    def sc(self, x):
        return pyref.int_to_limbs(self.R.to_mont(x % self.r))

    def pt_abi(self, P):
        """(24 limbs, infinity byte); infinity as zeros"""
        if P is None:
            return [0] * 24, 1
        return self.fe(P[0][0]) + self.fe(P[1][0]), 0

    def from_fe(self, limbs):
        return self.F.from_mont(pyref.limbs_to_int([int(v) for v in limbs]))

    def pt_from_abi(self, xy, inf):
        if inf:
            return None
        return ((self.from_fe(xy[:12]),), (self.from_fe(xy[12:24]),))


def random_point(curve, rng):
    return mul(curve, rng.randrange(1, curve.order), curve.G)


def make_bh(curve, rng, num_windows, window_size, recipe=True):
    """BH parameters: the reference's recipe from random segment bases, or independent random generators"""
    if recipe:
        return BoweHopwood(curve, recipe_generators(curve, [random_point(curve, rng) for _ in range(num_windows)], window_size))
    return BoweHopwood(curve, [[random_point(curve, rng) for _ in range(window_size)] for _ in range(num_windows)])


def rng(seed):
    return random.Random(seed)
