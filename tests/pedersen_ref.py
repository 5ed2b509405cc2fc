"""Python restatement of the Pedersen hash and the Pedersen commitment over the MNT4-753 / MNT6-753 G1 groups (test
infrastructure), on top of pyref and schnorr_ref.mul.

Written from the definitions.  generators[num_windows][window_size] are taken as they are and flattened window-major into
g_0 .. g_(G-1).  The input bytes as bits, the least significant bit of each byte first:
    evaluate(input)  = sum over b < 8 len(input) of bit_b g_b        (the empty input hashes to infinity; 8 len > G is an error)
    commit(input, r) = evaluate(input) + sum over k < 753 of bit_k(r) h_k, bit_k of the canonical integer of r
The reference's recipe (setup): generators[i][j] = 2^j B_i and h_k = 2^k H for drawn bases B_i, H.
"""
import random

import pyref
from schnorr_ref import mul

RAND_BITS = 753
# group curve -> the pyref name of its scalar field
SCALAR_FIELD = {"mnt6753_g1": "p4", "mnt4753_g1": "p6"}
CURVES = list(SCALAR_FIELD)


def bytes_to_bits(data):
    return [(b >> i) & 1 for b in data for i in range(8)]


def generator_powers(curve, base, num_powers):
    out, P = [], base
    for _ in range(num_powers):
        out.append(P)
        P = curve.add(P, P)
    return out


def recipe_generators(curve, bases, window_size):
    return [generator_powers(curve, B, window_size) for B in bases]


class Pedersen:
    def __init__(self, cname, generators, randomness_generator=None):
        """generators: num_windows lists of window_size affine points (None = infinity); randomness_generator: 753 points"""
        self.cname = cname
        self.C = pyref.CURVES[cname]
        self.p = self.C.F.p
        self.r = self.C.order
        self.R = pyref.FIELDS[SCALAR_FIELD[cname]]
        assert self.R.p == self.r
        self.gens = generators
        self.num_windows, self.window_size = len(generators), len(generators[0])
        self.rand = randomness_generator
        assert randomness_generator is None or len(randomness_generator) == RAND_BITS

    def input_size_bits(self):
        return self.num_windows * self.window_size

    def flat(self):
        return [g for w in self.gens for g in w]

    def evaluate(self, data):
        if 8 * len(data) > self.input_size_bits():
            raise ValueError("input longer than the parameters take")
        flat = self.flat()
        acc = None
        for b, bit in enumerate(bytes_to_bits(data)):
            if bit:
                acc = self.C.add(acc, flat[b])
        return acc

    def commit(self, data, r):
        assert 0 <= r < self.r
        acc = self.evaluate(data)
        for k in range(RAND_BITS):
            if (r >> k) & 1:
                acc = self.C.add(acc, self.rand[k])
        return acc

    # ABI conversions
    def fe(self, x):
        return pyref.int_to_limbs(self.C.F.to_mont(x % self.p))

    def sc(self, x):
        return pyref.int_to_limbs(self.R.to_mont(x % self.r))

    def pt_abi(self, P):
        """(24 limbs, infinity byte); infinity as zeros"""
        if P is None:
            return [0] * 24, 1
        return self.fe(P[0][0]) + self.fe(P[1][0]), 0

    def from_fe(self, limbs):
        return self.C.F.from_mont(pyref.limbs_to_int([int(v) for v in limbs]))

    def pt_from_abi(self, xy, inf):
        if inf:
            return None
        return ((self.from_fe(xy[:12]),), (self.from_fe(xy[12:24]),))


def random_point(curve, rng):
    return mul(curve, rng.randrange(1, curve.order), curve.G)


def chain_points(curve, rng, count):
    """P, P + Q, P + 2 Q, ... for drawn P, Q: `count` points none of which is the double of the one before it"""
    P, Q = random_point(curve, rng), random_point(curve, rng)
    out = []
    for _ in range(count):
        out.append(P)
        P = curve.add(P, Q)
    return out


def make(cname, rng, num_windows, window_size, recipe=True, commitment=False):
    """parameters from drawn bases by the reference's recipe, or generators that follow no recipe (chain_points; and, for
    a commitment, 753 randomness generators of the same kind)"""
    C = pyref.CURVES[cname]
    if recipe:
        gens = recipe_generators(C, [random_point(C, rng) for _ in range(num_windows)], window_size)
        rand = generator_powers(C, random_point(C, rng), RAND_BITS) if commitment else None
    else:
        flat = chain_points(C, rng, num_windows * window_size)
        gens = [flat[i * window_size:(i + 1) * window_size] for i in range(num_windows)]
        rand = chain_points(C, rng, RAND_BITS) if commitment else None
    return Pedersen(cname, gens, rand)


def rng(seed):
    return random.Random(seed)
