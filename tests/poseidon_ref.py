"""Python restatement of Poseidon (T = 3, R = 2, inverse S-box) and of the field-based Merkle tree (test
infrastructure; the parameter data is tests/golden/poseidon_params.json).

Written from the function's definition, not from the reference's code: state of 3 canonical integers, rounds
R_F full / R_P partial / R_F full, constants 3 per round in order, S-box x -> x^-1 with 0 -> 0 (all three
elements in a full round, element 0 in a partial one), state <- M state after every round but the last.
evaluate(): state = AFTER_ZERO_PERM; per full pair add (a, b, C2) and permute; an odd leftover adds (a, 0, C2)
and permutes; return state[0].  The tree: L = next_pow2(n) leaves (missing ones = evaluate([1])), node i =
evaluate([2i+1, 2i+2]) in heap order, then HEIGHT - tree_height padding steps cur = evaluate([cur, empty]).
"""
import json
import os

import pyref

_HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS_JSON = os.path.join(_HERE, "golden", "poseidon_params.json")
FIELD_OF = {"mnt4753": pyref.P6, "mnt6753": pyref.P4}     # Fr of MNT4-753 is the MNT6-753 base prime and vice versa
FIELD_ID = {"mnt4753": 0, "mnt6753": 1}
KATS_JSON = os.path.join(_HERE, "golden", "poseidon_kats.json")


def load_params():
    return json.load(open(PARAMS_JSON))


def phantom_root_kat():
    """the one hash answer the reference ships (MNT4753_PHANTOM_MERKLE_ROOT; tests/golden/extract_poseidon_kats.py)
    -> (tag, the input element: the sentence zero-padded to 96 bytes and read little-endian, the answer's twelve ABI words)"""
    k = json.load(open(KATS_JSON))["mnt4753_phantom_merkle_root"]
    data = k["sentence"].encode("ascii")
    assert len(data) == 81 and k["input_bytes"] == 96
    x = int.from_bytes(data.ljust(96, b"\0"), "little")
    words = [int(w, 16) for w in k["words_montgomery_2p768"]]
    assert len(words) == 12 and x < FIELD_OF[k["tag"]].p
    return k["tag"], x, words


class Poseidon:
    def __init__(self, tag, params=None):
        d = (params or load_params())[tag]
        self.tag = tag
        self.F = F = FIELD_OF[tag]
        self.p = F.p
        self.r_f, self.r_p = d["r_f"], d["r_p"]
        self.rounds = 2 * self.r_f + self.r_p
        dec = lambda h: F.from_mont(int(h, 16))
        self.rc = [dec(h) for h in d["round_cst"]]
        self.mds = [dec(h) for h in d["mds"]]
        self.c2 = dec(d["c2"])
        self.azp = [dec(h) for h in d["after_zero_perm"]]
        self.raw = d

    def sbox(self, x):
        return pow(x, -1, self.p) if x else 0

    def perm(self, s):
        p = self.p
        s = [x % p for x in s]
        for r in range(self.rounds):
            s = [(s[j] + self.rc[3 * r + j]) % p for j in range(3)]
            if r < self.r_f or r >= self.r_f + self.r_p:
                s = [self.sbox(x) for x in s]
            else:
                s[0] = self.sbox(s[0])
            if r != self.rounds - 1:
                m = self.mds
                s = [(m[3 * i] * s[0] + m[3 * i + 1] * s[1] + m[3 * i + 2] * s[2]) % p for i in range(3)]
        return s

    def evaluate(self, inp):
        p = self.p
        s = list(self.azp)
        for i in range(0, len(inp) - 1, 2):
            s = self.perm([(s[0] + inp[i]) % p, (s[1] + inp[i + 1]) % p, (s[2] + self.c2) % p])
        if len(inp) % 2:
            s = self.perm([(s[0] + inp[-1]) % p, s[1], (s[2] + self.c2) % p])
        return s[0]

    def empty(self):
        return self.evaluate([1])

    def tree(self, leaves, height):
        """-> (tree in heap order, padding hashes, root); ValueError if the tree is taller than height."""
        L = 1
        while L < len(leaves):
            L *= 2
        th = L.bit_length()
        if th > height:
            raise ValueError("tree height %d > %d" % (th, height))
        e = self.empty()
        t = [e] * (2 * L - 1)
        t[L - 1:L - 1 + len(leaves)] = list(leaves)
        for i in range(L - 2, -1, -1):
            t[i] = self.evaluate([t[2 * i + 1], t[2 * i + 2]])
        pad, cur = [], t[0]
        for _ in range(height - th):
            cur = self.evaluate([cur, e])
            pad.append(cur)
        return t, pad, cur

    # ABI conversions (12 u64 limbs of the Montgomery form x 2^768)
    def to_abi(self, x):
        return pyref.int_to_limbs(self.F.to_mont(x))

    def from_abi(self, limbs):
        return self.F.from_mont(pyref.limbs_to_int([int(v) for v in limbs]))
