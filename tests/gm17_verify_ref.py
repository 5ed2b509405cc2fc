"""What the GM17 verification tests share (tests/test_gm17_verify_host.py, tests/test_gpu_gm17_verify.py): a literal restatement
of proof-systems/src/gm17/verifier.rs:24-76 over an engine object `pr` of the pairing restatement (pairing_ref.engine("mnt4753")
or ("mnt6753")), a verifying key known in the exponent with its closed-form verdicts, and the edge rows every layer is checked
on.  Points are pyref's (None for infinity).  Test infrastructure."""
import random

import numpy as np


def on_curves(pr, proof):
    A, B, C = proof
    return pr.C1.on_curve(A) and pr.C2.on_curve(B) and pr.C1.on_curve(C)


def gm17_verify(pr, vk, proof, inputs):
    """verify_proof (verifier.rs:24-76), with the infinity rule of pr.product (a pair with a point at infinity contributes one)
    and the curves' own complete add.  vk: dict g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, h_g2, query.  None =
    MalformedVerifyingKey."""
    C1, C2 = pr.C1, pr.C2
    query = vk["query"]
    if len(inputs) + 1 != len(query):                                            # :29-31
        return None
    g_psi = query[0]                                                             # :36-39
    for x, b in zip(inputs, query[1:]):
        g_psi = C1.add(g_psi, C1.mul(x % pr.r, b))
    A, B, C = proof
    a_g_alpha = C1.add(A, vk["g_alpha_g1"])                                      # :41-43
    b_h_beta = C2.add(B, vk["h_beta_g2"])                                        # :45-47
    test1 = pr.product([(vk["g_alpha_g1"], vk["h_beta_g2"]),                     # test1_r1 (verifier.rs:14-16), :49-61
                        (C1.neg(a_g_alpha), b_h_beta), (g_psi, vk["h_gamma_g2"]), (C, vk["h_g2"])])
    test2 = pr.product([(A, vk["h_gamma_g2"]), (vk["g_gamma_g1"], C2.neg(B))])   # :65-73
    return test1 == pr.ONE and test2 == pr.ONE                                   # :75


class ExpKey:
    """g_alpha = alpha G, h_beta = beta H, g_gamma = gamma G, h_gamma = gamma H, h = H, query = [x0 G, x1 G, x2 G].  With
    psi = x0 + s0 x1 + s1 x2 the proof (a G, b H, c G) satisfies test1 iff (a + alpha)(b + beta) = alpha beta + psi gamma + c
    (mod r) and test2 iff a = b (gamma != 0); a point at infinity is the exponent 0."""

    def __init__(self, pr, seed, beta=None):
        self.pr = pr
        self.C1, self.C2, self.r = pr.C1, pr.C2, pr.r
        rng = random.Random(seed)
        self.alpha, self.beta, self.gamma = (rng.randrange(1, self.r) for _ in range(3))
        if beta is not None:
            self.beta = beta
        self.x = [rng.randrange(1, self.r) for _ in range(3)]
        self.vk = {"g_alpha_g1": self.g1(self.alpha), "h_beta_g2": self.g2(self.beta), "g_gamma_g1": self.g1(self.gamma),
                   "h_gamma_g2": self.g2(self.gamma), "h_g2": self.C2.G, "query": [self.g1(v) for v in self.x]}

    def g1(self, k):
        return self.C1.mul(k % self.r, self.C1.G)

    def g2(self, k):
        return self.C2.mul(k % self.r, self.C2.G)

    def psi(self, s):
        return (self.x[0] + s[0] * self.x[1] + s[1] * self.x[2]) % self.r

    def c_of(self, a, b, s):
        """the c that makes test1 hold"""
        return ((a + self.alpha) * (b + self.beta) - self.alpha * self.beta - self.psi(s) * self.gamma) % self.r

    def s1_of(self, a, b, c, s0):
        """the second input that makes test1 hold"""
        psi = ((a + self.alpha) * (b + self.beta) - self.alpha * self.beta - c) * pow(self.gamma, -1, self.r)
        return (psi - self.x[0] - s0 * self.x[1]) * pow(self.x[2], -1, self.r) % self.r

    def tests(self, a, b, c, s):
        """(test1, test2) in closed form"""
        return ((a + self.alpha) * (b + self.beta) - self.alpha * self.beta - self.psi(s) * self.gamma - c) % self.r == 0, (a - b) % self.r == 0

    def status(self, a, b, c, s):
        return int(all(self.tests(a, b, c, s)))

    def row(self, a, b, c, s):
        """the proof of the exponents (a, b, c) with the inputs s"""
        return (self.g1(a), self.g2(b), self.g1(c), list(s))


def edge_exponents(key):
    """the (a, b, c, inputs) of the edge rows that are on their curves, in the order of edge_rows"""
    r = key.r
    rng = random.Random(1700 + key.alpha % 1000)
    s = [rng.randrange(1, r), rng.randrange(1, r)]
    exps = []                                                                    # (a, b, c, inputs)
    for _ in range(2):                                                           # two valid proofs
        a = rng.randrange(1, r)
        exps.append((a, a, key.c_of(a, a, s), s))
    a0 = exps[0][0]
    exps.append((a0, a0, key.c_of(a0, a0, s) + 1, s))                            # C + G: test1 fails
    exps.append((a0, a0, key.c_of(a0, a0, s), [s[0], (s[1] + 1) % r]))           # a changed input
    b1 = rng.randrange(1, r)
    exps.append((a0, b1, key.c_of(a0, b1, s), s))                                # a != b, test1 holds: test2 fails
    for a in (key.alpha, key.beta):                                              # the G1 sum / the G2 sum is a doubling
        exps.append((a, a, key.c_of(a, a, s), s))
    na = -key.alpha % r
    exps.append((na, na, key.c_of(na, na, s), s))                                # S1 at infinity
    assert exps[-1][2] == (-key.alpha * key.beta - key.psi(s) * key.gamma) % r
    exps.append((na, na, key.c_of(na, na, s) + 1, s))                            # the same with C + G
    nb = -key.beta % r
    exps.append((nb, nb, key.c_of(nb, nb, s), s))                                # S2 at infinity
    exps.append((0, 0, key.c_of(0, 0, s), s))                                    # A and B at infinity
    assert exps[-1][2] == -key.psi(s) * key.gamma % r
    exps.append((0, 1, key.c_of(0, 1, s), s))                                    # A at infinity, B = H
    s_c = [s[0], key.s1_of(a0, a0, 0, s[0])]
    exps.append((a0, a0, 0, s_c))                                                # C at infinity, valid
    return exps


def edge_rows(key):
    """-> (rows (A, B, C, inputs), their closed-form statuses, the (test1, test2) of every row on its curves or None)"""
    C1, C2 = key.C1, key.C2
    exps = edge_exponents(key)
    s = exps[0][3]
    rows = [key.row(*e) for e in exps]
    tests = [key.tests(*e) for e in exps]
    assert rows[10][0] is None and rows[10][1] is None and rows[11][0] is None and rows[11][1] == C2.G and rows[12][2] is None
    assert rows[7][0] == C1.neg(key.vk["g_alpha_g1"]) and rows[9][1] == C2.neg(key.vk["h_beta_g2"])
    assert rows[5][0] == key.vk["g_alpha_g1"] and rows[6][1] == key.vk["h_beta_g2"]
    A, B, C, _ = rows[0]
    off1 = (A[0], ((A[1][0] + 1) % key.pr.p,))                                   # A off its curve
    off2 = (B[0], ((B[1][0] + 1) % key.pr.p,) + tuple(B[1][1:]))                 # B off its curve
    assert not C1.on_curve(off1) and not C2.on_curve(off2)
    rows += [(off1, B, C, list(s)), (A, off2, C, list(s))]
    tests += [None, None]
    expected = [2 if t is None else int(all(t)) for t in tests]
    assert expected == [1, 1, 0, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 2, 2]
    assert [t for t in tests if t is not None and not all(t)] == [(False, True), (False, True), (True, False), (False, True), (True, False)]
    return rows, expected, tests


# ---- the package's layouts
def pvk_of(gm17_verify_mod, key):
    """the package's PreparedVerifyingKey of an ExpKey (or of any vk dict of points)"""
    pr = key.pr
    vk = key.vk
    return gm17_verify_mod.PreparedVerifyingKey(pr.g1_row(vk["g_alpha_g1"]), pr.g2_row(vk["h_beta_g2"]), pr.g1_row(vk["g_gamma_g1"]),
                                                pr.g2_row(vk["h_gamma_g2"]), pr.g2_row(vk["h_g2"]),
                                                np.stack([pr.g1_row(P) for P in vk["query"]]), engine=pr.name)


def device_statuses(pr, pvk, rows):
    a, b, c = ([row[j] for row in rows] for j in range(3))
    st = pvk.verify(pr.g1_batch(a), pr.g2_batch(b), pr.g1_batch(c), pr.input_rows([row[3] for row in rows]))
    return [int(v) for v in st]
