"""A Groth16 verifying key known in the exponent, over an engine object `pr` of tests/pairing_ref.py, as the device tests of
the verifiers share it (tests/test_gpu_pairing.py, tests/test_gpu_points.py).  Test infrastructure."""
import random

import numpy as np

import schnorr_ref


class ExpKey:
    """gamma_abc_g1 = [x0 G1 .. xn G1], alpha_g1_beta_g2 = e0^(alpha beta), gamma_g2 = gamma G2, delta_g2 = delta G2: for inputs
    s, g_ic = g G1 with g = x0 + s0 x1 + .. + s(n-1) xn, and (a G1, b G2, c G1) is valid iff a b = alpha beta + g gamma + c delta.
    The draws from random.Random(seed) are alpha, beta, gamma, delta and then the x_i; `rng` stays open for a user's own."""

    def __init__(self, pr, seed, n_inputs=2):
        self.pr, r = pr, pr.r
        self.rng = rng = random.Random(seed)
        self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(1, r) for _ in range(4))
        self.x = [rng.randrange(1, r) for _ in range(n_inputs + 1)]
        self.ab0 = self.alpha * self.beta % r
        C2 = pr.C2
        self.vk = {"alpha_g1_beta_g2": pr.fpow(pr.e0, self.ab0), "gamma_g2": C2.mul(self.gamma, C2.G), "delta_g2": C2.mul(self.delta, C2.G),
                   "gamma_abc_g1": [self.g1(v) for v in self.x]}

    def g1(self, k):
        """k G1, None for k = 0 (mod r)"""
        return schnorr_ref.mul(self.pr.C1, k % self.pr.r, self.pr.C1.G)

    def g_of(self, s):
        return (self.x[0] + sum(si * xi for si, xi in zip(s, self.x[1:]))) % self.pr.r

    def c_of(self, a, b, s):
        """the c that makes (a G1, b G2, c G1) valid for the inputs s"""
        r = self.pr.r
        return (a * b - self.ab0 - self.g_of(s) * self.gamma) * pow(self.delta, -1, r) % r

    def pvk(self, pairing, gt=None):
        """the package's PreparedVerifyingKey, with another alpha_g1_beta_g2 where gt is given"""
        pr, vk = self.pr, self.vk
        return pairing.PreparedVerifyingKey(pr.gt_row(gt if gt is not None else vk["alpha_g1_beta_g2"]), pr.g2_row(vk["gamma_g2"]),
                                            pr.g2_row(vk["delta_g2"]), np.stack([pr.g1_row(P) for P in vk["gamma_abc_g1"]]), engine=pr.name)

    def device_statuses(self, pvk, rows):
        """rows: (A, B, C, inputs) with pyref points -> the device's statuses"""
        pr = self.pr
        a_xy, a_inf = pr.g1_batch([row[0] for row in rows])
        for i, row in enumerate(rows):
            if row[0] is not None and not pr.C1.on_curve(row[0]):
                assert a_inf[i] == 0
        x = pr.input_rows([row[3] for row in rows])
        return [int(v) for v in pvk.verify((a_xy, a_inf), pr.g2_batch([row[1] for row in rows]), pr.g1_batch([row[2] for row in rows]), x)]
