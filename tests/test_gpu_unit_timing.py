"""What every unit's *_last_timing reports after one call, and that a unit's record is its own: no other unit's call, no
transform inside its phases and no gh_shutdown / gh_init changes what it means.  Every unit times with a PhaseTimer of
ginger-lib_amd/csrc/unit_host.h that owns its events.  The calls use 65 rows (more than a block of 64) or
r1cs_ref.hand_built_system; what they compute is checked by each unit's own device tests, here only the timing records are
read, so the inputs are whatever is cheapest to make: generator multiples from the device, random rows below the modulus."""
import importlib

import numpy as np
import pytest

import gm17_verify_ref
import pairing_ref
import poseidon_ref
import pyref
import r1cs_ref
import schnorr_ref
from groth16_exp_key import ExpKey

pytestmark = pytest.mark.gpu

N = 65
ENGINE = "mnt4753"                                         # the verifiers' calls; the bare pairing runs on both engines
TAG, CURVE = schnorr_ref.SCHEMES["SchnorrMNT4"]            # Poseidon over MNT4-753's Fr, the group MNT6-753 G1
R1CS_MODULUS = pyref.P6.p                                  # Fr of the "mnt4753" pairing


def below_modulus(rng, n, words=12):
    """n rows of `words` limbs, every field element below 2^744: a valid row of either field in any form"""
    a = rng.integers(0, 1 << 63, size=(n, words), dtype=np.uint64)
    a[:, 11::12] &= np.uint64((1 << 40) - 1)
    return a


def mont(vals, r):
    R = (1 << 768) % r
    return np.array([pyref.int_to_limbs(v * R % r) for v in vals], dtype=np.uint64).reshape(-1, 12)


class Unit:
    """one timed call of a unit and how to read its record: names of the phases (None: the count comes from `count`), the
    phases the call runs, and whether the others must be zero (the calls that time one phase only)"""

    def __init__(self, call, read, phases, ran, count=None, others_zero=False):
        self.call, self.read, self.phases, self.ran, self.count, self.others_zero = call, read, phases, ran, count, others_zero

    def record(self):
        ms, total = self.read()
        if isinstance(ms, dict):
            assert list(ms) == self.phases
            ms = [ms[p] for p in self.phases]
        return list(ms), total

    def check(self):
        ms, total = self.record()
        want = len(self.phases) if self.phases is not None else self.count()
        assert len(ms) == want, (len(ms), want)
        assert all(v >= 0 for v in ms) and total > 0, (ms, total)
        ran = [self.phases.index(p) if isinstance(p, str) else p % want for p in self.ran]
        assert all(ms[i] > 0 for i in ran), ms
        if self.others_zero:
            assert all(ms[i] == 0 for i in range(want) if i not in ran), ms
        return ms, total


@pytest.fixture(scope="module")
def units(gpu):
    mods = {m: importlib.import_module("ginger_lib_amd." + m)
            for m in ("schnorr", "ecvrf", "poseidon", "pairing", "gm17_verify", "points", "pedersen", "r1cs", "sap", "poly")}
    schnorr, ecvrf, poseidon, pairing, gv, points, pedersen, r1cs, sap, poly = (mods[m] for m in mods)
    rng = np.random.default_rng(65)
    out, closers = {"mods": mods}, []

    # Schnorr verify: every phase runs.  The keys are sk G from the device; the signatures are random rows (status 0)
    prm = poseidon.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, TAG)
    scheme = schnorr.FieldBasedSchnorrSignatureScheme(prm, CURVE)
    closers += [scheme.close, prm.close]
    pk = scheme.get_public_key(below_modulus(rng, N))
    msg, sig = below_modulus(rng, N).reshape(N, 1, 12), below_modulus(rng, N, 24)
    out["schnorr"] = Unit(lambda: scheme.verify(pk, msg, sig), schnorr.last_timing, schnorr.PHASES, schnorr.PHASES)
    out["prm"] = prm

    # EC-VRF's joint multiplication: one bracket, the variable-base phase alone
    k = below_modulus(rng, N)
    out["ecvrf"] = Unit(lambda: ecvrf.batch_double_mul(CURVE, pk[0], k, pk[0], k), ecvrf.last_timing, ecvrf.PHASES, ["variable_base"],
                        others_zero=True)

    # Poseidon: a tree of 65 leaves with every level on the device (host_tail_nodes 0): seven bracketed levels, then the padding
    leaves = below_modulus(rng, N)

    def tree():
        poseidon.set_tuning(0, 0)
        try:
            poseidon.FieldBasedMerkleHashTree(prm, 9, leaves)
        finally:
            poseidon.set_tuning(0, None)
    out["poseidon"] = Unit(tree, poseidon.last_timing, None, range(7), count=lambda: 8)

    # the bare pairing on each engine: no g_ic and no compare phase
    for name in pairing_ref.ENGINES:
        pr = pairing_ref.engine(name)
        g1, g2 = pr.g1_batch([pr.C1.G] * N), pr.g2_batch([pr.C2.G] * N)
        out["pairing_" + name] = Unit(lambda g1=g1, g2=g2, name=name: pairing.pairing_product(g1, g2, 1, engine=name), pairing.last_timing,
                                      pairing.PHASES, ["upload", "miller", "final_exp", "download"], others_zero=True)

    # GM17 verify: all nine phases
    pr = pairing_ref.engine(ENGINE)
    gkey = gm17_verify_ref.ExpKey(pr, 1711)
    grow = gkey.row(*gm17_verify_ref.edge_exponents(gkey)[0])
    gpvk = gm17_verify_ref.pvk_of(gv, gkey)
    closers.append(gpvk.close)
    out["gm17"] = Unit(lambda: gm17_verify_ref.device_statuses(pr, gpvk, [grow] * N), gv.last_timing, gv.PHASES, gv.PHASES)

    # points: membership of 65 points of G1
    member = pr.g1_batch([pr.C1.G] * N)
    out["points"] = Unit(lambda: points.group_membership_test(ENGINE + "_g1", member), points.last_timing, points.PHASES, points.PHASES)

    # Pedersen: 2 windows of 8 generators (powers of two device-made bases), rows of two bytes
    gxy, ginf = pedersen.create_generators(CURVE, pk[0][:2], 8)
    crh = pedersen.PedersenCRH(CURVE, gxy, ginf, 2, 8)
    closers.append(crh.close)
    data = rng.integers(0, 256, size=(N, 2), dtype=np.uint8)
    out["pedersen"] = Unit(lambda: crh.evaluate(data), pedersen.last_timing, pedersen.PHASES, pedersen.PHASES)

    # R1CS / SAP witness maps over the hand-built system at segment length 4: conversion, the levels, what follows the products
    lcs = r1cs_ref.hand_built_system(R1CS_MODULUS)
    h = r1cs.ResidentR1CS(gpu, ENGINE, lcs, segment_terms=4)
    closers.append(h.free)
    d_z = gpu.DeviceBuffer(h.num_variables * 96).upload(mont(r1cs_ref.hand_built_vector(h.num_variables, R1CS_MODULUS), R1CS_MODULUS))
    dd = below_modulus(rng, 3)
    d_h = gpu.DeviceBuffer((h.size + 1) * 96)
    sap_size = sap.sap_info(h)["size"]
    d_sh = gpu.DeviceBuffer((sap_size + 1) * 96)
    levels = lambda: max(v for per in h.info()["levels"].values() for v in per) + 2
    out["r1cs"] = Unit(lambda: h.witness_map_dev(d_z, dd, d_h), r1cs.last_timing, None, [0, 1, -1], count=levels)
    out["sap"] = Unit(lambda: sap.sap_witness_map_dev(h, d_z, dd[:2], d_sh), sap.last_timing, None, [0, 1, -1], count=levels)

    # polynomials: one bracket, one number
    f = poly.DensePolynomial.from_coefficients("mnt4753_fr", list(range(1, N + 1)))
    out["poly"] = Unit(lambda: f.evaluate(3), lambda: ([poly.last_timing()], poly.last_timing()), None, [0], count=lambda: 1)

    # validated verification of compressed proofs: the points unit's validate bracket inside the pairing unit's phases
    K = ExpKey(pr, 1965)
    s = [K.rng.randrange(1, pr.r), K.rng.randrange(1, pr.r)]
    a, b = K.rng.randrange(1, pr.r), K.rng.randrange(1, 1 << 20)
    proof = [pr.g1_batch([K.g1(a)] * N), pr.g2_batch([pr.C2.mul(b, pr.C2.G)] * N), pr.g1_batch([K.g1(K.c_of(a, b, s))] * N)]
    wire = [points.compress_limbs("%s_g%d" % (ENGINE, 2 if j == 1 else 1), p) for j, p in enumerate(proof)]
    pvk = K.pvk(pairing)
    closers.append(pvk.close)
    inputs = pr.input_rows([s] * N)

    def verify_compressed():
        st, pst = pvk.verify_compressed(wire[0], wire[1], wire[2], inputs)
        assert st.tolist() == [1] * N and not pst.any()
    out["verify_compressed"] = Unit(verify_compressed, points.last_timing, points.PHASES, ["validate"], others_zero=True)
    out["hash"] = lambda: poseidon.PoseidonHash(prm).evaluate_many(below_modulus(rng, N, 24).reshape(N, 2, 12))
    yield out
    for close in reversed(closers):
        close()


UNITS = ["schnorr", "ecvrf", "poseidon", "pairing_mnt4753", "pairing_mnt6753", "gm17", "points", "pedersen", "r1cs", "sap", "poly",
         "verify_compressed"]


@pytest.mark.parametrize("name", UNITS)
def test_record_after_one_call(units, name):
    """the phase count, every phase >= 0, the phases that ran > 0, the total > 0"""
    units[name].call()
    units[name].check()


def test_verify_compressed_leaves_the_pairing_phases_to_the_pairing_unit(units):
    units["verify_compressed"].call()
    ptm, total = units["mods"]["pairing"].last_timing()
    assert all(ptm[ph] > 0 for ph in ("upload", "g_ic", "miller", "final_exp", "compare", "download")) and total > 0


def test_schnorr_record_survives_a_merkle_tree(units):
    """a Schnorr verify, a Poseidon Merkle tree of 8 leaves, then the Schnorr record: what it was"""
    poseidon = units["mods"]["poseidon"]
    units["schnorr"].call()
    before = units["schnorr"].check()
    poseidon.set_tuning(0, 0)                              # every level of the small tree on the device, each inside its own bracket
    try:
        poseidon.FieldBasedMerkleHashTree(units["prm"], 4, below_modulus(np.random.default_rng(8), 8))
    finally:
        poseidon.set_tuning(0, None)
    levels, _ = poseidon.last_timing()
    assert len(levels) == 4 and all(v > 0 for v in levels[:3])
    assert units["schnorr"].record() == before


def test_witness_map_phases_sum_to_the_total(units):
    """the witness maps run transforms inside their last phase; the record still is the unit's own intervals.  The phases and the
    total are sums of the same float32 intervals, fewer than 64 of them, in two orders: they agree to 64 * 2^-24 < 1e-5"""
    for name in ("r1cs", "sap"):
        units[name].call()
        ms, total = units[name].check()
        assert sum(ms) == pytest.approx(total, rel=1e-5), (name, ms, total)


def test_validate_phase_survives_a_hash(units):
    """gh_groth16_verify_compressed, a Poseidon hash, then gh_points_last_timing: the validate phase is still that call's"""
    units["verify_compressed"].call()
    before = units["verify_compressed"].check()
    assert before[1] == before[0][1]                       # the total of the validate bracket is the bracket
    units["hash"]()
    assert units["verify_compressed"].record() == before


def test_every_timer_works_after_shutdown_and_init(units, gpu):
    """gh_shutdown destroys every timer's events and resets it; after gh_init each unit's next call makes its own again"""
    gpu.shutdown()
    gpu.init()
    for name in UNITS:
        units[name].call()
        units[name].check()
