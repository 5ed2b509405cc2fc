"""The Pedersen hash and commitment without a GPU: the Python restatement tests/pedersen_ref.py against a closed form, the
kernels' digit header (ginger-lib_amd/csrc/pedersen_digits.h compiled by g++, tests/host_shim/pedersen_shim.cpp) against the
restatement's bits, and the argument checks / exports of include/ginger_hip_pedersen.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import pedersen_ref
import pyref
import shim_build
from schnorr_ref import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_BAD_ARG, GH_E_UNSUPPORTED, GH_E_NO_DEVICE = -1, -2, -3
MNT4_G1, MNT4_G2, MNT6_G1, MNT6_G2 = 0, 1, 2, 3
CURVE_ID = {"mnt4753_g1": MNT4_G1, "mnt6753_g1": MNT6_G1}


# ---- 1. the restatement is pinned by a closed form
@pytest.mark.parametrize("cname", pedersen_ref.CURVES)
@pytest.mark.parametrize("wn", [(4, 5), (3, 7)])
def test_restatement_closed_form_with_recipe_generators(cname, wn):
    """with generators[i][j] = 2^j B_i and h_k = 2^k H: evaluate = sum m_i B_i, m_i the little-endian integer of window i's
    bits, and commit adds r H"""
    W, N = wn
    C = pyref.CURVES[cname]
    rng = pedersen_ref.rng(W * 100 + N + len(cname))
    bases = [pedersen_ref.random_point(C, rng) for _ in range(W)]
    H = pedersen_ref.random_point(C, rng)
    P = pedersen_ref.Pedersen(cname, pedersen_ref.recipe_generators(C, bases, N), pedersen_ref.generator_powers(C, H, pedersen_ref.RAND_BITS))
    G = W * N
    assert P.input_size_bits() == G
    for nbytes in range(G // 8 + 1):
        data = bytes(rng.randrange(256) for _ in range(nbytes))
        bits = pedersen_ref.bytes_to_bits(data) + [0] * (G - 8 * nbytes)
        want = None
        for i in range(W):
            m = sum(bit << j for j, bit in enumerate(bits[i * N:(i + 1) * N]))
            want = C.add(want, mul(C, m, bases[i]))
        assert P.evaluate(data) == want, nbytes
        assert P.evaluate(data + b"\x00" * (G // 8 - nbytes)) == want                 # zero padding changes nothing
        for r in (0, 1, rng.randrange(P.r), P.r - 1):
            assert P.commit(data, r) == C.add(want, mul(C, r, H)), (nbytes, r)
    assert P.evaluate(b"") is None
    with pytest.raises(ValueError):
        P.evaluate(b"\x00" * (G // 8 + 1))


# ---- 2. the digit header against the restatement
@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("pedersen")
    u64, ci, vp = ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p
    lib.t_ped_positions.argtypes, lib.t_ped_positions.restype = [u64, ci], u64
    lib.t_ped_row_positions.argtypes, lib.t_ped_row_positions.restype = [u64, ci], u64
    lib.t_ped_width.argtypes, lib.t_ped_width.restype = [u64, ci, u64], ci
    lib.t_ped_entry.argtypes, lib.t_ped_entry.restype = [ci, u64, ctypes.c_uint32], u64
    lib.t_ped_digits.argtypes, lib.t_ped_digits.restype = [vp, u64, u64, ci, vp], u64
    return lib


@pytest.mark.parametrize("t", [1, 2, 4, 8])
@pytest.mark.parametrize("G", [20, 21, 753])
def test_digits_rebuild_the_input_bits(shim, t, G):
    rng = pedersen_ref.rng(1000 * t + G)
    npos = -(-G // t)
    assert shim.t_ped_positions(G, t) == npos
    for p in range(npos):
        assert shim.t_ped_width(G, t, p) == min(t, G - p * t)
    if G % t:
        assert shim.t_ped_width(G, t, npos - 1) == G - t * (G // t)
    seen = set()
    for nbytes in range(G // 8 + 1):
        for data in (bytes(rng.randrange(256) for _ in range(nbytes)), b"\xff" * nbytes):
            row = np.frombuffer(data + b"\xa5", dtype=np.uint8).copy()              # one byte beyond the row: never read
            digits = np.full(npos, 0xFFFFFFFF, dtype=np.uint32)
            assert shim.t_ped_digits(row.ctypes.data, nbytes, G, t, digits.ctypes.data) == npos
            bits = pedersen_ref.bytes_to_bits(data) + [0] * (G - 8 * nbytes)
            got = []
            for p in range(npos):
                w = min(t, G - p * t)
                assert digits[p] < (1 << w), (nbytes, p)
                got += [(int(digits[p]) >> j) & 1 for j in range(w)]
            assert got == bits, nbytes
            # the positions the kernel visits hold every non-zero digit
            rp = shim.t_ped_row_positions(nbytes, t)
            assert rp == -(-8 * nbytes // t) and rp <= npos and not digits[rp:].any()
            seen |= {shim.t_ped_entry(t, p, int(d)) for p, d in enumerate(digits) if d}
    assert seen and max(seen) < npos * ((1 << t) - 1)
    assert shim.t_ped_entry(t, 0, 1) == 0 and shim.t_ped_entry(t, 1, 1) == (1 << t) - 1
    assert [bool(shim.t_ped_table_bits_ok(x)) for x in range(10)] == [x in (1, 2, 4, 8) for x in range(10)]


# ---- 3. symbols
def test_pedersen_symbols_exported_and_kept_apart(gl):
    from ginger_lib_amd import ecvrf, pedersen, poseidon, schnorr
    lib = gl.load_library()
    for s in pedersen.PEDERSEN_SYMBOLS:
        assert hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_pedersen.h")).read()
    assert sorted(re.findall(r"^int (gh_\w+)\(", hdr, re.M)) == sorted(pedersen.PEDERSEN_SYMBOLS)
    assert len(pedersen.PEDERSEN_SYMBOLS) == 7
    others = gl.ABI_SYMBOLS + gl.DIST_SYMBOLS + poseidon.POSEIDON_SYMBOLS + schnorr.SCHNORR_SYMBOLS + ecvrf.ECVRF_SYMBOLS
    import importlib
    for mod, name in (("pairing", "PAIRING_SYMBOLS"), ("gm17_verify", "GM17_SYMBOLS"), ("points", "POINTS_SYMBOLS"), ("r1cs", "R1CS_SYMBOLS"),
                      ("sap", "SAP_SYMBOLS")):
        others = others + list(getattr(importlib.import_module("ginger_lib_amd." + mod), name))
    assert not set(pedersen.PEDERSEN_SYMBOLS) & set(others)
    # and no other header declares one of them
    inc = os.path.join(ROOT, "include")
    for f in sorted(os.listdir(inc)):
        if f != "ginger_hip_pedersen.h":
            assert "gh_pedersen" not in open(os.path.join(inc, f)).read(), f


def test_package_pedersen_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "pedersen.py")).read()
    for needle in ("tests/", "import pyref", "schnorr_ref", "pedersen_ref", "oracle"):
        assert needle not in txt, needle


# ---- 4. argument checks that need no device
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pts(P, pts):
    xy = np.zeros((len(pts), 24), dtype=np.uint64)
    for i, Q in enumerate(pts):
        xy[i] = P.pt_abi(Q)[0]
    return xy


@pytest.fixture(scope="module")
def params():
    """per curve: (restatement with (W, N) = (4, 5) and recipe randomness generators, gen_xy, rand_xy)"""
    out = {}
    for cname in pedersen_ref.CURVES:
        P = pedersen_ref.make(cname, pedersen_ref.rng(len(cname)), 4, 5, recipe=True, commitment=True)
        out[cname] = (P, _pts(P, P.flat()), _pts(P, P.rand))
    return out


def test_create_checks_arguments(gl, params):
    from ginger_lib_amd import pedersen
    lib = pedersen._lib()
    err = lambda: lib.gh_last_error().decode()
    for cname, cid in CURVE_ID.items():
        P, g, r = params[cname]
        other = params[[c for c in CURVE_ID if c != cname][0]][1]
        h = ctypes.c_void_p()
        create = lambda gen=g, ginf=None, W=4, N=5, rand=r, rinf=None, nr=753, tb=0, curve=cid, out=ctypes.byref(h): lib.gh_pedersen_create(
            curve, None if gen is None else _p(gen), None if ginf is None else _p(ginf), W, N, None if rand is None else _p(rand),
            None if rinf is None else _p(rinf), nr, tb, out)
        for tb in (0, 1, 2, 4, 8):
            assert create(tb=tb) == 0 and h.value
            assert lib.gh_pedersen_free(h) == 0
        assert create(rand=None, nr=0) == 0 and h.value                              # a handle that only hashes
        assert lib.gh_pedersen_free(h) == 0
        for tb in (3, 5, 16, -1):
            assert create(tb=tb) == GH_E_BAD_ARG and not h.value
            assert "table_bits" in err()
        assert create(nr=752) == GH_E_BAD_ARG and "n_rand" in err()
        assert create(nr=754) == GH_E_BAD_ARG
        assert create(nr=0) == GH_E_BAD_ARG                                          # generators given, count 0
        assert create(rand=None, nr=753) == GH_E_BAD_ARG
        assert create(W=0) == GH_E_BAD_ARG and create(N=0) == GH_E_BAD_ARG
        assert "num_windows" in err()
        assert create(gen=None) == GH_E_BAD_ARG
        assert create(out=None) == GH_E_BAD_ARG
        assert create(curve=MNT4_G2) == GH_E_UNSUPPORTED and create(curve=MNT6_G2) == GH_E_UNSUPPORTED
        assert create(curve=9) == GH_E_BAD_ARG
        assert create(gen=other) == GH_E_BAD_ARG and "gen_xy" in err() and "curve" in err()   # not on that curve
        off = g.copy()
        off[3, 12:] = off[3, :12]
        assert create(gen=off) == GH_E_BAD_ARG and "gen_xy" in err() and "curve" in err()
        inf = np.zeros(20, dtype=np.uint8)
        inf[3] = 1
        assert create(gen=off, ginf=inf) == 0                                        # off the curve but at infinity
        assert lib.gh_pedersen_free(h) == 0
        bad = g.copy()
        bad[7, :12] = pyref.int_to_limbs(P.p)                                        # a coordinate equal to the modulus
        assert create(gen=bad) == GH_E_BAD_ARG and "gen_xy" in err() and "modulus" in err()
        inf[:] = 0
        inf[7] = 1
        assert create(gen=bad, ginf=inf) == GH_E_BAD_ARG                             # ... still checked at infinity
        roff = r.copy()
        roff[752, 12:] = roff[752, :12]
        assert create(rand=roff) == GH_E_BAD_ARG and "rand_xy" in err() and "curve" in err()
        rbad = r.copy()
        rbad[0, 12:] = pyref.int_to_limbs(P.p)
        assert create(rand=rbad) == GH_E_BAD_ARG and "rand_xy" in err() and "modulus" in err()
    assert lib.gh_pedersen_free(None) == 0
    with pytest.raises(pedersen.GingerHipError):
        pedersen.PedersenCRH("mnt4753_g1", params["mnt6753_g1"][1], None, 4, 5)
    with pytest.raises(ValueError):
        pedersen.PedersenCRH("mnt4753_g1", params["mnt4753_g1"][1], None, 4, 6)


def test_compute_entry_points_without_gpu(gl, params):
    """n == 0 is a no-op, an over-long input, a commitment on a handle without randomness generators and a randomness row at
    the modulus are GH_E_BAD_ARG before any device work, and without a device a valid call is GH_E_NO_DEVICE"""
    from ginger_lib_amd import pedersen
    lib = pedersen._lib()
    err = lambda: lib.gh_last_error().decode()
    P, g, r = params["mnt6753_g1"]
    H = pedersen.PedersenCRH("mnt6753_g1", g, None, 4, 5)
    K = pedersen.PedersenCommitment("mnt6753_g1", g, None, 4, 5, r, None, table_bits=4)
    assert H.input_size_bits == K.input_size_bits == 20
    x = np.zeros((4, 24), dtype=np.uint64)
    y = np.zeros(64, dtype=np.uint8)
    p, pb = _p(x), _p(y)
    for h in (H.handle, K.handle):
        assert lib.gh_pedersen_hash(h, pb, 0, 2, p, pb) == 0
        assert lib.gh_pedersen_hash_dev(h, pb, 0, 2, p, pb) == 0
        assert lib.gh_pedersen_hash(h, pb, 1, 3, p, pb) == GH_E_BAD_ARG              # 24 bits > G = 20
        assert "nbytes" in err()
        assert lib.gh_pedersen_hash_dev(h, pb, 1, 3, p, pb) == GH_E_BAD_ARG
        assert lib.gh_pedersen_hash(h, None, 1, 2, p, pb) == GH_E_BAD_ARG
        assert lib.gh_pedersen_hash(h, pb, 1, 2, None, pb) == GH_E_BAD_ARG
        assert lib.gh_pedersen_hash(h, pb, 1, 2, p, None) == GH_E_BAD_ARG
    assert lib.gh_pedersen_commit(K.handle, pb, 0, 2, p, p, pb) == 0
    assert lib.gh_pedersen_commit_dev(K.handle, pb, 0, 2, p, p, pb) == 0
    assert lib.gh_pedersen_commit(H.handle, pb, 1, 2, p, p, pb) == GH_E_BAD_ARG      # made without randomness generators
    assert "randomness" in err() and "rand_xy" in err()
    assert lib.gh_pedersen_commit_dev(H.handle, pb, 1, 2, p, p, pb) == GH_E_BAD_ARG
    assert lib.gh_pedersen_commit(H.handle, pb, 0, 2, p, p, pb) == GH_E_BAD_ARG      # whatever n is
    assert lib.gh_pedersen_commit(K.handle, pb, 1, 3, p, p, pb) == GH_E_BAD_ARG
    assert "nbytes" in err()
    assert lib.gh_pedersen_commit(K.handle, pb, 1, 2, None, p, pb) == GH_E_BAD_ARG
    rbad = np.zeros((1, 12), dtype=np.uint64)
    rbad[0] = pyref.int_to_limbs(P.r)                                                # the scalar field's modulus
    assert lib.gh_pedersen_commit(K.handle, pb, 1, 2, _p(rbad), p, pb) == GH_E_BAD_ARG
    assert "randomness" in err() and "modulus" in err()
    assert lib.gh_pedersen_hash(None, pb, 1, 2, p, pb) != 0
    t = (ctypes.c_float * 4)()
    assert lib.gh_pedersen_last_timing(t, 4, None) == 4
    # whether a device is usable is the library's own verdict (gh_init), not the framework's
    if lib.gh_init(None, 0) == GH_E_NO_DEVICE:
        e = GH_E_NO_DEVICE
        assert lib.gh_pedersen_hash(H.handle, pb, 1, 2, p, pb) == e
        assert lib.gh_pedersen_hash(H.handle, pb, 1, 0, p, pb) == e
        assert lib.gh_pedersen_hash_dev(K.handle, pb, 1, 2, p, pb) == e
        assert lib.gh_pedersen_commit(K.handle, pb, 1, 2, p, p, pb) == e
        assert lib.gh_pedersen_commit_dev(K.handle, pb, 1, 2, p, p, pb) == e
        with pytest.raises(pedersen.GingerHipError):
            H.evaluate(np.zeros((1, 2), dtype=np.uint8))
    H.close()
    K.close()
