"""Poseidon without a GPU: the parameter fixture against the Python restatement, the GH_HD permutation of
ginger-lib_amd/csrc/poseidon_perm.h compiled by g++ (tests/host_shim/poseidon_shim.cpp) against the restatement at
every K and in both stores, and the argument checks / exports of include/ginger_hip_poseidon.h."""
import ctypes
import re
import os
import random
import subprocess

import numpy as np
import pytest

import poseidon_ref
import pyref
import shim_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["mnt4753", "mnt6753"]
U = ctypes.c_uint32
GH_E_BAD_ARG, GH_E_NO_DEVICE = -1, -3


@pytest.fixture(scope="module")
def shim():
    lib = shim_build.host_shim("poseidon")
    lib.t_poseidon_perm.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def refs():
    return {t: poseidon_ref.Poseidon(t) for t in TAGS}


def abi_words(P, vals):
    out = np.zeros(len(vals) * 24, dtype=np.uint32)
    for i, v in enumerate(vals):
        m = P.F.to_mont(v % P.p)
        out[24 * i:24 * i + 24] = [(m >> (32 * j)) & 0xFFFFFFFF for j in range(24)]
    return out


def from_words(P, w):
    return [P.F.from_mont(sum(int(x) << (32 * j) for j, x in enumerate(w[24 * i:24 * i + 24]))) for i in range(len(w) // 24)]


def const_words(P):
    n = 3 * P.rounds
    return abi_words(P, P.rc[:n] + P.mds + [P.c2] + P.azp)


def shim_perm(shim, P, states, k, slab):
    cst = const_words(P)
    flat = [x for s in states for x in s]
    w = abi_words(P, flat)
    fid = 6 if P.F is pyref.P6 else 4
    assert shim.t_poseidon_perm(fid, k, slab, P.r_f, P.r_p, cst.ctypes.data, w.ctypes.data) == 0
    out = from_words(P, w)
    return [out[3 * i:3 * i + 3] for i in range(len(states))]


def crafted(P, rng):
    """states whose first-round S-box inputs are zero: one, two and all three elements equal to -round_cst"""
    p = P.p
    neg = [(-P.rc[e]) % p for e in range(3)]
    r = lambda: rng.randrange(p)
    return [[neg[0], r(), r()], [r(), neg[1], r()], [r(), r(), neg[2]], [neg[0], neg[1], r()], [neg[0], r(), neg[2]], neg[:]]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_after_zero_perm(refs, tag):
    P = refs[tag]
    assert P.perm([0, 0, 0]) == P.azp
    assert (P.r_f, P.r_p) == {"mnt4753": (4, 57), "mnt6753": (2, 60)}[tag]
    assert len(P.rc) == 195 and len(P.mds) == 9


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_words_are_the_reference_montgomery_form(refs, tag):
    P = refs[tag]
    assert P.c2 == 3                         # C2 is the field element 3 (mod.rs evaluate: "add the constant 3")
    for h in P.raw["round_cst"] + P.raw["mds"] + P.raw["after_zero_perm"] + [P.raw["c2"]]:
        assert int(h, 16) < P.p


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("k,slab", [(1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (4, 1), (8, 1)])
def test_host_permutation_matches_restatement(shim, refs, tag, k, slab):
    P = refs[tag]
    rng = random.Random(1000 * k + slab + len(tag))
    p = P.p
    pool = [[0, 0, 0], [1, 1, 1], [p - 1, p - 1, p - 1], [0, 1, p - 1]] + crafted(P, rng) + \
           [[rng.randrange(p) for _ in range(3)] for _ in range(2)]
    # every state of the pool once in every position of a batch of k (a crafted state also as the batch's last)
    batches = []
    for i, s in enumerate(pool):
        b = [[rng.randrange(p) for _ in range(3)] for _ in range(k)]
        b[i % k] = s
        batches.append(b)
        if k > 1:
            b2 = [[rng.randrange(p) for _ in range(3)] for _ in range(k)]
            b2[-1] = s
            batches.append(b2)
    batches.append([pool[4 + (j % 6)] for j in range(k)])     # a batch of crafted states only
    for b in batches:
        assert shim_perm(shim, P, b, k, slab) == [P.perm(s) for s in b]


def test_restatement_reproduces_the_reference_phantom_merkle_root(refs):
    """evaluate() against the one hash answer the reference ships (after_zero_perm anchors the permutation only)"""
    tag, x, words = poseidon_ref.phantom_root_kat()
    P = refs[tag]
    assert P.to_abi(P.evaluate([x])) == words
    assert P.evaluate([x]) == P.from_abi(words) != P.evaluate([x, 1])


@pytest.mark.parametrize("k,slab", [(1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (4, 1), (8, 1)])
def test_host_permutation_reproduces_the_reference_phantom_merkle_root(shim, refs, k, slab):
    """the same answer through the g++ build of the permutation: evaluate([x]) is element 0 of perm(after_zero_perm + (x, 0, C2));
    the state in every position of a batch of k"""
    tag, x, words = poseidon_ref.phantom_root_kat()
    P = refs[tag]
    state = [(P.azp[0] + x) % P.p, P.azp[1], (P.azp[2] + P.c2) % P.p]
    rng = random.Random(40 + k)
    for at in range(k):
        b = [[rng.randrange(P.p) for _ in range(3)] for _ in range(k)]
        b[at] = state
        assert P.to_abi(shim_perm(shim, P, b, k, slab)[at][0]) == words, (k, slab, at)


def test_poseidon_symbols_exported_and_kept_apart(gl):
    from ginger_lib_amd import poseidon
    lib = gl.load_library()
    for s in poseidon.POSEIDON_SYMBOLS:
        assert hasattr(lib, s), s
    assert not set(poseidon.POSEIDON_SYMBOLS) & set(gl.ABI_SYMBOLS + gl.DIST_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "ginger_hip_poseidon.h")).read()
    import re
    declared = re.findall(r"^int (gh_\w+)\(", hdr, re.M)
    assert sorted(declared) == sorted(poseidon.POSEIDON_SYMBOLS)


def _params(tag):
    from ginger_lib_amd import poseidon
    return poseidon.PoseidonParameters.from_json(poseidon_ref.PARAMS_JSON, tag)


def test_create_checks_arguments(gl):
    from ginger_lib_amd import poseidon
    lib = poseidon._lib()
    d = poseidon_ref.load_params()["mnt4753"]
    rc = poseidon._hex_rows(d["round_cst"])
    mds, c2, azp = poseidon._hex_rows(d["mds"]), poseidon._hex_rows([d["c2"]]), poseidon._hex_rows(d["after_zero_perm"])
    h = ctypes.c_void_p()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gh_poseidon_create(0, 4, 57, P(rc), 195, P(mds), P(c2), P(azp), ctypes.byref(h)) == 0 and h.value
    assert lib.gh_poseidon_free(h) == 0
    assert lib.gh_poseidon_create(0, 0, 57, P(rc), 195, P(mds), P(c2), P(azp), ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_poseidon_create(0, 4, 57, P(rc), 194, P(mds), P(c2), P(azp), ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_poseidon_create(0, 4, 57, None, 195, P(mds), P(c2), P(azp), ctypes.byref(h)) == GH_E_BAD_ARG
    assert lib.gh_poseidon_create(0, 4, 57, P(rc), 195, P(mds), P(c2), P(azp), None) == GH_E_BAD_ARG
    bad = mds.copy()
    bad[4] = pyref.int_to_limbs(pyref.P6.p)                 # == p: not below the modulus
    assert lib.gh_poseidon_create(0, 4, 57, P(rc), 195, P(bad), P(c2), P(azp), ctypes.byref(h)) == GH_E_BAD_ARG
    assert "modulus" in lib.gh_last_error().decode()
    assert lib.gh_poseidon_set_tuning(3, 0) == GH_E_BAD_ARG
    assert lib.gh_poseidon_set_tuning(0, (1 << 64) - 1) == 0


def test_compute_entry_points_without_gpu(gl):
    """n == 0 is a no-op everywhere; on a machine without a device every compute entry point fails with GH_E_NO_DEVICE."""
    from ginger_lib_amd import poseidon
    lib = poseidon._lib()
    prm = _params("mnt4753")
    x = np.zeros((4, 12), dtype=np.uint64)
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert lib.gh_poseidon_hash(prm.handle, p, 0, 2, p) == 0
    assert lib.gh_poseidon_permute(prm.handle, p, 0) == 0
    assert lib.gh_poseidon_merkle_verify(prm.handle, p, p, p, 0, 4, p, p) == 0
    assert lib.gh_poseidon_merkle_tree(prm.handle, p, 4, 2, None, None, p) == GH_E_BAD_ARG      # 4 leaves need height 3
    assert lib.gh_poseidon_merkle_verify(prm.handle, p, p, p, 1, 1, p, p) == GH_E_BAD_ARG      # an empty path
    # whether a device is usable is the library's own verdict (gh_init), not the framework's
    expect = GH_E_NO_DEVICE if lib.gh_init(None, 0) == GH_E_NO_DEVICE else 0
    assert lib.gh_poseidon_hash(prm.handle, p, 1, 2, p) == expect
    assert lib.gh_poseidon_permute(prm.handle, p, 1) == expect
    assert lib.gh_poseidon_merkle_tree(prm.handle, p, 4, 3, None, None, p) == expect
    if expect == GH_E_NO_DEVICE:
        with pytest.raises(poseidon.GingerHipError):
            poseidon.PoseidonHash(prm).evaluate(x[:2])
        with pytest.raises(poseidon.GingerHipError):
            poseidon.FieldBasedMerkleHashTree(prm, 4, x)


def test_package_poseidon_module_has_no_test_dependency():
    txt = open(os.path.join(ROOT, "ginger-lib_amd", "poseidon.py")).read()
    assert "tests/" not in txt and "import pyref" not in txt and "poseidon_ref" not in txt and "oracle" not in txt


# ---- the Rust side (delivered as files: no Rust toolchain checks them here)
RUST_SRC = os.path.join(ROOT, "rust", "algebra-hip-sys", "src")
PRIM_PATCH = os.path.join(ROOT, "rust", "patches", "primitives-gpu-feature.patch")


def test_rust_poseidon_extern_block_is_generated_from_the_header():
    import re
    import sys
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0
    rs = open(os.path.join(RUST_SRC, "poseidon.rs")).read()
    block = rs[rs.index("// ---- GENERATED by"):rs.index("// ---- GENERATED: end")]
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (gh_\w+)\((.*?)\)", block)}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ginger_hip_poseidon.h")).read(), flags=re.S)
    c = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(gh_\w+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)}
    assert sorted(rust) == sorted(c) and len(c) == 9
    for name, params in c.items():
        assert params.count(",") == rust[name].count(","), name
    lib = open(os.path.join(RUST_SRC, "lib.rs")).read()
    assert "pub mod poseidon;" in lib[lib.index("// ---- GENERATED: end"):]
    assert "gh_poseidon" not in lib                      # the crate's main extern block stays the two headers


def test_primitives_patch_hooks_both_entry_points_without_unsafe():
    p = open(PRIM_PATCH).read()
    for needle in ("primitives/Cargo.toml", 'gpu = ["algebra-hip-sys"]', "primitives/src/crh/poseidon/mod.rs",
                   "gpu::batch_evaluate_2_1::<F, P>(input_array)", "primitives/src/merkle_tree/field_based_mht/mod.rs",
                   "gpu_merkle_tree(leaves, P::HEIGHT)", "primitives/src/crh/poseidon/gpu.rs", "primitives/src/crh/mod.rs",
                   "P::ROUND_CST", "P::MDS_CST", "P::C2", "P::AFTER_ZERO_PERM", "mnt4753::Fr", "mnt6753::Fr", "P::T != 3"):
        assert needle in p, needle
    added = "\n".join(l[1:] for l in p.split("\n") if l.startswith("+") and not l.startswith("+++"))
    code = re.sub(r"//[^\n]*", "", added)
    assert "unsafe" not in code and "transmute" not in code
    # every device call falls back: the hooks return to the CPU code unless the dispatch reports success
    assert "if gpu::batch_evaluate_2_1::<F, P>(input_array) {\n+                return;" in p
    assert "if let Some((tree, padding_tree, root))" in p
