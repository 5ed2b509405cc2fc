"""One fixed sequence through the host layer of the library (keys, the key cache with and without GH_TEST_TABLE_NOMEM, a
fixed-base table, a chain key, transforms, the host-buffer entry points, trim, shutdown, a second init): free device memory in
MiB (torch.cuda.mem_get_info) after each step.  For comparing two trees (profiles/host_ownership_parity.md):
python tools/host_memory_sequence.py TREE OUT.json      (TREE: repository root whose built library is loaded)"""
import ctypes, json, os, sys
import numpy as np

TREE = os.path.abspath(sys.argv[1])
OUT = sys.argv[2]
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "tests"))
import torch
import pyref
import support as S
from __graft_entry__ import _load_pkg
gl = _load_pkg()
lib = gl.load_library()
steps = []


def mark(name, *results):
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0] >> 20
    steps.append([name, int(free)])
    print("%-60s %8d MiB" % (name, free), flush=True)


torch.cuda.init()
torch.zeros(1, device="cuda")
mark("before gh_init")
gl.init()
mark("gh_init")
curve = "mnt4753_g1"
C = pyref.CURVES[curve]
n = 1 << 20
prng = pyref.Rng(5)
xy, _ = S.bases_array(C, [C.mul(prng.next_u64() | 1, C.G), C.mul(prng.next_u64() | 1, C.G)])
rb = gl.ResidentBases.chain(curve, xy[0], xy[1], n)
bases = rb.download(0, n)
rb.free()
mark("chain key 2^20 generated, downloaded, freed", bases[:4], bases[-4:])
scalars = S.random_scalars_np(n, seed=9, below=C.order)
rb = gl.ResidentBases(curve, bases)
mark("2^20-base key uploaded")
rb.free()
mark("key freed")
for tag, nomem in (("", "0"), (" (GH_TEST_TABLE_NOMEM=1)", "1")):
    os.environ["GH_TEST_TABLE_NOMEM"] = nomem
    for i in range(3):
        out = gl.msm_cached(curve, bases, scalars)
        mark("gh_msm_cached %d%s" % (i + 1, tag), out)
    st = gl.KeyCacheStats()
    lib.gh_key_cache_stats(ctypes.byref(st))
    steps.append(["key cache stats" + tag, {k: int(getattr(st, k)) for k, _ in st._fields_}])
    gl.key_cache_clear()
    mark("gh_key_cache_clear" + tag)
os.environ["GH_TEST_TABLE_NOMEM"] = "0"
aff = gl.VariableBaseMSM.multi_scalar_mul(curve, bases[:1], np.array([[1] + [0] * 11], np.uint64))   # 1 * P_0 as a projective point
fb = gl.FixedBaseMSM(curve, aff, 753, window=14)
mark("fixed-base table created")
fo = fb.multi_scalar_mul(scalars[:1 << 16])
mark("fixed-base msm 2^16", fo)
fb.free()
mark("fixed-base table freed")
rb = gl.ResidentBases.chain(curve, xy[0], xy[1], n)
mark("chain key generated")
rb.free()
mark("chain key freed")
F = "mnt4753_fr"
dom = gl.EvaluationDomain(F, n)
rows = S.random_scalars_np(n, seed=21, below=pyref.P6.p)
o = dom.fft(rows)
mark("gh_fft 2^20", o)
o = dom.coset_fft(rows)
mark("gh_fft 2^20 coset", o)
o = dom.coset_ifft(rows)
mark("gh_fft 2^20 coset inverse", o)
m = 1 << 16
a, b, c = rows[:m], rows[m:2 * m], rows[2 * m:3 * m]
z = np.zeros(12, np.uint64)
mark("gh_witness_map 2^16", gl.witness_map(F, a, b, c, z, z, z))
mark("gh_sap_witness_map 2^16", gl.sap_witness_map(F, a, c, z, z))
mark("gh_batch_inverse 2^16", gl.batch_inversion(F, a))
mark("gh_lagrange_coefficients 2^16", gl.evaluate_all_lagrange_coefficients(F, 16, rows[5]))
mark("gh_vec_mul 2^16", gl.EvaluationDomain(F, m).mul_polynomials_in_evaluation_domain(a, b))
mark("gh_vec_scale 2^16", gl.vec_scale(F, a, rows[7]))
gl.dev_trim()
mark("gh_dev_trim")
gl.shutdown()
mark("gh_shutdown")
gl.init()
out = gl.VariableBaseMSM.multi_scalar_mul(curve, bases[:4096], scalars[:4096])
mark("gh_init again + gh_msm 2^12", out)
gl.shutdown()
mark("gh_shutdown again")
with open(OUT, "w") as f:
    json.dump({"tree": TREE, "steps": steps}, f, indent=1)
