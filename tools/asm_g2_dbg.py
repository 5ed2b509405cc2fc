"""stage markers of the debug build of a G2 round kernel (GH_ASM_DEBUG=1 python -m asmgen.build build/dbg): development only.
Runs the inputs of tests/test_asmgen_g2.py through the kernels of build/dbg/gh_asm.hsaco on the card (tests/asm_card.py is the
HIP binding; the card-against-simulator comparison itself is tests/test_gpu_asm_sim.py) and prints the flag words."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "ginger-lib_amd"))
import asm_card
import test_asmgen_g2 as T
card = asm_card.Card()
module = card.load(os.path.join(ROOT, "build", "dbg", "gh_asm.hsaco"))
NAME = {}
for fwd in (True, False):
    for r0 in (True, False):
        g, _ = T._prog("mnt4753_g2", fwd, r0)
        NAME[g.name] = "gh_asm_aff_f2_%s_%s" % ("fwd" if fwd else "bwd", "r0" if r0 else "rn")
g, _ = T._prog("mnt4753_g2", False, True)
NAME[g.name] += "_dbg"

def runner(g, bufs, scalars, waves):
    dev = {k: card.malloc(v.nbytes) for k, v in bufs.items()}
    for k, v in bufs.items():
        card.upload(dev[k], np.ascontiguousarray(v))
    karg = np.zeros(22, dtype=np.uint32)
    for j, k in enumerate(T.ARG_ORDER):
        karg[2 * j], karg[2 * j + 1] = dev[k] & 0xFFFFFFFF, dev[k] >> 32
    karg[18], karg[19], karg[20] = scalars
    card.launch(card.function(module, NAME[g.name]), ((waves + 1 + 3) // 4, 1), 256, karg)
    for k in T.WRITABLE:
        got = np.empty(bufs[k].size, dtype=np.uint32)
        card.download(dev[k], got)
        bufs[k][...] = got.reshape(bufs[k].shape)
    for d in dev.values():
        card.free(d)
    print(NAME[g.name], "flag words", [int(x) for x in bufs["flag"]])
orig = T._run_round
def patched(*a, **k):
    k["runner"] = runner
    return orig(*a, **k)
T._run_round = patched
try:
    T.test_g2_round_kernels_in_the_simulator("mnt4753_g2")
except AssertionError as e:
    print("assert", str(e)[:100])
card.close()
