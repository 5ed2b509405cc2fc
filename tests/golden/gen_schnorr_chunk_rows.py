"""Writes schnorr_chunk_rows.json: for either scheme, 261 field-based Schnorr signatures made by the restatement
tests/schnorr_ref.py (Schnorr.sign_with), for the slab-chunk test of tests/test_gpu_schnorr.py.  A Poseidon hash of the restatement
takes 20 ms and two nonces in three are rejected, so the test reads the signatures instead of making them.

Row i has the secret key sk0 + i (its public key is pk0 + i G: one addition each in the test), the message m0 + i * m_step and
a nonce of its own; all three differ between any two rows.  The file holds the integers in hexadecimal.

    python tests/golden/gen_schnorr_chunk_rows.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import schnorr_ref  # noqa: E402

N = 261


def main():
    out = {}
    for seed, scheme in enumerate(schnorr_ref.SCHEMES):
        S = schnorr_ref.Schnorr(scheme)
        rng = random.Random(261 + seed)
        sk0, m0, m_step = rng.randrange(S.r - N), rng.randrange(S.p), rng.randrange(1, S.p)
        pk = S.pk(sk0)
        nonces, sigs = [], []
        for i in range(N):
            while True:
                k = rng.randrange(1, S.r)
                sig = S.sign_with(sk0 + i, pk, [(m0 + i * m_step) % S.p], k)
                if sig:
                    break
            nonces.append(k)
            sigs.append(sig)
            pk = S.C.add(pk, S.G)
        assert len(set(nonces)) == N
        out[scheme] = {"sk0": hex(sk0), "m0": hex(m0), "m_step": hex(m_step), "nonces": [hex(k) for k in nonces],
                       "sigs": [[hex(e), hex(s)] for e, s in sigs]}
    with open(os.path.join(HERE, "schnorr_chunk_rows.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
