#!/usr/bin/env python3
"""Extract the known answer of the reference's pairing test (algebra/src/curves/mnt4753/tests.rs test_bilinearity) into
tests/golden/pairing_kats.json.  Only DATA is taken: the 13 BigInteger768 literals (Fq::from_repr: canonical integers), in order:
  0-2   a: G1 projective x, y, z
  3-8   b: G2 projective x.c0, x.c1, y.c0, y.c1, z.c0, z.c1
  9-12  the expected Fq4 e(a, b): c0.c0, c0.c1, c1.c0, c1.c1
Run in the authoring container only."""
import json
import os
import re

REF = "/root/reference/algebra/src/curves/mnt4753/tests.rs"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pairing_kats.json")


def main():
    src = open(REF).read()
    start = src.index("fn test_bilinearity")
    body = src[start:]
    vals = []
    for m in re.finditer(r"BigInteger768\(\[(.*?)\]\)", body, re.S):
        limbs = [int(t.strip(), 0) for t in m.group(1).replace("\n", " ").split(",") if t.strip()]
        assert len(limbs) == 12
        vals.append(hex(sum(v << (64 * i) for i, v in enumerate(limbs))))
    vals = vals[:13]
    assert len(vals) == 13
    json.dump({"test_bilinearity": {"line": src[:start].count("\n") + 1, "from_repr": vals}}, open(OUT, "w"), indent=0)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
