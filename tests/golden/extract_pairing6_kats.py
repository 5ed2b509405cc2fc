#!/usr/bin/env python3
"""Extract the known answer of the reference's pairing test (algebra/src/curves/mnt6753/tests.rs test_bilinearity) into
tests/golden/pairing6_kats.json.  Only DATA is taken: the 18 BigInteger768 literals (Fq::from_repr: canonical integers), in order:
  0-2    a: G1 projective x, y, z
  3-11   b: G2 projective x.c0, x.c1, x.c2, y.c0, y.c1, y.c2, z.c0, z.c1, z.c2
  12-17  the expected Fq6 e(a, b): c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2
Run in the authoring container only."""
import json
import os
import re

REF = "/root/reference/algebra/src/curves/mnt6753/tests.rs"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pairing6_kats.json")


def main():
    src = open(REF).read()
    start = src.index("fn test_bilinearity")
    body = src[start:]
    assert body.index("assert_eq!(MNT6::pairing(a, b), Fq6::new(") > 0
    vals = []
    for m in re.finditer(r"BigInteger768\(\[(.*?)\]\)", body, re.S):
        limbs = [int(t.strip(), 0) for t in m.group(1).replace("\n", " ").split(",") if t.strip()]
        assert len(limbs) == 12
        vals.append(hex(sum(v << (64 * i) for i, v in enumerate(limbs))))
    vals = vals[:18]
    assert len(vals) == 18
    json.dump({"test_bilinearity": {"line": src[:start].count("\n") + 1, "from_repr": vals}}, open(OUT, "w"), indent=0)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
