#!/usr/bin/env python3
"""Extract the reference's even and odd known points of its compression tests into tests/golden/compression_kats.json:
   algebra/src/curves/mnt4753/tests.rs   test_g1_compression_decompression, test_g2_compression_decompression
   algebra/src/curves/mnt6753/tests.rs   the same two tests
Numbers only: per curve the canonical coordinates (hex) of `even` (y.is_odd() == false) and `odd`.  Run in the authoring
container; the output is committed and nothing at run time reads the reference.  Test infrastructure."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/algebra/src"


def big(body):
    body = re.sub(r"//[^\n]*", "", body)
    return sum(int(t.strip(), 0) << (64 * i) for i, t in enumerate(t for t in body.replace("\n", " ").split(",") if t.strip()))


def points(src, fn, deg):
    body = src[src.index("fn %s()" % fn):]
    body = body[:body.index("compression_test::<")]
    marks = sorted((body.index("let %s = " % name), name) for name in ("even", "odd"))     # either may come first
    out = {}
    for k, (at, name) in enumerate(marks):
        part = body[at:marks[k + 1][0]] if k + 1 < len(marks) else body[at:]
        v = [big(m) for m in re.findall(r"BigInteger768\(\[(.*?)\]\)", part, re.S)]
        assert len(v) == 2 * deg, (fn, name, len(v))
        out[name] = {"x": [hex(c) for c in v[:deg]], "y": [hex(c) for c in v[deg:]]}
    return out


def main():
    J = {}
    for fam, g2deg in (("mnt4753", 2), ("mnt6753", 3)):
        src = open(os.path.join(REF, "curves", fam, "tests.rs")).read()
        J[fam + "_g1"] = points(src, "test_g1_compression_decompression", 1)
        J[fam + "_g2"] = points(src, "test_g2_compression_decompression", g2deg)
    out = os.path.join(HERE, "compression_kats.json")
    json.dump(J, open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
