#!/usr/bin/env python3
"""Extract the two Poseidon parameter sets of the reference (primitives/src/crh/poseidon/parameters.rs:
MNT4753PoseidonParameters, MNT6753PoseidonParameters) into tests/golden/poseidon_params.json.

Only DATA is taken: R_F, R_P and, as the reference stores them (12 little-endian u64 limbs of the Montgomery
form with R = 2^768, written as hex integers here), C2, AFTER_ZERO_PERM (3), ROUND_CST (every entry, also the
three MNT6 entries its 64 rounds never read) and MDS_CST (9, row-major).  MDS_CST_SHORT (the same matrix in an
R = 2^64 representation) is not needed: the library multiplies by the full-size entries.
Run in the authoring container only (the reference is not on the GPU box).
"""
import json, os, re

REF = "/root/reference/primitives/src/crh/poseidon/parameters.rs"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "poseidon_params.json")
SETS = {"mnt4753": ("MNT4753PoseidonParameters", "mnt4753_fr"), "mnt6753": ("MNT6753PoseidonParameters", "mnt6753_fr")}


def limbs_to_hex(body):
    toks = [t.strip() for t in body.replace("\n", " ").split(",") if t.strip()]
    limbs = [int(t, 0) for t in toks]
    assert len(limbs) == 12
    return hex(sum(v << (64 * i) for i, v in enumerate(limbs)))


def field_list(block, name):
    m = re.search(r"const %s\s*:[^=]*=\s*&\s*\[(.*?)\n\s*\];" % name, block, re.S)
    assert m, name
    return [limbs_to_hex(b) for b in re.findall(r"BigInteger768\(\[(.*?)\]\)", m.group(1), re.S)]


def main():
    src = open(REF).read()
    out = {}
    for tag, (struct, field) in SETS.items():
        start = src.index("impl PoseidonParameters for %s" % struct)
        nxt = src.find("impl FieldBasedHashParameters", start)
        block = src[start:nxt if nxt > 0 else len(src)]
        c2 = re.search(r"const C2\s*:.*?BigInteger768\(\[(.*?)\]\)", block, re.S).group(1)
        out[tag] = {
            "field": field,
            "t": int(re.search(r"const T\s*:\s*usize\s*=\s*(\d+)", block).group(1)),
            "rate": int(re.search(r"const R\s*:\s*usize\s*=\s*(\d+)", block).group(1)),
            "r_f": int(re.search(r"const R_F\s*:\s*i32\s*=\s*(\d+)", block).group(1)),
            "r_p": int(re.search(r"const R_P\s*:\s*i32\s*=\s*(\d+)", block).group(1)),
            "c2": limbs_to_hex(c2),
            "after_zero_perm": field_list(block, "AFTER_ZERO_PERM"),
            "round_cst": field_list(block, "ROUND_CST"),
            "mds": field_list(block, "MDS_CST"),
        }
        s = out[tag]
        assert s["t"] == 3 and s["rate"] == 2 and len(s["after_zero_perm"]) == 3 and len(s["mds"]) == 9
        assert len(s["round_cst"]) >= 3 * (2 * s["r_f"] + s["r_p"])
    json.dump(out, open(OUT, "w"), indent=1)
    print("wrote", OUT, {k: (v["r_f"], v["r_p"], len(v["round_cst"])) for k, v in out.items()})


if __name__ == "__main__":
    main()
