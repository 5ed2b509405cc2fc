#!/usr/bin/env python3
"""Derive the constants of the MNT4-753 ate pairing from p and r alone and emit
   ginger-lib_amd/csrc/pairing_constants_gen.h   (device-internal radix-2^29 Montgomery form, digit strings)
   tests/golden/pairing_constants.json           (the same numbers for the Python side)

Run in the authoring container only: every value is cross-checked against the reference's literal
(algebra/src/curves/mnt4753/mod.rs:27-103, algebra/src/fields/mnt4753/fq2.rs, fq4.rs) as tools/gen_constants.py does for the
field and curve constants.  The outputs are committed; nothing at run time reads the reference.

  T            = r - p, the absolute value of the (negative) Frobenius trace minus one: the ate loop count
  NAF(T)       the signed-digit form the Miller loop runs over (without its leading 1)
  (p^2 + 1)/r  = m1 p + m0 with m1 = 1 and m0 = -(T - 1): the last chunk of the final exponent
  NAF(T - 1)   the signed-digit form of |m0| for the cyclotomic exponentiation
  Frobenius    13^((p^i - 1)/2), i < 2 (Fq2) and 13^((p^i - 1)/4), i < 4 (Fq4)
  twist = (0, 1), a' = a * twist^2 = (26, 0)
"""
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/algebra/src"
OUT_H = os.path.join(HERE, "..", "ginger-lib_amd", "csrc", "pairing_constants_gen.h")
OUT_J = os.path.join(HERE, "..", "tests", "golden", "pairing_constants.json")
NR = 13


def naf(x):
    """non-adjacent form, least significant digit first"""
    out = []
    while x:
        if x & 1:
            d = 2 - (x & 3)
            x -= d
        else:
            d = 0
        out.append(d)
        x >>= 1
    return out


def derive(p, r):
    T = r - p
    assert T > 0 and (p * p + 1) % r == 0 and (p * p + 1) // r == p - (T - 1)
    ate = naf(T)
    assert ate[-1] == 1
    w0 = naf(T - 1)
    return {
        "nonresidue": NR,
        "ate_loop_count": hex(T),
        "ate_is_loop_count_neg": True,
        "ate_naf": ate[:-1],                        # least significant first, leading 1 dropped (the reference's WNAF)
        "final_exponent_last_chunk_1": hex(1),
        "final_exponent_last_chunk_abs_of_w0": hex(T - 1),
        "final_exponent_last_chunk_w0_is_neg": True,
        "w0_naf": w0,                               # least significant first, leading 1 kept
        "frobenius_fq2_c1": [hex(pow(NR, (p ** i - 1) // 2, p)) for i in range(2)],
        "frobenius_fq4_c1": [hex(pow(NR, (p ** i - 1) // 4, p)) for i in range(4)],
        "twist": [hex(0), hex(1)],
        "twist_coeff_a": [hex(2 * NR), hex(0)],
    }


def _ints(body):
    body = re.sub(r"//[^\n]*", "", body)
    return [int(t.strip(), 0) for t in body.replace("\n", " ").split(",") if t.strip()]


def _big(body):
    return sum(v << (64 * i) for i, v in enumerate(_ints(body)))


def cross_check(J, p):
    """every derived value against the reference's literal"""
    Rinv = pow(1 << 768, -1, p)
    src = open(os.path.join(REF, "curves/mnt4753/mod.rs")).read()
    assert _big(re.search(r"ATE_LOOP_COUNT: &'static \[u64\] = &\[(.*?)\]", src, re.S).group(1)) == int(J["ate_loop_count"], 16)
    assert _ints(re.search(r"WNAF: &'static \[i32\] = &\[(.*?)\]", src, re.S).group(1)) == J["ate_naf"]
    assert "ATE_IS_LOOP_COUNT_NEG: bool = true" in src and "FINAL_EXPONENT_LAST_CHUNK_W0_IS_NEG: bool = true" in src
    assert _big(re.search(r"FINAL_EXPONENT_LAST_CHUNK_1: BigInteger = BigInteger\(\[(.*?)\]\)", src, re.S).group(1)) == 1
    assert _big(re.search(r"FINAL_EXPONENT_LAST_CHUNK_ABS_OF_W0: BigInteger = BigInteger\(\[(.*?)\]\)", src, re.S).group(1)) == \
        int(J["final_exponent_last_chunk_abs_of_w0"], 16)
    assert "const TWIST: Fq2 = field_new!(Fq2, FQ_ZERO, FQ_ONE)" in src
    a = re.search(r"TWIST_COEFF_A: Fq2 = field_new!\(Fq2,(.*?);", src, re.S).group(1)
    assert [_big(m) * Rinv % p for m in re.findall(r"BigInteger\(\[(.*?)\]\)", a, re.S)] == [int(J["twist_coeff_a"][0], 16)]
    assert a.rstrip().rstrip(")").rstrip().endswith("FQ_ZERO,") and int(J["twist_coeff_a"][1], 16) == 0
    for path, name, key in (("fields/mnt4753/fq2.rs", "FROBENIUS_COEFF_FP2_C1", "frobenius_fq2_c1"),
                            ("fields/mnt4753/fq4.rs", "FROBENIUS_COEFF_FP4_C1", "frobenius_fq4_c1")):
        s = open(os.path.join(REF, path)).read()
        body = s[s.index(name):]
        body = body[:body.index("];")]
        got = [_big(m) * Rinv % p for m in re.findall(r"BigInteger\(\[(.*?)\]\)", body, re.S)]
        assert got == [int(v, 16) for v in J[key]], name


def main():
    C = json.load(open(os.path.join(HERE, "..", "tests", "golden", "constants.json")))
    p, r = int(C["fields"]["p4"]["p"], 16), int(C["fields"]["p6"]["p"], 16)
    J = derive(p, r)
    cross_check(J, p)
    json.dump(J, open(OUT_J, "w"), indent=0)

    def arr29(x):
        x = x * pow(2, 754, p) % p
        return "{" + ", ".join("0x%08xu" % ((x >> (29 * i)) & ((1 << 29) - 1)) for i in range(26)) + "}"

    def digits(d):  # most significant first
        return "{" + ", ".join(str(v) for v in reversed(d)) + "}"

    L = ["// GENERATED by tools/gen_pairing_constants.py -- do not edit.",
         "// Constants of the MNT4-753 ate pairing, derived from p and r and cross-checked against the reference's literals",
         "// (algebra/src/curves/mnt4753/mod.rs:27-103, algebra/src/fields/mnt4753/fq2.rs, fq4.rs).",
         "#pragma once",
         "// twist = (0, 1), a' = (26, 0) (ec29.h Mnt4G2::mul_by_a); the trace is negative, and so is w0 = -(T - 1); m1 = 1",
         "// signed digits of the loop count T = r - p, most significant first, the leading 1 dropped",
         "#define GH_MNT4_ATE_DIGITS %d" % len(J["ate_naf"]),
         "#define GH_MNT4_ATE_NONZERO %d" % sum(1 for d in J["ate_naf"] if d),
         "#define GH_MNT4_ATE_NAF %s" % digits(J["ate_naf"]),
         "// signed digits of T - 1 = |w0|, most significant first, the leading 1 kept",
         "#define GH_MNT4_W0_DIGITS %d" % len(J["w0_naf"]),
         "#define GH_MNT4_W0_NAF %s" % digits(J["w0_naf"])]
    for key, name in (("frobenius_fq2_c1", "GH_MNT4_FROB2_C1"), ("frobenius_fq4_c1", "GH_MNT4_FROB4_C1")):
        for i, v in enumerate(J[key]):
            L.append("#define %s_%d_I29 %s" % (name, i, arr29(int(v, 16))))
    L.append("")
    open(OUT_H, "w").write("\n".join(L))
    print("wrote", os.path.normpath(OUT_H), "and", os.path.normpath(OUT_J))


if __name__ == "__main__":
    main()
