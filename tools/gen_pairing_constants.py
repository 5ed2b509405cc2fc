#!/usr/bin/env python3
"""Derive the constants of the MNT4-753 and MNT6-753 ate pairings from p and r alone and emit
   ginger-lib_amd/csrc/pairing_constants_gen.h   (device-internal radix-2^29 Montgomery form, digit strings)
   tests/golden/pairing_constants.json           (the MNT4-753 numbers for the Python side)
   tests/golden/pairing6_constants.json          (the MNT6-753 numbers)

Run in the authoring container only: every value is cross-checked against the reference's literal
(algebra/src/curves/mnt4753/mod.rs:27-103, algebra/src/fields/mnt4753/fq2.rs, fq4.rs) as tools/gen_constants.py does for the
field and curve constants.  The outputs are committed; nothing at run time reads the reference.

  T            = r - p, the absolute value of the (negative) Frobenius trace minus one: the ate loop count
  NAF(T)       the signed-digit form the Miller loop runs over (without its leading 1)
  (p^2 + 1)/r  = m1 p + m0 with m1 = 1 and m0 = -(T - 1): the last chunk of the final exponent
  NAF(T - 1)   the signed-digit form of |m0| for the cyclotomic exponentiation
  Frobenius    13^((p^i - 1)/2), i < 2 (Fq2) and 13^((p^i - 1)/4), i < 4 (Fq4)
  twist = (0, 1), a' = a * twist^2 = (26, 0)

MNT6-753 (algebra/src/curves/mnt6753/mod.rs:27-104, fields/mnt6753/fq3.rs, fq6.rs), with p and r exchanged:
  T            = p - r, the (positive) Frobenius trace minus one: the same integer as MNT4's loop count
  (p^2-p+1)/r  = m1 p + m0 with m1 = 1 and m0 = +T
  NAF(T)       with its leading 1: the digits of the cyclotomic exponentiation
  Frobenius    11^((p^i - 1)/3) and its square, i < 3 (Fq3), and 11^((p^i - 1)/6), i < 6 (Fq6)
  twist = (0, 1, 0), a' = a * twist^2 = (0, 0, 11)
"""
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/algebra/src"
OUT_H = os.path.join(HERE, "..", "ginger-lib_amd", "csrc", "pairing_constants_gen.h")
OUT_J = os.path.join(HERE, "..", "tests", "golden", "pairing_constants.json")
OUT_J6 = os.path.join(HERE, "..", "tests", "golden", "pairing6_constants.json")
NR = 13
NR6 = 11


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


def derive6(p, r):
    """p: the MNT6-753 base field, r: its group order"""
    T = p - r
    assert T > 0 and (p * p - p + 1) % r == 0 and (p * p - p + 1) // r == p + T
    assert (p ** 6 - 1) // r == (p ** 3 - 1) * (p + 1) * (p + T)
    ate = naf(T)
    assert ate[-1] == 1
    c1 = [pow(NR6, (p ** i - 1) // 3, p) for i in range(3)]
    return {
        "nonresidue": NR6,
        "ate_loop_count": hex(T),
        "ate_is_loop_count_neg": False,
        "ate_naf": ate[:-1],                        # least significant first, leading 1 dropped (the reference's WNAF)
        "final_exponent_last_chunk_1": hex(1),
        "final_exponent_last_chunk_abs_of_w0": hex(T),
        "final_exponent_last_chunk_w0_is_neg": False,
        "w0_naf": ate,                              # least significant first, leading 1 kept
        "frobenius_fq3_c1": [hex(v) for v in c1],
        "frobenius_fq3_c2": [hex(v * v % p) for v in c1],
        "frobenius_fq6_c1": [hex(pow(NR6, (p ** i - 1) // 6, p)) for i in range(6)],
        "twist": [hex(0), hex(1), hex(0)],
        "twist_coeff_a": [hex(0), hex(0), hex(NR6)],
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


def cross_check6(J, p):
    """the same for MNT6-753"""
    Rinv = pow(1 << 768, -1, p)
    src = open(os.path.join(REF, "curves/mnt6753/mod.rs")).read()
    assert _big(re.search(r"ATE_LOOP_COUNT: &'static \[u64\] = &\[(.*?)\]", src, re.S).group(1)) == int(J["ate_loop_count"], 16)
    assert _ints(re.search(r"WNAF: &'static \[i32\] = &\[(.*?)\]", src, re.S).group(1)) == J["ate_naf"]
    assert "ATE_IS_LOOP_COUNT_NEG: bool = false" in src and "FINAL_EXPONENT_LAST_CHUNK_W0_IS_NEG: bool = false" in src
    assert _big(re.search(r"FINAL_EXPONENT_LAST_CHUNK_1: BigInteger = BigInteger\(\[(.*?)\]\)", src, re.S).group(1)) == 1
    assert _big(re.search(r"FINAL_EXPONENT_LAST_CHUNK_ABS_OF_W0: BigInteger =\s*BigInteger\(\[(.*?)\]\)", src, re.S).group(1)) == \
        int(J["final_exponent_last_chunk_abs_of_w0"], 16)
    assert "const TWIST: Fq3 = field_new!(Fq3, FQ_ZERO, FQ_ONE, FQ_ZERO)" in src
    a = re.search(r"TWIST_COEFF_A: Fq3 = field_new!\(Fq3,(.*?);", src, re.S).group(1)
    assert re.match(r"\s*FQ_ZERO,\s*FQ_ZERO,\s*field_new!", a)
    assert [_big(m) * Rinv % p for m in re.findall(r"BigInteger\(\[(.*?)\]\)", a, re.S)] == [int(J["twist_coeff_a"][2], 16)]
    for path, name, key in (("fields/mnt6753/fq3.rs", "FROBENIUS_COEFF_FP3_C1", "frobenius_fq3_c1"),
                            ("fields/mnt6753/fq3.rs", "FROBENIUS_COEFF_FP3_C2", "frobenius_fq3_c2"),
                            ("fields/mnt6753/fq6.rs", "FROBENIUS_COEFF_FP6_C1", "frobenius_fq6_c1")):
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
    J6 = derive6(r, p)                              # the cycle: MNT6-753's base field is MNT4-753's group order
    cross_check6(J6, r)
    json.dump(J6, open(OUT_J6, "w"), indent=0)

    def arr29(x, p=p):
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
    L += ["// Constants of the MNT6-753 ate pairing (algebra/src/curves/mnt6753/mod.rs:27-104, algebra/src/fields/mnt6753/fq3.rs, fq6.rs).",
          "// twist = (0, 1, 0), a' = (0, 0, 11); the trace is positive, and so is w0 = +T; m1 = 1",
          "// signed digits of the loop count T = p - r (MNT4's integer), most significant first, the leading 1 dropped",
          "#define GH_MNT6_ATE_DIGITS %d" % len(J6["ate_naf"]),
          "#define GH_MNT6_ATE_NONZERO %d" % sum(1 for d in J6["ate_naf"] if d),
          "#define GH_MNT6_ATE_NAF %s" % digits(J6["ate_naf"]),
          "// signed digits of T = w0, most significant first, the leading 1 kept",
          "#define GH_MNT6_W0_DIGITS %d" % len(J6["w0_naf"]),
          "#define GH_MNT6_W0_NAF %s" % digits(J6["w0_naf"])]
    for key, name in (("frobenius_fq3_c1", "GH_MNT6_FROB3_C1"), ("frobenius_fq3_c2", "GH_MNT6_FROB3_C2"),
                      ("frobenius_fq6_c1", "GH_MNT6_FROB6_C1")):
        for i, v in enumerate(J6[key]):
            L.append("#define %s_%d_I29 %s" % (name, i, arr29(int(v, 16), r)))
    L.append("")
    open(OUT_H, "w").write("\n".join(L))
    print("wrote", os.path.normpath(OUT_H), ",", os.path.normpath(OUT_J), "and", os.path.normpath(OUT_J6))


if __name__ == "__main__":
    main()
