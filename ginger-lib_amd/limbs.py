"""Field constants of the two pairings and the limb forms of field elements, shared by the prover, verifier and R1CS
modules (groth16.py, gm17.py, pairing.py, gm17_verify.py, r1cs.py).  Imports nothing from the package.

An element of Fp768 is a row of 12 u64 limbs, little-endian: canonical (the integer itself: into_repr, scalars of an MSM,
coefficients on the wire) or Montgomery (x * 2^768 mod p: the in-memory form, fp_768.rs:24-30)."""
import numpy as np

# base-field bytes of one coordinate coefficient / degree of the G2 coordinate field / bytes of the target-field element
# vk.alpha_g1_beta_g2 (Fq4 resp. Fq6)
FQ_BYTES = 96
G2_DEG = {"mnt4753": 2, "mnt6753": 3}
FQK_BYTES = {"mnt4753": 4 * 96, "mnt6753": 6 * 96}
MODULUS = {   # r = scalar field of the pairing = base field of the other curve
    "mnt4753": 0x1c4c62d92c41110229022eee2cdadb7f997505b8fafed5eb7e8f96c97d87307fdb925e8a0ed8d99d124d9a15af79db26c5c28c859a99b3eebca9429212636b9dff97634993aa4d6c381bc3f0057974ea099170fa13a4fd90776e240000001,
    "mnt6753": 0x1c4c62d92c41110229022eee2cdadb7f997505b8fafed5eb7e8f96c97d87307fdb925e8a0ed8d99d124d9a15af79db117e776f218059db80f0da5cb537e38685acce9767254a4638810719ac425f0e39d54522cdd119f5e9063de245e8001,
}
FR_FIELD = {"mnt4753": "mnt4753_fr", "mnt6753": "mnt6753_fr"}      # the C ABI's name of the pairing's scalar field


def base_modulus(pairing):
    """q = base field of the pairing's curves: the other curve's scalar field"""
    return MODULUS["mnt6753" if pairing == "mnt4753" else "mnt4753"]


def domain_size(n):
    """the smallest power of two >= n (EvaluationDomain::new)"""
    return 1 << max(0, int(n) - 1).bit_length()


def canon_rows(vals):
    """integers in [0, 2^768) -> (n, 12) u64 rows of their limbs, writable; anything else raises OverflowError"""
    raw = bytearray().join(int(v).to_bytes(96, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(raw) // 96, 12)


def mont_rows(vals, modulus):
    """integers -> (n, 12) u64 Montgomery rows (x * 2^768 mod p)"""
    R = (1 << 768) % modulus
    return canon_rows([v * R % modulus for v in vals])


def ints_from_canon_rows(rows):
    raw = np.ascontiguousarray(rows, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 96], "little") for i in range(0, len(raw), 96)]


def ints_from_mont_rows(rows, modulus):
    rinv = pow(1 << 768, -1, modulus)
    return [v * rinv % modulus for v in ints_from_canon_rows(rows)]


def affine_to_wire(pairing, group, xy, is_infinity):
    """GroupAffine::write of an affine result (Montgomery x || y limbs from gh_proj_to_affine): canonical little-endian
    coefficients + infinity byte; zero() is written as (0, 1, true) (swp.rs:130-132)."""
    words = 24 * (1 if group == "g1" else G2_DEG[pairing])
    coeffs = ints_from_mont_rows(np.asarray(xy, dtype=np.uint64).ravel()[:words], base_modulus(pairing))
    return b"".join(v.to_bytes(FQ_BYTES, "little") for v in coeffs) + (b"\x01" if is_infinity else b"\x00")
