"""asm_probes.py -- the unit programs of tests/test_gpu_asm_sim.py: every computing mnemonic the generators emit, at operand edges,
each with the plain Python-integer definition of what it computes (written here, not taken from asmgen/sim.py).  Not a test module.

Operands (256 lanes = four waves of one workgroup unless said otherwise):
  32-bit sources   all ordered pairs of VALS: the edges 0, 1, 2, 2^24 - 1, 2^24, 2^29 - 1, 2^29, 2^31 - 1, 2^31, 2^32 - 2, 2^32 - 1
                   and five seeded random words
  shift counts     COUNTS = 0, 1, 28, 29, 31, 32, 33, 63, 64, 2^32 - 1, against every value of VALS
  carry-in masks   all ones, all zero, alternating
  v_mad_u64_u32    additionally the columns the bound checker admits: (2^29 - 1)^2 accumulated 1 .. 64 times (64 (2^29 - 1)^2 is the
                   last multiple below 2^64), and addends around 2^64 - (2^29 - 1)^2: the sum 2^64 - 1 without and 2^64 with the carry
  f64              1 / (p_25 + 1) of both primes and 0.5 as field.mul_small passes them, and 1.0, 2.0, 0.5 over the u32 edges
"""
import random
import struct

from asm_card import I, O, Unit, V_OFF
from asmgen.build import P4, P6
from asmgen.isa import EXEC, S, V, VCC

M = 0xFFFFFFFF
M64 = (1 << 64) - 1
_rnd = random.Random(20240)
VALS = [0, 1, 2, (1 << 24) - 1, 1 << 24, (1 << 29) - 1, 1 << 29, (1 << 31) - 1, 1 << 31, M - 1, M] + [_rnd.getrandbits(32) for _ in range(5)]
COUNTS = [0, 1, 28, 29, 31, 32, 33, 63, 64, M]
N = 256
A = [VALS[l // 16] for l in range(N)]
B = [VALS[l % 16] for l in range(N)]
C = [VALS[(5 * (l // 16) + 3 * (l % 16) + 7) % 16] for l in range(N)]
CNT = [COUNTS[l % 10] for l in range(N)]
X = [VALS[(l // 10) % 16] for l in range(N)]
XH = [VALS[(3 * (l // 10) + 1) % 16] for l in range(N)]
Y = [VALS[(7 * (l // 10) + 5) % 16] for l in range(N)]
YH = [VALS[(11 * (l // 10) + 2) % 16] for l in range(N)]
MASKS = [M64, 0, 0xAAAAAAAA55555555]
L29 = (1 << 29) - 1


def s32(x):
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    return x - (1 << 64) if x >> 63 else x


def lanewise(fn):
    """fn(inputs of one lane) -> outputs of that lane; as an expectation over planes"""
    def e(inp):
        rows = [fn(*[p[l] for p in inp]) for l in range(len(inp[0]))]
        return [list(col) for col in zip(*rows)]
    return e


def wave_masks(bits):
    """lane predicate -> (low word, high word) of the lane's wave mask, per lane"""
    lo, hi = [], []
    for w in range(len(bits) // 64):
        m = sum(1 << l for l in range(64) if bits[64 * w + l])
        lo += [m & M] * 64
        hi += [m >> 32] * 64
    return lo, hi


S_VIA = S(44, 2)            # VCC's halves are moved through this pair


def put_mask(g, reg, m):
    via = S_VIA if reg.kind == "vcc" else reg
    g.s_mov_b32(via.lo(), m & M)
    g.s_mov_b32(via.hi(), m >> 32)
    if via is not reg:
        g.s_mov_b64(reg, via)


def out_mask(g, k, reg):
    if reg.kind == "vcc":
        g.s_mov_b64(S_VIA, reg)
        reg = S_VIA
    g.v_mov_b32(O(k), reg.lo())
    g.v_mov_b32(O(k + 1), reg.hi())


# ------------------------------------------------------------------ VALU, two sources
BIN = [("v_add_u32", lambda a, b: a + b), ("v_sub_u32", lambda a, b: a - b), ("v_subrev_u32", lambda a, b: b - a),
       ("v_and_b32", lambda a, b: a & b), ("v_or_b32", lambda a, b: a | b), ("v_xor_b32", lambda a, b: a ^ b),
       ("v_lshlrev_b32", lambda a, b: b << (a & 31)), ("v_lshrrev_b32", lambda a, b: b >> (a & 31)),
       ("v_ashrrev_i32", lambda a, b: s32(b) >> (a & 31)), ("v_mul_lo_u32", lambda a, b: a * b),
       ("v_mul_hi_u32", lambda a, b: (a * b) >> 32), ("v_mul_u32_u24", lambda a, b: (a & 0xFFFFFF) * (b & 0xFFFFFF))]
SCONST = 0x1FFFFFFF


def valu_bin():
    def body(g):
        for k, (op, _) in enumerate(BIN):
            getattr(g, op)(O(k), I(0), I(1))
        k = len(BIN)
        g.v_mov_b32(O(k), I(0))
        g.v_bfrev_b32(O(k + 1), I(0))
        g.s_mov_b32(S(20), SCONST)                               # the forms with a scalar, a literal and an inline constant
        g.v_and_b32(O(k + 2), S(20), I(1))
        g.v_mul_lo_u32(O(k + 3), I(0), S(20))
        g.v_add_u32(O(k + 4), 0x12345678, I(1))
        g.v_sub_u32(O(k + 5), 0, I(1))
        g.v_mov_b32(O(k + 6), S(20))
        g.v_mov_b32(O(k + 7), -16)

    def ref(a, b):
        return tuple(f(a, b) for _, f in BIN) + (a, int("{:032b}".format(a)[::-1], 2), SCONST & b, a * SCONST, 0x12345678 + b, -b,
                                                SCONST, -16)
    return Unit("valu_bin", [op for op, _ in BIN] + ["v_mov_b32", "v_bfrev_b32", "s_mov_b32"], 2, len(BIN) + 8, body, [A, B], lanewise(ref))


# ------------------------------------------------------------------ VALU, three sources
def _bfe(a, off, wd):
    return (a >> (off & 31)) & ((1 << (wd & 31)) - 1)


TERN = [("v_add3_u32", lambda a, b, c: a + b + c), ("v_or3_b32", lambda a, b, c: a | b | c),
        ("v_bfi_b32", lambda a, b, c: (a & b) | (~a & c)), ("v_lshl_add_u32", lambda a, b, c: (a << (b & 31)) + c),
        ("v_lshl_or_b32", lambda a, b, c: (a << (b & 31)) | c), ("v_alignbit_b32", lambda a, b, c: ((a << 32 | b) >> (c & 31))),
        ("v_bfe_u32", _bfe), ("v_mad_u32_u24", lambda a, b, c: (a & 0xFFFFFF) * (b & 0xFFFFFF) + c)]


def valu_tern():
    def body(g):
        for k, (op, _) in enumerate(TERN):
            getattr(g, op)(O(k), I(0), I(1), I(2))
        k = len(TERN)
        g.s_mov_b32(S(20), SCONST)
        g.v_add3_u32(O(k), I(0), S(20), I(2))                    # the product's form: the prime's limb in the middle
        g.v_bfi_b32(O(k + 1), S(20), 0, I(2))                    # the mask of the low 29 bits cleared
        g.v_bfe_u32(O(k + 2), I(0), 29, 3)
        g.v_alignbit_b32(O(k + 3), I(0), I(1), 29)

    def ref(a, b, c):
        return tuple(f(a, b, c) for _, f in TERN) + (a + SCONST + c, ~SCONST & c, _bfe(a, 29, 3), (a << 32 | b) >> 29)
    return Unit("valu_tern", [op for op, _ in TERN], 3, len(TERN) + 4, body, [A, B, C], lanewise(ref))


# ------------------------------------------------------------------ shifts and offsets at the counts
def shifts():
    x64, y64, cnt = I(0, 2), I(2, 2), I(4)

    def body(g):
        g.v_lshlrev_b32(O(0), cnt, I(0))
        g.v_lshrrev_b32(O(1), cnt, I(0))
        g.v_ashrrev_i32(O(2), cnt, I(0))
        g.v_alignbit_b32(O(3), I(0), I(2), cnt)
        g.v_bfe_u32(O(4), I(0), cnt, 29)
        g.v_bfe_u32(O(5), I(0), 3, cnt)
        g.v_lshl_add_u32(O(6), I(0), cnt, I(2))
        g.v_lshl_or_b32(O(7), I(0), cnt, I(2))
        g.v_lshrrev_b64(O(8, 2), cnt, x64)
        g.v_ashrrev_i64(O(10, 2), cnt, x64)
        g.v_lshrrev_b64(O(12, 2), 29, x64)
        g.v_ashrrev_i64(O(14, 2), 29, x64)
        for k in range(5):
            g.v_lshl_add_u64(O(16 + 2 * k, 2), x64, k, y64)

    def ref(x, xh, y, yh, c):
        x64, y64 = xh << 32 | x, yh << 32 | y
        pair = lambda v: (v & M, (v >> 32) & M)
        r = (x << (c & 31), x >> (c & 31), s32(x) >> (c & 31), (x << 32 | y) >> (c & 31), _bfe(x, c, 29), _bfe(x, 3, c),
             (x << (c & 31)) + y, (x << (c & 31)) | y)
        r += pair(x64 >> (c & 63)) + pair(s64(x64) >> (c & 63)) + pair(x64 >> 29) + pair(s64(x64) >> 29)
        for k in range(5):
            r += pair((x64 << k) + y64)
        return r
    return Unit("shifts", ["v_lshrrev_b64", "v_ashrrev_i64", "v_lshl_add_u64"], 5, 26, body, [X, XH, Y, YH, CNT], lanewise(ref))


# ------------------------------------------------------------------ carries
def carries():
    def body(g):
        g.v_add_co_u32(O(0), S(20, 2), I(0), I(1))
        out_mask(g, 1, S(20, 2))
        g.v_sub_co_u32(O(3), S(22, 2), I(0), I(1))
        out_mask(g, 4, S(22, 2))
        k = 6
        for j, m in enumerate(MASKS):
            cin, cout = (VCC, VCC) if j == 2 else (S(24, 2), S(26, 2))      # the generators' form: VCC in and out
            put_mask(g, cin, m)
            g.v_addc_co_u32(O(k), cout, I(0), I(1), cin)
            out_mask(g, k + 1, cout)
            put_mask(g, cin, m)
            g.v_subb_co_u32(O(k + 3), cout, I(0), I(1), cin)
            out_mask(g, k + 4, cout)
            k += 6

    def expect(inp):
        a, b = inp
        n = len(a)
        out = [[(a[l] + b[l]) & M for l in range(n)]]
        out += wave_masks([a[l] + b[l] > M for l in range(n)])
        out += [[(a[l] - b[l]) & M for l in range(n)]]
        out += wave_masks([a[l] < b[l] for l in range(n)])
        for m in MASKS:
            ci = [(m >> (l % 64)) & 1 for l in range(n)]
            out += [[(a[l] + b[l] + ci[l]) & M for l in range(n)]]
            out += wave_masks([a[l] + b[l] + ci[l] > M for l in range(n)])
            out += [[(a[l] - b[l] - ci[l]) & M for l in range(n)]]
            out += wave_masks([a[l] - b[l] - ci[l] < 0 for l in range(n)])
        return out
    return Unit("carries", ["v_add_co_u32", "v_sub_co_u32", "v_addc_co_u32", "v_subb_co_u32"], 2, 6 + 18, body, [A, B], expect)


# ------------------------------------------------------------------ compares and selects
CMP = [("v_cmp_eq_u32", lambda a, b: a == b), ("v_cmp_ne_u32", lambda a, b: a != b), ("v_cmp_gt_u32", lambda a, b: a > b),
       ("v_cmp_gt_i32", lambda a, b: s32(a) > s32(b))]


def compares():
    def body(g):
        for k, (op, _) in enumerate(CMP):
            d = VCC if k == 2 else S(20 + 2 * k, 2)
            getattr(g, op)(d, I(0), I(1))
            out_mask(g, 2 * k, d)
        k = 2 * len(CMP)
        g.v_cmp_eq_u32(S(30, 2), 0, I(1))                        # the generators' form: an inline constant first
        out_mask(g, k, S(30, 2))
        for j, m in enumerate(MASKS):
            put_mask(g, S(32, 2), m)
            g.v_cndmask_b32(O(k + 2 + j), I(0), I(1), S(32, 2))
        g.v_cndmask_b32(O(k + 5), 0, -1, S(32, 2))
        g.v_cmp_gt_u32(S(34, 2), I(0), I(1))                     # a compare feeding the select, as cond_sub does
        g.v_cndmask_b32(O(k + 6), I(0), I(1), S(34, 2))

    def expect(inp):
        a, b = inp
        n = len(a)
        out = []
        for _, f in CMP:
            out += wave_masks([f(a[l], b[l]) for l in range(n)])
        out += wave_masks([b[l] == 0 for l in range(n)])
        for m in MASKS:
            out.append([b[l] if (m >> (l % 64)) & 1 else a[l] for l in range(n)])
        out.append([M if (MASKS[2] >> (l % 64)) & 1 else 0 for l in range(n)])
        out.append([b[l] if a[l] > b[l] else a[l] for l in range(n)])
        return out
    return Unit("compares", [op for op, _ in CMP] + ["v_cndmask_b32"], 2, 2 * len(CMP) + 2 + 5, body, [A, B], expect)


# ------------------------------------------------------------------ the multiplier
SPAIR = 0xFFFFFFFF00000001


def mads():
    rnd = random.Random(7)
    c = []
    for l in range(N):
        prod = A[l] * B[l]
        c.append([0, M64 - prod, (1 << 64) - prod & M64, rnd.getrandbits(64)][(l // 16 + l % 16) % 4])
    sq = L29 * L29
    a2, b2, c2 = [], [], []
    for l in range(N):
        if l < 64:                                               # the column as the checker admits it: (l + 1) products, the last below 2^64
            a2.append(L29), b2.append(L29), c2.append(l * sq)
        elif l < 128:                                            # around 2^64: lane 95 reaches 2^64 - 1, lane 96 the carry
            a2.append(L29), b2.append(L29), c2.append((1 << 64) - sq + (l - 64) - 32)
        else:
            a2.append(rnd.randrange(L29 + 1)), b2.append(rnd.randrange(L29 + 1)), c2.append(rnd.getrandbits(64))
    assert 64 * sq < 1 << 64 <= 65 * sq
    inputs = [A, B, [x & M for x in c], [x >> 32 for x in c], a2, b2, [x & M for x in c2], [x >> 32 for x in c2]]

    def body(g):
        g.v_mad_u64_u32(O(0, 2), S(20, 2), I(0), I(1), I(2, 2))
        out_mask(g, 2, S(20, 2))
        g.v_mad_u64_u32(O(4, 2), S(22, 2), I(4), I(5), I(6, 2))
        out_mask(g, 6, S(22, 2))
        put_mask(g, S(26, 2), SPAIR)
        g.v_mad_u64_u32(O(8, 2), S(24, 2), I(0), I(1), S(26, 2))     # an SGPR pair as the addend
        out_mask(g, 10, S(24, 2))
        g.s_mov_b32(S(30), SCONST)
        g.v_mad_u64_u32(O(12, 2), S(28, 2), I(0), S(30), I(2, 2))    # the prime's limb: a scalar factor
        out_mask(g, 14, S(28, 2))
        g.v_mad_u64_u32(O(16, 2), S(32, 2), I(0), I(1), 0)           # the head of a chain
        out_mask(g, 18, S(32, 2))
        g.v_mad_i64_i32(O(20, 2), S(34, 2), I(0), I(1), I(2, 2))     # {mask, result} is the 65-bit signed sum: the mask is its sign
        out_mask(g, 22, S(34, 2))
        g.v_mad_i64_i32(O(24, 2), S(36, 2), I(0), I(1), 0)
        out_mask(g, 26, S(36, 2))
        g.v_mad_i64_i32(O(28, 2), S(38, 2), I(0), S(30), I(2, 2))
        out_mask(g, 30, S(38, 2))

    def expect(inp):
        a, b, cl, ch, a2, b2, c2l, c2h = inp
        n = len(a)
        out = []

        def mad(x, y, add):
            r = [x[l] * y[l] + add[l] for l in range(n)]
            lo, hi = wave_masks([v >> 64 for v in r])
            return [[v & M for v in r], [(v >> 32) & M for v in r], lo, hi]
        c = [ch[l] << 32 | cl[l] for l in range(n)]
        out += mad(a, b, c)
        out += mad(a2, b2, [c2h[l] << 32 | c2l[l] for l in range(n)])
        out += mad(a, b, [SPAIR] * n)
        out += mad(a, [SCONST] * n, c)
        out += mad(a, b, [0] * n)
        for r in ([s32(a[l]) * s32(b[l]) + s64(c[l]) for l in range(n)], [s32(a[l]) * s32(b[l]) for l in range(n)],
                  [s32(a[l]) * SCONST + s64(c[l]) for l in range(n)]):
            out += [[v & M for v in r], [(v >> 32) & M for v in r]] + list(wave_masks([v < 0 for v in r]))
        return out
    return Unit("mads", ["v_mad_u64_u32", "v_mad_i64_i32"], 8, 32, body, inputs, expect)


# ------------------------------------------------------------------ the four f64 instructions
def _dbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


FCONST = [1.0 / ((P4 >> 29 * 25) + 1), 1.0 / ((P6 >> 29 * 25) + 1), 1.0, 2.0, 0.5]


def f64s():
    rnd = random.Random(9)
    x = [VALS[l % 16] for l in range(64)] + [rnd.getrandbits(32) for _ in range(N - 64)]

    def body(g):
        g.v_cvt_f64_u32(O(0, 2), I(0))
        for k, c in enumerate(FCONST):
            put_mask(g, S(20, 2), _dbits(c))
            g.v_cvt_f64_u32(V(30, 2), I(0))
            g.v_add_f64(V(30, 2), V(30, 2), "0.5")
            g.v_mul_f64(V(30, 2), V(30, 2), S(20, 2))
            g.v_cvt_u32_f64(O(2 + k), V(30, 2))
        for k, c in enumerate(FCONST):                           # convert, multiply, convert back: no half added
            put_mask(g, S(20, 2), _dbits(c))
            g.v_cvt_f64_u32(V(32, 2), I(0))
            g.v_mul_f64(O(7 + 5 + 2 * k, 2), V(32, 2), S(20, 2))
            g.v_cvt_u32_f64(O(7 + k), O(7 + 5 + 2 * k, 2))

    def ref(v):
        cvt = lambda f: min(max(int(f), 0), M)                   # truncation, saturating
        r = [_dbits(float(v)) & M, _dbits(float(v)) >> 32]
        r += [cvt((float(v) + 0.5) * c) for c in FCONST]
        r += [cvt(float(v) * c) for c in FCONST]
        for c in FCONST:
            r += [_dbits(float(v) * c) & M, _dbits(float(v) * c) >> 32]
        return tuple(r)
    return Unit("f64s", ["v_cvt_f64_u32", "v_add_f64", "v_mul_f64", "v_cvt_u32_f64"], 1, 22, body, [x], lanewise(ref))


# ------------------------------------------------------------------ across lanes
def _flags(kind):
    f = []
    for l in range(N):
        w, j = l // 64, l % 64
        if kind == "rfl":       # full, partial from lane 6, empty, lane 63 only
            f.append([1, int(j >= 5 and j % 3 == 0), 0, int(j == 63)][w])
        else:                   # full, alternating, scattered, the low half
            f.append([1, j & 1, int((j * 37 + 11) % 5 < 2), int(j < 32)][w])
    return f


def readfirstlane():
    flags = _flags("rfl")

    def body(g):
        g.v_cmp_ne_u32(S(20, 2), 0, I(0))
        g.v_readfirstlane_b32(S(24), I(1))
        g.s_mov_b64(EXEC, S(20, 2))
        g.v_readfirstlane_b32(S(25), I(1))
        g.s_mov_b64(EXEC, -1)
        g.v_mov_b32(O(0), S(24))
        g.v_mov_b32(O(1), S(25))

    def expect(inp):
        f, x = inp
        o0, o1 = [], []
        for w in range(N // 64):
            on = [l for l in range(64) if f[64 * w + l]]
            o0 += [x[64 * w]] * 64
            o1 += [x[64 * w + (on[0] if on else 0)]] * 64       # no lane enabled: lane 0
        return [o0, o1]
    return Unit("readfirstlane", ["v_readfirstlane_b32", "s_mov_b64"], 2, 2, body, [flags, C], expect)


SENTINEL = 0xDEAD0000


def bpermute():
    flags = _flags("bperm")
    rnd = random.Random(11)
    addr = [4 * rnd.randrange(64) if l % 4 else rnd.getrandbits(16) * 4 for l in range(N)]

    def body(g):
        g.v_cmp_ne_u32(S(20, 2), 0, I(0))
        g.v_mov_b32(O(0), SENTINEL)
        g.ds_bpermute_b32(O(1), I(1), I(2))
        g.s_mov_b64(EXEC, S(20, 2))
        g.ds_bpermute_b32(O(0), I(1), I(2))
        g.s_waitcnt(lgkmcnt=0)
        g.s_mov_b64(EXEC, -1)

    def expect(inp):
        f, a, x = inp
        o0, o1 = [], []
        for l in range(N):
            src = (l & ~63) | ((a[l] >> 2) & 63)
            o1.append(x[src])
            o0.append(SENTINEL if not f[l] else (x[src] if f[src] else 0))     # a source lane outside EXEC delivers 0
        return [o0, o1]
    return Unit("bpermute", ["ds_bpermute_b32"], 3, 2, body, [flags, addr, B], expect)


# ------------------------------------------------------------------ LDS and global memory, scalar loads
def lds():
    mirror = [((l & ~63) | (63 - (l & 63))) * 4 for l in range(N)]
    own = [l * 4 for l in range(N)]

    def body(g):
        g.ds_write_b32(I(0), I(2), offset=2048)
        g.ds_write_b32(I(1), I(2))
        g.s_waitcnt(lgkmcnt=0)
        g.ds_read_b32(O(0), I(1), offset=2048)
        g.ds_read_b32(O(1), I(0))
        g.s_waitcnt(lgkmcnt=0)

    def expect(inp):
        _, _, x = inp
        return [[x[m // 4] for m in mirror], [x[m // 4] for m in mirror]]
    return Unit("lds", ["ds_write_b32", "ds_read_b32"], 3, 2, body, [mirror, own, A], expect, lds_bytes=4096)


def _copy(n):
    def body(g):
        for k in range(n):
            g.v_xor_b32(O(k), 0x5A5A5A5A, I(k))
    return body


def memory_units():
    rnd = random.Random(13)
    planes = [[rnd.getrandbits(32) for _ in range(N)] for _ in range(4)]
    ref = lambda inp: [[v ^ 0x5A5A5A5A for v in p] for p in inp]
    us = [Unit("mem_x2", ["global_load_dwordx2", "global_store_dwordx2"], 4, 4, _copy(4), planes, ref, load=2, store=2),
          Unit("mem_x4", ["global_load_dwordx4", "global_store_dwordx4"], 4, 4, _copy(4), planes, ref, load=4, store=4),
          Unit("mem_a64_x1", ["global_load_dword", "global_store_dword"], 2, 2, _copy(2), planes[:2], ref, addr64=True),
          Unit("mem_a64_x2", ["global_load_dwordx2", "global_store_dwordx2"], 2, 2, _copy(2), planes[:2], ref, load=2, store=2, addr64=True),
          Unit("mem_a64_x4", ["global_load_dwordx4"], 4, 4, _copy(4), planes, ref, load=4, store=4, addr64=True)]
    init = 0xFFFFFF00                                           # the sums wrap
    add = lambda inp: [[(init + v) & M for v in p] for p in inp]
    us.append(Unit("atomic_noret", ["global_atomic_add"], 2, 2, lambda g: [g.v_mov_b32(O(k), I(k)) for k in range(2)],
                   [A, B], add, atomic=False, out_init=init))
    us.append(Unit("atomic_ret", ["global_atomic_add"], 2, 2, lambda g: [g.v_mov_b32(O(k), I(k)) for k in range(2)],
                   [A, B], lambda inp: add(inp) + [[init] * N] * 2, atomic=True, out_init=init))
    return us


def s_loads():
    rnd = random.Random(15)
    words = [rnd.getrandbits(32) for _ in range(N)]
    at = [0] + [2, 3] + [4, 5, 6, 7] + list(range(8, 16)) + [132, 133, 134, 135]

    def body(g):
        g.s_load_dword(S(20), S(4, 2), 0)
        g.s_load_dwordx2(S(22, 2), S(4, 2), 8)
        g.s_load_dwordx4(S(24, 4), S(4, 2), 16)
        g.s_load_dwordx8(S(32, 8), S(4, 2), 32)
        g.s_load_dwordx4(S(40, 4), S(4, 2), 0x210)               # a literal offset, as the kernels' argument blocks use
        g.s_waitcnt(lgkmcnt=0)
        for k, r in enumerate([20, 22, 23, 24, 25, 26, 27] + list(range(32, 44))):
            g.v_mov_b32(O(k), S(r))
    return Unit("s_loads", ["s_load_dword", "s_load_dwordx2", "s_load_dwordx4", "s_load_dwordx8", "s_waitcnt"], 1, len(at), body, [words],
                lambda inp: [[inp[0][j]] * N for j in at])


# ------------------------------------------------------------------ SALU: one operand set per workgroup (256 one-wave workgroups)
def salu():
    G = 256
    wa = [VALS[w // 16] for w in range(G)]
    wb = [VALS[w % 16] for w in range(G)]
    wx = [COUNTS[w % 10] for w in range(G)]
    wy = [COUNTS[(w // 10) % 10] for w in range(G)]
    wf = [(w // 16 + w % 16 + w // 64) & 1 for w in range(G)]
    spread = lambda p: [p[l // 64] for l in range(64 * G)]
    a, b, x, y, f = S(20), S(21), S(22), S(23), S(24)
    a64, b64, d, d64, sc = S(20, 2), S(22, 2), S(30), S(30, 2), S(40, 2)
    plan = []                   # (emit, reference -> tuple of words), in output order

    def scc_in(g):
        g.s_cmp_lg_u32(f, 0)

    def rec32(g, k):
        g.s_cselect_b64(sc, -1, 0)
        g.v_mov_b32(O(k), d)
        g.v_mov_b32(O(k + 1), sc.lo())

    def rec64(g, k):
        g.s_cselect_b64(sc, -1, 0)
        out_mask(g, k, d64)
        g.v_mov_b32(O(k + 2), sc.hi())

    def op32(name, ref, first=a, second=b, carry=False):
        def emit(g, k):
            if carry:
                scc_in(g)
            getattr(g, name)(d, first, second)
            rec32(g, k)
        plan.append((emit, ref, 2))

    scc = lambda t: M if t else 0
    op32("s_add_u32", lambda v: (v["a"] + v["b"], scc(v["a"] + v["b"] > M)))
    op32("s_addc_u32", lambda v: (v["a"] + v["b"] + v["f"], scc(v["a"] + v["b"] + v["f"] > M)), carry=True)
    op32("s_sub_u32", lambda v: (v["a"] - v["b"], scc(v["a"] < v["b"])))
    op32("s_and_b32", lambda v: (v["a"] & v["b"], scc(v["a"] & v["b"])))
    op32("s_lshl_b32", lambda v: (v["a"] << (v["b"] & 31), scc((v["a"] << (v["b"] & 31)) & M)))
    op32("s_lshr_b32", lambda v: (v["a"] >> (v["b"] & 31), scc(v["a"] >> (v["b"] & 31))))
    op32("s_lshl_b32", lambda v: (v["a"] << (v["x"] & 31), scc((v["a"] << (v["x"] & 31)) & M)), a, x)
    op32("s_lshr_b32", lambda v: (v["a"] >> (v["x"] & 31), scc(v["a"] >> (v["x"] & 31))), a, x)
    op32("s_mul_i32", lambda v: (v["a"] * v["b"], scc(v["f"])), carry=True)                  # SCC is left alone
    op32("s_mul_hi_u32", lambda v: ((v["a"] * v["b"]) >> 32, scc(v["f"])), carry=True)

    def emit_mov(g, k):
        scc_in(g)
        g.s_mov_b32(d, a)
        rec32(g, k)
    plan.append((emit_mov, lambda v: (v["a"], scc(v["f"])), 2))
    for name, fn in (("s_cmp_eq_u32", lambda p, q: p == q), ("s_cmp_lg_u32", lambda p, q: p != q),
                     ("s_cmp_lt_u32", lambda p, q: p < q), ("s_cmp_ge_u32", lambda p, q: p >= q)):
        def emit(g, k, name=name):
            getattr(g, name)(a, b)
            g.s_cselect_b64(sc, -1, 0)
            g.v_mov_b32(O(k), sc.lo())
        plan.append((emit, lambda v, fn=fn: (scc(fn(v["a"], v["b"])),), 1))
    p64 = lambda v: (v & M, (v >> 32) & M, scc(v & M64))
    for name, fn in (("s_and_b64", lambda p, q: p & q), ("s_andn2_b64", lambda p, q: p & ~q), ("s_or_b64", lambda p, q: p | q)):
        def emit(g, k, name=name):
            getattr(g, name)(d64, a64, b64)
            rec64(g, k)
        plan.append((emit, lambda v, fn=fn: p64(fn(v["A"], v["B"])), 3))

    def emit_mov64(g, k):
        scc_in(g)
        g.s_mov_b64(d64, a64)
        rec64(g, k)
    plan.append((emit_mov64, lambda v: (v["a"], v["b"], scc(v["f"])), 3))
    for name, fn in (("s_cmp_eq_u64", lambda p: p == 0), ("s_cmp_lg_u64", lambda p: p != 0)):
        def emit(g, k, name=name):
            getattr(g, name)(a64, 0)
            g.s_cselect_b64(sc, -1, 0)
            g.v_mov_b32(O(k), sc.lo())
        plan.append((emit, lambda v, fn=fn: (scc(fn(v["A"])),), 1))
    bfm = lambda n, o: (((1 << (n & 63)) - 1) << (o & 63)) & M64
    for first, second, fa, fb in ((a, b, "a", "b"), (x, y, "x", "y"), (y, x, "y", "x")):
        def emit(g, k, first=first, second=second):
            scc_in(g)
            g.s_bfm_b64(d64, first, second)
            rec64(g, k)
        plan.append((emit, lambda v, fa=fa, fb=fb: (bfm(v[fa], v[fb]) & M, bfm(v[fa], v[fb]) >> 32, scc(v["f"])), 3))

    def emit_bfm_imm(g, k):                                     # the generators' form: a quarter of the wave
        g.s_bfm_b64(d64, 16, 48)
        out_mask(g, k, d64)
    plan.append((emit_bfm_imm, lambda v: (0, 0xFFFF0000), 2))

    def emit_csel(g, k):
        scc_in(g)
        g.s_cselect_b64(d64, a64, b64)
        out_mask(g, k, d64)
    plan.append((emit_csel, lambda v: ((v["A"] if v["f"] else v["B"]) & M, (v["A"] if v["f"] else v["B"]) >> 32), 2))

    def emit_saveexec(g, k):
        g.s_mov_b64(VCC, a64)
        g.s_and_saveexec_b64(d64, VCC)
        g.s_mov_b64(S(32, 2), EXEC)
        g.s_cselect_b64(sc, -1, 0)
        g.s_mov_b64(EXEC, -1)
        out_mask(g, k, d64)
        out_mask(g, k + 2, S(32, 2))
        g.v_mov_b32(O(k + 4), sc.lo())
    plan.append((emit_saveexec, lambda v: (M, M, v["a"], v["b"], scc(v["A"])), 5))
    nout = sum(n for _, _, n in plan)

    def body(g):
        for k in range(5):
            g.v_readfirstlane_b32(S(20 + k), I(k))
        k = 0
        for emit, _, n in plan:
            emit(g, k)
            k += n

    def expect(inp):
        rows = []
        for w in range(G):
            v = dict(a=wa[w], b=wb[w], x=wx[w], y=wy[w], f=wf[w], A=wb[w] << 32 | wa[w], B=wy[w] << 32 | wx[w])
            r = ()
            for _, ref, n in plan:
                t = ref(v)
                assert len(t) == n
                r += t
            rows += [r] * 64
        return [list(col) for col in zip(*rows)]
    covers = ["s_add_u32", "s_addc_u32", "s_sub_u32", "s_and_b32", "s_lshl_b32", "s_lshr_b32", "s_mul_i32", "s_mul_hi_u32", "s_mov_b32",
              "s_cmp_eq_u32", "s_cmp_lg_u32", "s_cmp_lt_u32", "s_cmp_ge_u32", "s_and_b64", "s_andn2_b64", "s_or_b64", "s_mov_b64",
              "s_cmp_eq_u64", "s_cmp_lg_u64", "s_bfm_b64", "s_cselect_b64", "s_and_saveexec_b64"]
    return Unit("salu", covers, 5, nout, body, [spread(p) for p in (wa, wb, wx, wy, wf)], expect, grid=G, threads=64)


def mnemonic_units():
    return [valu_bin(), valu_tern(), shifts(), carries(), compares(), mads(), f64s(), readfirstlane(), bpermute(), lds(),
            s_loads(), salu()] + memory_units()


# ------------------------------------------------------------------ register dependencies at the spacing the shipped kernels rely on
# One unit per class of asm_card.dependency_table(): the register's old value (the complement of the new one, set well ahead),
# the writer, `gap` independent instructions, the reader.  Padded by fix_hazards like every program; never run unpadded.
NEWMASK = 0x9C3A5F0FE1D2B487
T, D, D32, V_ADDR2 = V(30), S(20, 2), S(20), V(6)


def dependency_unit(cls, gap):
    wunit, wkind, rfile, use = cls
    name = "dep_" + "_".join(x.lower().replace(" ", "").replace("-", "x").replace("_", "") for x in cls)
    n = N
    f = [(l // 64) & 1 for l in range(n)]
    own = [4 * l for l in range(n)]
    rnd = random.Random(len(name))
    a = [rnd.getrandbits(32) for _ in range(n)]
    na = [~v & M for v in a]
    wide = use in ("select mask", "carry-in", "64-bit pair", "VMEM address") or wkind not in ("-", "v_readfirstlane_b32") or rfile in ("VCC", "EXEC")
    reg = VCC if rfile == "VCC" else (EXEC if rfile == "EXEC" else (D if wide else D32))
    newbits = [(NEWMASK >> (l % 64)) & 1 for l in range(n)]      # the lanes of the new mask where it is a constant
    st = {"wait": None}

    # ---- inputs: plane 0 / 1 feed the writer, plane 2 is the old value of a VGPR under test, plane 3 a second operand
    if use in ("LDS address", "VMEM address") and rfile == "VGPR":
        p0, p1, old = own, [0] * n, [((l & ~63) | (63 - l % 64)) * 4 for l in range(n)] if use == "LDS address" else [4 * l + 8 * n for l in range(n)]
    elif wunit in ("VMEM return", "LDS return"):
        p0, p1, old = a, [0] * n, na
    else:
        p0, p1 = a, [rnd.getrandbits(32) for _ in range(n)]
        old = [~(p0[l] + p1[l]) & M for l in range(n)]
    inputs = [p0, p1, old, na, f, own]
    newv = [(p0[l] + p1[l]) & M for l in range(n)] if wunit == "VALU" else list(a)      # the VGPR under test after the writer

    def cmask(pred):
        lo, hi = wave_masks(pred)
        return [hi[l] << 32 | lo[l] for l in range(n)]
    if wkind == "v_cmp":
        new64 = cmask([p0[l] > p1[l] for l in range(n)])
    elif wkind == "v_add_co_u32":
        new64 = cmask([p0[l] + p1[l] > M for l in range(n)])
    elif wkind == "v_sub_co_u32":
        new64 = cmask([p0[l] < p1[l] for l in range(n)])
    elif wkind == "v_subb_co_u32":
        new64 = cmask([p0[l] - p1[l] - ((MASKS[2] >> (l % 64)) & 1) < 0 for l in range(n)])
    elif wkind == "v_readfirstlane_b32":
        new64 = [p0[l & ~63] for l in range(n)]
    elif wunit == "SMEM return":
        new64 = [p0[0]] * n
    elif rfile == "SCC":
        new64 = [f[l] for l in range(n)]
    elif use == "VMEM address":
        new64 = None                                             # the input buffer's address
    else:
        new64 = [NEWMASK if wide else NEWMASK & M] * n

    def fill(g, k):
        if st["wait"]:
            g.s_waitcnt(**{st["wait"]: 0})
            k -= 1
        assert k >= 0, "a returning load needs its wait"
        for j in range(k):
            g.v_mov_b32(V(9), j)

    def body(g):
        # ---- ahead of everything: what readers need besides the register under test
        g.v_mov_b32(O(0), SENTINEL)
        g.v_mov_b32(O(1), SENTINEL)
        g.v_add_u32(V_ADDR2, n * 4, V_OFF)                       # plane 1 of the output: where a store-data reader stores
        g.ds_write_b32(V_OFF, I(0))
        g.s_waitcnt(lgkmcnt=0)
        g.v_readfirstlane_b32(S(36), I(4))
        put_mask(g, S(26, 2), NEWMASK)
        put_mask(g, S(28, 2), ~NEWMASK & M64)
        put_mask(g, S(24, 2), MASKS[2])
        # ---- the old value
        if rfile == "VGPR":
            g.v_mov_b32(T, I(2))
        elif rfile == "SCC":
            g.s_cmp_eq_u32(S(36), 0)
        elif rfile == "EXEC":
            g.s_mov_b64(EXEC, S(28, 2))
        elif wkind == "v_readfirstlane_b32":
            g.v_readfirstlane_b32(D32, I(3))
        elif wunit == "SMEM return":
            g.s_mov_b32(D32, ~p0[0] & M)
        elif wkind != "-":                                       # a VALU mask: the complement of what the writer will give
            _writer(g, S(32, 2))
            g.s_andn2_b64(reg, EXEC, S(32, 2))
        elif use == "VMEM address":
            g.s_mov_b64(D, S(6, 2))                              # the output buffer: as valid as the new address
        elif wide:
            g.s_mov_b64(reg, S(28, 2))
        else:
            g.s_mov_b32(D32, ~NEWMASK & M)
        g.s_nop(7)
        # ---- writer, gap, reader
        _writer(g, reg)
        fill(g, gap)
        _reader(g)
        if st["wait"]:
            g.s_waitcnt(**{st["wait"]: 0})
        if rfile == "EXEC":
            g.s_mov_b64(EXEC, -1)
        if st.get("sgpr_out"):
            for k, r in enumerate(st["sgpr_out"]):
                g.v_mov_b32(O(k), r)

    def _writer(g, dst):
        st["wait"] = None
        if wunit == "VALU" and rfile == "VGPR":
            g.v_add_u32(T, I(0), I(1))
        elif wunit == "VMEM return":
            g.global_load_dword(T, V_OFF, S(4, 2))
            st["wait"] = "vmcnt"
        elif wunit == "LDS return":
            g.ds_read_b32(T, V_OFF)
            st["wait"] = "lgkmcnt"
        elif wunit == "SMEM return":
            g.s_load_dword(dst, S(4, 2), 0)
            st["wait"] = "lgkmcnt"
        elif wkind == "v_cmp":
            g.v_cmp_gt_u32(dst, I(0), I(1))
        elif wkind == "v_add_co_u32":
            g.v_add_co_u32(V(8), dst, I(0), I(1))
        elif wkind == "v_sub_co_u32":
            g.v_sub_co_u32(V(8), dst, I(0), I(1))
        elif wkind == "v_subb_co_u32":
            g.v_subb_co_u32(V(8), dst, I(0), I(1), S(24, 2))
        elif wkind == "v_readfirstlane_b32":
            g.v_readfirstlane_b32(dst, I(0))
        elif rfile == "SCC":
            g.s_cmp_lg_u32(S(36), 0)
        elif use == "VMEM address":
            g.s_mov_b64(dst, S(4, 2))
        elif wide:
            g.s_mov_b64(dst, S(26, 2))
        else:
            g.s_mov_b32(dst, NEWMASK & M)

    def _reader(g):
        st["wait"] = None
        if use == "VALU source":
            g.v_xor_b32(O(0), 0x5A5A5A5A, T)
        elif use == "readfirstlane source":
            g.v_readfirstlane_b32(S(30), T)
            st["sgpr_out"] = [S(30)]
        elif use == "VMEM store data":
            g.global_store_dword(V_ADDR2, T, S(6, 2))
        elif use == "LDS store data":
            g.ds_write_b32(V_OFF, T)
            g.s_waitcnt(lgkmcnt=0)
            g.ds_read_b32(O(0), V_OFF)
            st["wait"] = "lgkmcnt"
        elif use == "LDS address":
            g.ds_read_b32(O(0), T)
            st["wait"] = "lgkmcnt"
        elif use == "VMEM address":
            g.global_load_dword(O(0), T if rfile == "VGPR" else V_OFF, S(4, 2) if rfile == "VGPR" else D)
            st["wait"] = "vmcnt"
        elif use == "select mask":
            g.v_cndmask_b32(O(0), I(0), I(3), reg)
        elif use == "carry-in":
            g.v_addc_co_u32(O(0), S(32, 2), I(0), I(1), reg)
        elif use == "scalar constant":
            g.v_add_u32(O(0), D32, I(0))
        elif use == "64-bit pair":
            g.v_mad_u64_u32(O(0, 2), S(32, 2), I(0), I(1), reg)
        elif use == "EXEC of VALU":
            g.v_mov_b32(O(0), I(0))
        elif use == "EXEC of VMEM":
            g.global_load_dword(O(0), V_OFF, S(4, 2))
            st["wait"] = "vmcnt"
        elif use == "EXEC of LDS":
            g.ds_read_b32(O(0), V_OFF)
            st["wait"] = "lgkmcnt"
        elif use == "SALU source":
            if rfile == "SCC":
                g.s_cselect_b64(S(30, 2), -1, 0)
            elif rfile == "EXEC":
                g.s_mov_b64(S(30, 2), EXEC)
            elif wide:
                g.s_and_b64(S(30, 2), reg, EXEC)
            else:
                g.s_add_u32(S(30), D32, 1)
            st["sgpr_out"] = [S(30), S(31)] if wide or rfile in ("SCC", "EXEC") else [S(30)]
        else:
            raise KeyError(use)

    def expect(inp):
        o0, o1 = [SENTINEL] * n, [SENTINEL] * n
        for l in range(n):
            v = new64[l] if new64 is not None else None
            bit = (v >> (l % 64)) & 1 if v is not None else None
            if use == "VALU source":
                o0[l] = newv[l] ^ 0x5A5A5A5A
            elif use == "readfirstlane source":
                o0[l] = newv[l & ~63]
            elif use == "VMEM store data":
                o1[l] = newv[l]
            elif use == "LDS store data":
                o0[l] = newv[l]
            elif use in ("LDS address", "VMEM address"):
                o0[l] = p0[l] if rfile == "SGPR" else inp[0][newv[l] // 4]
            elif use == "select mask":
                o0[l] = na[l] if bit else p0[l]
            elif use == "carry-in":
                o0[l] = p0[l] + p1[l] + bit
            elif use == "scalar constant":
                o0[l] = v + p0[l]
            elif use == "64-bit pair":
                o0[l], o1[l] = (p0[l] * p1[l] + v) & M, ((p0[l] * p1[l] + v) >> 32) & M
            elif use.startswith("EXEC of"):
                o0[l] = p0[l] if bit else SENTINEL
            elif use == "SALU source":
                if rfile == "SCC":
                    o0[l] = o1[l] = M if v else 0
                elif wide or rfile == "EXEC":
                    o0[l], o1[l] = v & M, v >> 32
                else:
                    o0[l] = v + 1
        return [o0, o1]
    u = Unit(name, [], 6, 1 if use == "VMEM store data" else 2, body, inputs, expect, lds_bytes=4 * n, out_init=0xDEADBEEF,
             extra_out=1 if use == "VMEM store data" else 0)
    u.cls, u.gap = cls, gap
    return u
