"""g1_reduce.py -- lean level 1 of the G1 bucket reduction (MNT4-753 / MNT6-753 G1) as gfx950 assembly.

Same inputs, output layout and meaning as mode 2 of csrc/msm_reduce_kernels.h msm_wave_reduce_kernel (which restates the running
sum of algebra/src/msm/variable_base.rs:60-66 without its per-window inversion): one wave per program, lane l owns the items
k = item0 + l + 64 i, and for i = L-1 .. 0:  run += item_i,  then (except after i = 0)  wacc += run.  At the end
out[(blk 64 + l) 2 + {0, 1}] = (run, wacc).  The grid is (segments per window, windows): blk = w segs + seg.

Only the common path of the group law is here.  An operand at infinity is a copy or nothing (no arithmetic), P + (-P) falls
out of the formula (Z = 0), and a lane that meets P + P sets the program's flag: flag[blk] = 1 tells the C++ kernel, launched
behind this one with run_if = flag, to compute the program again from the buckets (it owns the doubling detour).

Register plan (256 VGPRs = two waves per SIMD, 0 bytes of scratch, no LDS):
  v0 lane | v1 4 lane | v[2:6] slab offsets (4 lane + 4096 c) | v[8:9] item address | v[10:11] output address | v12 item index
  v13 flag offset | v14, v15 temporaries | v[20:21], v[22:23] base addresses | v39 temporary
  E0..E7 = v[40 + 26 i ..]: eight field-element slots; chains as in g1_xyzz.py (v[248:255])
run and wacc live in the program's slab (WaveSlab of msm_reduce_kernels.h: slab[(slot 78 + word) 64 + lane]) between steps.

One step = one projective addition in proj_add_raw's order, p = (E0, E1, E2) the destination, q = (E3, E4, E5) the other operand:
  y1z2 -> E6   u -> E7   x1z2 -> E1   v -> E0   z1z2 -> E3   vv -> E4   r -> E2   vvv -> E1   uu -> E5   a -> E4
  X3 -> E5   Z3 -> E0   Y3 = (r - a) u + vvv (-y1z2) -> E3 (one reduction)
The first item step and the first wacc step of a program are copies: they are done as such, so L items cost 2 L - 3 additions.
"""
from .isa import Prog, V, S, EXEC, OFF, fix_hazards
from .field import FieldGen, Chain, interleave, run, NL
from .g1_xyzz import seq

PROJ_WORDS = 3 * NL             # 78
PROJ_BYTES = 4 * PROJ_WORDS     # 312
SLAB_ROW = 64 * 4               # bytes of one word of a slab slot (64 lanes)
SLOT_BYTES = PROJ_WORDS * SLAB_ROW
SLAB_BYTES = 3 * SLOT_BYTES     # run, wacc, and the C++ program's tmp
ROWS_PER_OFF = 16               # a global instruction's immediate offset is below 4096

# SGPR map
S_KARG = S(0, 2)
S_SEG, S_W = S(2), S(3)         # workgroup id x, y
S_ITEMS, S_OUT, S_SLABS, S_FLAG = S(4, 2), S(6, 2), S(8, 2), S(10, 2)
S_STEP, S_NST = S(12), S(13)
S_LM, S_INV = 20, 21
S_P, S_NP = 24, 50
S_COUNT, S_VALID, S_SEGS, S_L = S(76), S(77), S(78), S(79)
S_NPROG, S_ITEM0 = S(80), S(81)
S_RUN, S_WACC, S_DST = S(82, 2), S(84, 2), S(86, 2)
S_ACT, S_QZ, S_PZ = S(88, 2), S(90, 2), S(92, 2)
S_JMP = S(94, 2)
S_ARITH, S_BAD, S_T0 = S(96, 2), S(98, 2), S(100, 2)
S_BLK, S_WCOUNT = S(0), S(1)    # over the kernarg pointer, once the arguments are in
S_312 = S(77)                   # over `valid`, once the padding test is done

V_TID, V_L4 = V(0), V(1)
V_OFF = [V(2 + c) for c in range(5)]
V_ADDR, V_OUT = V(8, 2), V(10, 2)
V_K, V_FLAGOFF = V(12), V(13)
V_T0, V_T1 = V(14), V(15)
V_BASE, V_OUTB = V(20, 2), V(22, 2)
V_TMP = V(39)


def slot(i):
    return V(40 + NL * i, NL)


E = [slot(i) for i in range(8)]
RUN, WACC = 0, 1


def build(name, p, one_mont):
    """p: the base prime; one_mont = 2^754 mod p (internal Montgomery one)."""
    g = Prog(name)
    g.wg_id_y = 1
    for _ in range(4):
        g.add_arg(8, "ptr")
    for _ in range(6):
        g.add_arg(4, "val")
    f = FieldGen(g, p, S_P, S_NP, S_INV, S_LM)
    chA = Chain(V(248, 2), V(252), V(253), S(14, 2), S(16, 2))
    chB = Chain(V(250, 2), V(254), V(255), S(18, 2), S(22, 2))
    L_MAIN, L_LOOP, L_KW, L_KJ, L_NC, L_AR, L_END, L_FIN, L_GO = (
        g.uniq(s) for s in ("main", "loop", "kind_wacc", "kind_join", "no_copy", "arith", "step_end", "fin", "go"))

    def slab_words(sl, first):
        for w in range(NL):
            word = first + w
            yield sl.sub(w), V_OFF[word // ROWS_PER_OFF], (word % ROWS_PER_OFF) * SLAB_ROW

    def slab_ld(sbase, sls):
        for n, sl in enumerate(sls):
            for reg, off, imm in slab_words(sl, n * NL):
                g.global_load_dword(reg, off, sbase, offset=imm)

    def slab_st(sbase, sls):
        for n, sl in enumerate(sls):
            for reg, off, imm in slab_words(sl, n * NL):
                g.global_store_dword(off, reg, sbase, offset=imm)

    def set_infinity(sls):
        for w in range(NL):
            g.v_mov_b32(sls[0].sub(w), 0)
            g.v_mov_b32(sls[2].sub(w), 0)
        run(f.set_const(sls[1], one_mont))

    def load_item(s_i):
        """q = item i of every lane that has one (S_ACT) into E3, E4, E5 (contiguous registers; a wave reads 64 adjacent points)"""
        g.s_lshl_b32(S_T0.lo(), s_i, 6)
        g.s_add_u32(S_T0.lo(), S_T0.lo(), S_ITEM0)
        g.v_add_u32(V_K, S_T0.lo(), V_TID)
        g.v_cmp_gt_u32(S_ACT, S_COUNT, V_K)
        g.v_add_u32(V_T0, S_WCOUNT, V_K)
        g.v_mad_u64_u32(V_ADDR, chB.sdum, V_T0, S_312, V_BASE)
        g.s_mov_b64(EXEC, S_ACT)
        for j in range(PROJ_WORDS // 2):
            g.global_load_dwordx2(V(E[3].idx + 2 * j, 2), V_ADDR, OFF, offset=8 * j)
        g.s_mov_b64(EXEC, -1)

    # ------------------------------------------------------------ prologue
    g.s_load_dwordx8(S(4, 8), S_KARG, 0)
    g.s_load_dwordx4(S(76, 4), S_KARG, 32)
    g.s_load_dword(S_NPROG, S_KARG, 48)
    f.load_constants()
    g.v_lshlrev_b32(V_L4, 2, V_TID)
    g.v_mov_b32(V_OFF[0], V_L4)
    for c in range(1, 5):
        g.v_add_u32(V_OFF[c], c * ROWS_PER_OFF * SLAB_ROW, V_L4)
    g.s_waitcnt(lgkmcnt=0)
    g.s_mul_i32(S_BLK, S_W, S_SEGS)
    g.s_add_u32(S_BLK, S_BLK, S_SEG)
    g.s_cmp_lt_u32(S_BLK, S_NPROG)
    g.s_cbranch_scc1(L_GO)
    g.s_endpgm()
    g.label(L_GO)
    g.s_mul_i32(S_ITEM0, S_SEG, S_L)
    g.s_lshl_b32(S_ITEM0, S_ITEM0, 6)
    g.s_mul_i32(S_WCOUNT, S_W, S_COUNT)
    g.s_mov_b32(S_T0.hi(), 2 * PROJ_BYTES)
    g.v_mov_b32(V_T0, S_BLK)
    g.v_lshl_add_u32(V_T0, V_T0, 6, V_TID)
    g.v_mov_b32(V_OUTB.lo(), S_OUT.lo()); g.v_mov_b32(V_OUTB.hi(), S_OUT.hi())
    g.v_mov_b32(V_BASE.lo(), S_ITEMS.lo()); g.v_mov_b32(V_BASE.hi(), S_ITEMS.hi())
    g.v_mad_u64_u32(V_OUT, chB.sdum, V_T0, S_T0.hi(), V_OUTB)
    g.v_mov_b32(V_FLAGOFF, S_BLK)
    g.v_lshlrev_b32(V_FLAGOFF, 2, V_FLAGOFF)
    g.s_mov_b64(S_BAD, 0)
    # a segment of padding only: both sums are the point at infinity
    g.s_add_u32(S_T0.lo(), S_WCOUNT, S_ITEM0)
    g.s_cmp_ge_u32(S_T0.lo(), S_VALID)
    g.s_cbranch_scc0(L_MAIN)
    set_infinity(E[0:3])
    for j in range(PROJ_WORDS // 2):
        g.global_store_dwordx2(V_OUT, V(E[0].idx + 2 * j, 2), OFF, offset=8 * j)
        g.global_store_dwordx2(V_OUT, V(E[0].idx + 2 * j, 2), OFF, offset=PROJ_BYTES + 8 * j)
    g.v_mov_b32(V_T0, 0)
    g.s_mov_b64(EXEC, 1)
    g.global_store_dword(V_FLAGOFF, V_T0, S_FLAG)
    g.s_endpgm()

    g.label(L_MAIN)
    # this program's slab: slabs + blk * SLAB_BYTES
    g.s_mov_b32(S_T0.hi(), SLAB_BYTES)
    g.s_mul_i32(S_T0.lo(), S_BLK, S_T0.hi())
    g.s_mul_hi_u32(S_T0.hi(), S_BLK, S_T0.hi())
    g.s_add_u32(S_RUN.lo(), S_SLABS.lo(), S_T0.lo())
    g.s_addc_u32(S_RUN.hi(), S_SLABS.hi(), S_T0.hi())
    g.s_add_u32(S_WACC.lo(), S_RUN.lo(), SLOT_BYTES)
    g.s_addc_u32(S_WACC.hi(), S_RUN.hi(), 0)
    g.s_mov_b32(S_312, PROJ_BYTES)
    # item L - 1 is the first value of run and of wacc (lanes without one: infinity)
    g.s_sub_u32(S_STEP, S_L, 1)
    load_item(S_STEP)
    g.s_waitcnt(vmcnt=0)
    g.s_andn2_b64(EXEC, EXEC, S_ACT)
    set_infinity(E[3:6])
    g.s_mov_b64(EXEC, -1)
    slab_st(S_RUN, E[3:6])
    slab_st(S_WACC, E[3:6])
    g.s_lshl_b32(S_NST, S_L, 1)
    g.s_sub_u32(S_NST, S_NST, 3)                                     # 2 L - 3 additions (L >= 2: the launcher checks)
    g.s_mov_b32(S_STEP, 0)
    g.s_waitcnt(vmcnt=0)

    # ------------------------------------------------------------ one step: even = run += item_i, odd = wacc += run; i = L - 2 - step / 2
    g.label(L_LOOP)
    g.s_and_b32(S_T0.lo(), S_STEP, 1)
    g.s_cbranch_scc1(L_KW)
    g.s_lshr_b32(S_T0.lo(), S_STEP, 1)
    g.s_sub_u32(S_DST.lo(), S_L, 2)
    g.s_sub_u32(S_DST.lo(), S_DST.lo(), S_T0.lo())
    load_item(S_DST.lo())
    g.s_mov_b64(S_DST, S_RUN)
    g.s_branch(L_KJ)
    g.label(L_KW)
    g.s_mov_b64(S_ACT, -1)
    slab_ld(S_RUN, E[3:6])
    g.s_mov_b64(S_DST, S_WACC)
    g.label(L_KJ)
    slab_ld(S_DST, E[0:3])
    g.s_waitcnt(vmcnt=0)
    interleave(f.is_zero_mask(chA, E[5], S_QZ), f.is_zero_mask(chB, E[2], S_PZ))
    g.s_andn2_b64(S_ACT, S_ACT, S_QZ)                               # lanes whose q counts: the others keep their destination
    g.s_andn2_b64(S_ARITH, S_ACT, S_PZ)
    g.s_and_b64(EXEC, S_ACT, S_PZ)                                  # destination at infinity: it becomes q
    g.s_cbranch_execz(L_NC)
    slab_st(S_DST, E[3:6])
    g.label(L_NC)
    g.s_mov_b64(EXEC, S_ARITH)
    g.s_cbranch_execnz(L_AR)
    g.long_branch(L_END, S_JMP)
    g.label(L_AR)

    seq(f.mul(chA, E[1], E[5], E[6], E[1]),                         # y1z2 = Y1 Z2   -> E6
        f.mul(chB, E[2], E[4], E[7], E[4]))                         # Z1 Y2          -> E7
    run(f.sub(chA, E[7], E[6], E[7]))                               # u              -> E7
    seq(f.mul(chA, E[0], E[5], E[1], E[0]),                         # x1z2 = X1 Z2   -> E1
        f.mul(chB, E[2], E[3], E[0], E[3]))                         # Z1 X2          -> E0
    run(f.sub(chA, E[0], E[1], E[0]))                               # v              -> E0
    run(f.mul(chA, E[2], E[5], E[3], E[2]))                         # z1z2           -> E3   (p, q dead)
    # p == q as points (neither at infinity here): the program is computed again by the C++ kernel
    interleave(f.is_zero_mask(chA, E[7], S_T0), f.is_zero_mask(chB, E[0], S_JMP))
    g.s_and_b64(S_T0, S_T0, S_JMP)
    g.s_or_b64(S_BAD, S_BAD, S_T0)
    run(f.sqr(chA, E[0], E[2], E[4]))                               # vv             -> E4
    seq(f.mul(chA, E[4], E[1], E[2], E[1]),                         # r = vv x1z2    -> E2
        f.mul(chB, E[0], E[4], E[1], E[4]))                         # vvv = v vv     -> E1
    run(f.sqr(chA, E[7], E[4], E[5]))                               # uu             -> E5
    run(f.mul(chA, E[5], E[3], E[4], E[5]))                         # uu z1z2        -> E4
    run(f.sub(chA, E[4], E[1], E[4]))                               # a = uu z1z2 - vvv - 2 r -> E4
    run(f.sub(chA, E[4], E[2], E[4]))
    run(f.sub(chA, E[4], E[2], E[4]))
    seq(f.mul(chA, E[0], E[4], E[5], E[0]),                         # X3 = v a       -> E5
        f.mul(chB, E[1], E[3], E[0], E[3]))                         # Z3 = vvv z1z2  -> E0
    slab_st(S_DST, [E[5]])
    run(f.sub(chA, E[2], E[4], E[2]))                               # r - a          -> E2
    g.s_mov_b64(S_T0, -1)
    run(f.neg_sel(chA, E[6], V_TMP, S_T0))                          # -y1z2 (p where y1z2 == 0: a product accepts it)
    run(f.dual(chA, chB, E[2], E[7], E[1], E[6], E[3], E[4]))       # Y3             -> E3
    for n, sl in ((1, E[3]), (2, E[0])):
        for reg, off, imm in slab_words(sl, n * NL):
            g.global_store_dword(off, reg, S_DST, offset=imm)

    g.label(L_END)
    g.s_mov_b64(EXEC, -1)
    g.s_waitcnt(vmcnt=0)
    g.s_add_u32(S_STEP, S_STEP, 1)
    g.s_cmp_lt_u32(S_STEP, S_NST)
    g.s_cbranch_scc0(L_FIN)
    g.long_branch(L_LOOP, S_JMP)

    # ------------------------------------------------------------ epilogue: (run, wacc) of every lane, the program's flag
    g.label(L_FIN)
    slab_ld(S_RUN, E[0:3])
    slab_ld(S_WACC, E[3:6])
    g.s_cmp_lg_u64(S_BAD, 0)
    g.s_cselect_b64(S_T0, 1, 0)
    g.v_mov_b32(V_T0, S_T0.lo())
    g.s_waitcnt(vmcnt=0)
    for j in range(PROJ_WORDS):
        g.global_store_dwordx2(V_OUT, V(E[0].idx + 2 * j, 2), OFF, offset=8 * j)
    g.s_mov_b64(EXEC, 1)
    g.global_store_dword(V_FLAGOFF, V_T0, S_FLAG)
    g.s_endpgm()
    g.hazard_nops = fix_hazards(g)      # isa.py: the gfx950 VALU -> SGPR -> VALU wait states
    return g
