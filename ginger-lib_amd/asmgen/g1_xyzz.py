"""g1_xyzz.py -- the G1 bucket accumulation kernel (MNT4-753 / MNT6-753 G1) as gfx950 assembly.

Same task list, list walk, salt detour and output as csrc/msm_kernels.h msm_accumulate_xyzz_kernel (which restates the
bucket loop of algebra/src/msm/variable_base.rs:36-59 with add_assign_mixed, swp.rs:481-519, replaced by madd-2008-s on
(X, Y, ZZ, ZZZ) accumulators): one thread per task, every list entry one mixed addition.

Register plan (256 VGPRs = two waves per SIMD, 0 bytes of scratch):
  v0 tid | v1 LDS address | v[2:3] list cursor | v4 entries left | v5 phase | v6 sigma | v7 salt id | v[8:9] dst
  v[10:11] gather address | v12 list entry | v13 guard | v14..v19 temporaries | v[20:21] bases | v[22:23] salts | v39 temp
  E0..E7 = v[40 + 26 i ..]: eight field-element slots; E0 = ZZ, E1 = ZZZ for the whole task
  chain A: v[248:249] accumulator, v252, v253;  chain B: v[250:251], v254, v255
  X, V = sigma Y and (between two steps) R^2 of the running sum are parked in LDS, word-major: park[3][26][256].
The prime, -p, the Montgomery constant and the limb mask live in SGPRs.

Two launch forms of the same update (nothing between L_LOOP and L_ADV differs):
  block (default)   a workgroup of four waves takes the 256 tasks its id names and ends; the grid is one block per 256 tasks.
  persistent=True   a workgroup is ONE wave (park[3][26][64], 19 968 B of LDS: eight per CU hold what two blocks hold) that
                    loads the constants once and then takes tiles of 64 consecutive tasks from a 32-bit counter in global memory
                    (one lane, a returning global_atomic_add; relaxed: nothing is handed over through the counter) until the
                    counter has passed n_tiles, or until it has taken `budget` tiles (0: no limit; the host launches at least
                    n_tiles / budget waves).  No wave waits for another: any grid size and any residency give the same
                    buckets, and a wave that starts after the counter ran out ends having stored nothing.  The counter must
                    be 0 when the launch starts (msm_kernels.h msm_acc_tasks_kernel writes it).
debug=True adds stamps (shader clock, constant-rate clock, hardware id) per tile / per wave of a block into a side buffer;
the shipped kernels hold none (build.py: GH_ASM_DEBUG).

Order of the products (each one chain of mads, one after the other):
  U2, S2  P, W  PP, RR  zero tests  park RR  PPP, ZZ3  Q, ZZZ3  X3, T  dual(W T + V PPP)

The lazy forms (csrc/ec29.h xyzz_madd_lazy restates the update limb for limb).  Table rows, the task
table and the stored buckets are as before (x R, fully reduced); the running sum is private to the kernel and lives in the
forms the 27-digit reduction REDC27(a, b) = a b (R D)^-1 (field.py, D = 2^29) closes on:
  X R D, V R D (parked)   ZZ R D^2, ZZZ R D^2 (registers)   U2, S2, P, W, PP, RR, PPP, Q, X3, T and the dual product: R D
REDC27 returns less than a b / (R D) + p, "almost reduced" (below p + 2^733) whatever its operands were, so no product has a
conditional subtraction behind it, and the differences are carry-normalised a - b + k p with an unmasked top limb:
  P = U2 - X + 8 p in (3 p, 9 p)   W = S2 - V + 2 p in (p, 3 p)   X3 = RR - PPP - 2 Q + 4 p in (p, 5 p), parked unreduced
  T = X3 - Q + 2 p in (2 p, 7 p)
field.py checks every product's columns against these declared bounds when the kernel is built; the dual product closes the
columns that could pass 2^64 in two parts.  A zero is 0 or p: "the sum is infinity" is ZZ in {0, p}, "acc == q" is PP and RR in
{0, p}, tested after the two squarings (nothing is parked before).  L_INIT converts q into the forms (two products by
c = R D^2 mod p), the epilogue converts back: x = REDC27(X, ZZZ), y = REDC27(Y, ZZ), z = REDC27(REDC27(ZZ, ZZZ), R) all carry
R D^2 -- the same projective point -- and get the kernel's only conditional subtractions.
"""
from .isa import Prog, V, S, VCC, EXEC, OFF, fix_hazards
from .field import FieldGen, Chain, Bound, run, runv, NL, LB

AFF_BYTES = 2 * NL * 4          # 208
PROJ_WORDS = 3 * NL             # 78
PARK_X, PARK_V, PARK_RR = 0, 1, 2
LDS_BYTES = 3 * NL * 256 * 4    # block form; the persistent form parks 64 lanes: a quarter

# SGPR map
S_KARG = S(0, 2)
S_WG = S(2)
S_BASES, S_SORTED, S_TASKS, S_SALTS = S(4, 2), S(6, 2), S(8, 2), S(10, 2)
S_NTASKS = S(12)
S_208 = S(13)
S_LM, S_INV = 20, 21
S_P, S_NP = 24, 50
S_ACTIVE = S(76, 2)
S_NEGSEL = S(78, 2)
S_T0, S_T1 = S(80, 2), S(82, 2)
S_LAUNCH = S(84, 2)
S_SAVE = S(86, 2)
S_DETOUR = S(88, 2)
S_T2 = S(90, 2)
S_ZERO = S(92, 2)
# persistent form: the tile counter's address, the number of tiles, the tile in hand
S_CTR = S(96, 2)
S_NTILES = S(98)
S_TILE = S(99)
S_BUDGET = S(3)                 # tiles this wave may still take (the launch's budget; 0 = no limit)
S_STAMPS = S(100, 2)            # debug form: the stamp records
STAMP_BYTES = 64                # a record: clk0, rt0 | clk1, rt1 | hw id, xcc id, index, live lanes (low word) | unused

V_TID, V_LDS = V(0), V(1)
V_CUR = V(2, 2)
V_LEFT, V_PHASE, V_SNEG, V_SALT = V(4), V(5), V(6), V(7)
V_DST = V(8, 2)
V_ADDR = V(10, 2)
V_E = V(12)
V_GUARD = V(13)
V_T = [V(14), V(15), V(16), V(17), V(18), V(19)]
V_BASES, V_SALTS = V(20, 2), V(22, 2)
V_TMP = V(39)
V_LDS2 = V(24)
V_ENEXT = V(25)
V_TOUCH = V(26)
V_NADDR = V(28, 2)
# debug form (never together with prefetch): the start stamps, the end stamps, the ids, the record's offset
V_ST0, V_ST1, V_STID, V_STOFF = V(30, 4), V(34, 4), V(26, 4), V(38)


def slot(i):
    return V(40 + NL * i, NL)


def seq(*gens):
    """The products of a pair one after the other (g1_reduce.py).  (Rounds 2-4 interleaved them instruction by instruction on two
    accumulator chains; measured on the card, tools/asm_mb mul_seq2 / sqr_seq2 against mul_pair / sqr_pair, the sequential form is
    1.6 % / 2.6 % faster at two waves per SIMD: a v_mad_u64_u32 whose 64-bit addend is its predecessor's result does not read it
    from the register file.)"""
    for gen in gens:
        run(gen)


E = [slot(i) for i in range(8)]


def build(name, p, one_mont, prefetch=False, split=4, persistent=False, debug=False):
    """p: the base prime; one_mont = 2^754 mod p (internal Montgomery one).
    Arguments: bases, sorted, tasks, salts, n_tasks; persistent: + n_tiles, counter, budget; debug: + stamps (last)."""
    assert not (debug and prefetch)
    g = Prog(name)
    lanes = 64 if persistent else 256
    park_stride = lanes * 4                                         # bytes between consecutive words of a parked element
    g.lds_bytes = 3 * NL * park_stride
    for _ in range(4):
        g.add_arg(8, "ptr")
    g.add_arg(4, "val")
    if persistent:
        g.add_arg(4, "val")
        off_ctr = g.add_arg(8, "ptr")
        off_budget = g.add_arg(4, "val")
    if debug:
        off_stamps = g.add_arg(8, "ptr")
    f = FieldGen(g, p, S_P, S_NP, S_INV, S_LM)
    chA = Chain(V(248, 2), V(252), V(253), S(14, 2), S(16, 2))
    chB = Chain(V(250, 2), V(254), V(255), S(18, 2), S(22, 2))
    # The lazy forms (module docstring): what each value of the update may reach.  AR = "almost reduced", the result of any
    # REDC27 whose operands stay below 2^758; the routines of field.py check every product's columns against these bounds and
    # return their result's bound, which is checked against the declaration it feeds (`within`).
    c_lazy = one_mont * (1 << (2 * LB)) % p                         # R D^2 mod p: ZZ = ZZZ = 1 in the accumulator's form
    AR = Bound(1, 1 << 733)
    B_TAB = Bound(1)                                                # a table row, and q.y after neg_sel (at most p)
    B_X = Bound(5, 1 << 733)                                        # the parked X: RR - PPP - 2 Q + 4 p

    def within(b, decl):
        assert b.value(p) <= decl.value(p), (b, decl)
        return decl

    def mul27(ch, a, b, m, ba, bb, r=None, decl=AR):
        return within(runv(f.mul27(ch, a, b, m, ba, bb, r)), decl)

    def park_addr(which, w):
        # DS offsets are 16 bits: the third parked element is addressed from a second base register
        if which < 2:
            return V_LDS, (which * NL + w) * park_stride
        return V_LDS2, ((which - 2) * NL + w) * park_stride

    def park_put(which, sl):
        for w in range(NL):
            a, off = park_addr(which, w)
            g.ds_write_b32(a, sl.sub(w), offset=off)

    def park_get(which, sl):
        for w in range(NL):
            a, off = park_addr(which, w)
            g.ds_read_b32(sl.sub(w), a, offset=off)

    L_LOOP, L_INIT, L_INIT_RET, L_DETOUR, L_DET_RET, L_ADV, L_DONE, L_START = (
        g.uniq(s) for s in ("loop", "init", "init_ret", "detour", "det_ret", "adv", "done", "start"))
    S_JMP = S(94, 2)                                                # scratch of the long jumps

    def stamp(dst):
        """dst[0:2] = shader clock, dst[2:4] = constant-rate clock (S_T0 / S_T1 are free outside the loop)"""
        g.s_memtime(S_T0)
        g.s_memrealtime(S_T1)
        g.s_waitcnt(lgkmcnt=0)
        g.v_mov_b32(dst.sub(0), S_T0.lo()); g.v_mov_b32(dst.sub(1), S_T0.hi())
        g.v_mov_b32(dst.sub(2), S_T1.lo()); g.v_mov_b32(dst.sub(3), S_T1.hi())

    def stamp_store():
        """the record of this tile / wave, by every live lane alike (ordinary vector stores into the side buffer)"""
        stamp(V_ST1)
        g.s_getreg_b32(S_T0.lo(), "hwreg(HW_REG_HW_ID)")
        g.s_getreg_b32(S_T0.hi(), "hwreg(HW_REG_XCC_ID)")
        g.v_mov_b32(V_STID.sub(0), S_T0.lo()); g.v_mov_b32(V_STID.sub(1), S_T0.hi())
        g.v_mov_b32(V_STID.sub(3), S_LAUNCH.lo())
        for k, r in enumerate((V_ST0, V_ST1, V_STID)):
            g.global_store_dwordx4(V_STOFF, r, S_STAMPS, offset=16 * k)

    def wave_constants():
        g.v_mov_b32(V_BASES.lo(), S_BASES.lo()); g.v_mov_b32(V_BASES.hi(), S_BASES.hi())
        g.v_mov_b32(V_SALTS.lo(), S_SALTS.lo()); g.v_mov_b32(V_SALTS.hi(), S_SALTS.hi())

    def reset_task(v_task, with_constants=False):
        """the task row of v_task and the state of an empty running sum; ends in front of L_LOOP"""
        g.v_lshlrev_b32(V_T[1], 4, v_task)
        g.global_load_dwordx4(V(16, 4), V_T[1], S_TASKS)            # beg, cnt, dst
        if with_constants:
            wave_constants()
        g.v_mov_b32(V_CUR.lo(), S_SORTED.lo()); g.v_mov_b32(V_CUR.hi(), S_SORTED.hi())
        g.v_mov_b32(V_PHASE, 0); g.v_mov_b32(V_SNEG, 0); g.v_mov_b32(V_SALT, 0)
        for w in range(NL):                                         # ZZ = ZZZ = 0: the running sum is the point at infinity
            g.v_mov_b32(E[0].sub(w), 0)
            g.v_mov_b32(E[1].sub(w), 0)
        g.s_waitcnt(vmcnt=0)
        g.v_mov_b32(V_LEFT, V(17))
        g.v_mov_b32(V_DST.lo(), V(18)); g.v_mov_b32(V_DST.hi(), V(19))
        g.v_mad_u64_u32(V_CUR, chA.sdum, V(16), 4, V_CUR)
        g.v_lshl_add_u32(V_GUARD, V_LEFT, 2, 8)                     # at most 4 cnt + 8 iterations (the C++ kernel's guard)

    # ------------------------------------------------------------ prologue
    L_FETCH, L_EXIT = g.uniq("fetch"), g.uniq("exit")
    if debug and not persistent:
        stamp(V_ST0)
    g.s_load_dwordx8(S(4, 8), S_KARG, 0)
    g.s_load_dword(S_NTASKS, S_KARG, 32)
    if persistent:
        g.s_load_dword(S_NTILES, S_KARG, 36)
        g.s_load_dwordx2(S_CTR, S_KARG, off_ctr)
        g.s_load_dword(S_BUDGET, S_KARG, off_budget)
    if debug:
        g.s_load_dwordx2(S_STAMPS, S_KARG, off_stamps)
    f.load_constants()
    g.s_mov_b32(S_208, AFF_BYTES)
    g.v_lshlrev_b32(V_LDS, 2, V_TID)
    g.v_add_u32(V_LDS2, 2 * NL * park_stride, V_LDS)
    if not persistent:
        g.v_lshl_or_b32(V_T[0], S_WG, 8, V_TID)
        g.s_waitcnt(lgkmcnt=0)
        g.v_cmp_gt_u32(VCC, S_NTASKS, V_T[0])
        g.s_and_saveexec_b64(S_LAUNCH, VCC)
        g.s_cbranch_execnz(L_START)
        g.s_endpgm()
        g.label(L_START)
        g.s_mov_b64(S_LAUNCH, EXEC)
        if debug:                                                   # one record per wave of the block: 4 wg + wave
            g.v_lshrrev_b32(V_STID.sub(2), 6, V_T[0])
            g.v_lshlrev_b32(V_STOFF, 6, V_STID.sub(2))
        reset_task(V_T[0], with_constants=True)
        g.s_branch(L_LOOP)
    else:
        g.s_waitcnt(lgkmcnt=0)
        wave_constants()
        # -------------------------------------------------------- tile loop: one lane draws the next tile
        g.label(L_FETCH)
        g.s_mov_b64(EXEC, 1)
        g.v_mov_b32(V_T[0], 1)
        g.v_mov_b32(V_T[1], 0)
        g.global_atomic_add(V_T[2], V_T[1], V_T[0], S_CTR, sc0=True)   # sc0: the count before the add
        g.s_waitcnt(vmcnt=0)                                        # (also the stores of the tile before)
        g.v_readfirstlane_b32(S_TILE, V_T[2])
        g.s_mov_b64(EXEC, -1)
        g.s_cmp_ge_u32(S_TILE, S_NTILES)
        g.s_cbranch_scc1(L_EXIT)
        g.v_lshl_or_b32(V_T[0], S_TILE, 6, V_TID)
        g.v_cmp_gt_u32(VCC, S_NTASKS, V_T[0])                       # the last tile may be ragged
        g.s_and_b64(EXEC, EXEC, VCC)
        g.s_cbranch_execz(L_FETCH)
        g.s_mov_b64(S_LAUNCH, EXEC)
        if debug:                                                   # one record per tile
            stamp(V_ST0)
            g.v_mov_b32(V_STID.sub(2), S_TILE)
            g.v_lshlrev_b32(V_STOFF, 6, V_STID.sub(2))
        reset_task(V_T[0])
        g.s_branch(L_LOOP)
        g.label(L_EXIT)
        g.s_endpgm()

    # ------------------------------------------------------------ epilogue: (X ZZZ : Y ZZ : ZZ ZZZ), infinity -> (0, 1, 0)
    g.label(L_DONE)
    g.s_mov_b64(EXEC, S_LAUNCH)
    f.zero_or_p_mask(chA, E[0], S_ZERO, S_T0)
    # lanes that never parked anything (empty task) read whatever LDS holds: their products wrap harmlessly and their result is
    # replaced below
    park_get(PARK_X, E[2])
    park_get(PARK_V, E[3])
    g.v_cmp_ne_u32(S_NEGSEL, 0, V_SNEG)
    g.s_waitcnt(lgkmcnt=0)
    b_neg = runv(f.lazy_diff(chA, None, [(E[3], 1)], 1, E[4], None, [AR]))        # 2 p - V: Y where sigma is set
    for w in range(NL):
        g.v_cndmask_b32(E[3].sub(w), E[3].sub(w), E[4].sub(w), S_NEGSEL)
    mul27(chA, E[2], E[1], E[4], B_X, AR)                           # x = X ZZZ -> E4   (all three in the form R D^2)
    mul27(chB, E[3], E[0], E[5], b_neg, AR)                         # y = Y ZZ  -> E5
    mul27(chA, E[0], E[1], E[6], AR, AR)                            # ZZ ZZZ in the form R D^3 -> E6
    run(f.set_const(E[7], one_mont))
    mul27(chA, E[6], E[7], E[2], AR, B_TAB, r=E[6])                 # z: times R, the reduction takes one D back
    run(f.cond_sub(chA, E[4], E[2], E[4]))                          # the output is fully reduced
    run(f.cond_sub(chA, E[5], E[2], E[5]))
    run(f.cond_sub(chA, E[6], E[2], E[6]))
    g.s_mov_b64(S_SAVE, EXEC)
    g.s_and_b64(EXEC, EXEC, S_ZERO)
    for w in range(NL):
        g.v_mov_b32(E[4].sub(w), 0)
        g.v_mov_b32(E[6].sub(w), 0)
    run(f.set_const(E[5], one_mont))
    g.s_mov_b64(EXEC, S_SAVE)
    for j in range(PROJ_WORDS // 2):                                # E4, E5, E6 are contiguous: Proj = x[26] y[26] z[26]
        g.global_store_dwordx2(V_DST, V(E[4].idx + 2 * j, 2), OFF, offset=8 * j)
    if debug:
        stamp_store()
    if persistent:
        # a wave that has used up its budget ends, so that the dispatcher can hand its slot to whatever waits -- the next
        # workgroup of this grid, or a kernel of another stream.  A budget of 0 wraps: no limit.
        g.s_sub_u32(S_BUDGET, S_BUDGET, 1)
        g.s_cmp_eq_u32(S_BUDGET, 0)
        g.s_cbranch_scc0(L_FETCH)
        g.s_endpgm()
    else:
        g.s_endpgm()

    # ------------------------------------------------------------ loop head
    g.label(L_LOOP)
    g.s_mov_b64(EXEC, S_LAUNCH)
    g.v_cmp_ne_u32(S_ACTIVE, 0, V_LEFT)
    g.v_cmp_ne_u32(S_T0, 0, V_GUARD)
    g.s_and_b64(S_ACTIVE, S_ACTIVE, S_T0)
    g.s_mov_b64(S_DETOUR, 0)
    g.s_and_b64(EXEC, S_ACTIVE, EXEC)
    g.s_cbranch_execz(L_DONE)
    # the entry of phases 0 / 2 (read by every active lane: the cursor stays inside the list while entries are left)
    g.global_load_dword(V_E, V_CUR, OFF)
    if prefetch:                                                    # the entry after this one (the same again at the end of the list)
        g.v_cmp_lt_u32(S_T1, 1, V_LEFT)
        g.v_cndmask_b32(V_T[2], 0, 4, S_T1)
        g.v_add_co_u32(V_NADDR.lo(), VCC, V_CUR.lo(), V_T[2])
        g.v_addc_co_u32(V_NADDR.hi(), VCC, 0, V_CUR.hi(), VCC)
        g.global_load_dword(V_ENEXT, V_NADDR, OFF)
    g.v_and_b32(V_T[1], 1, V_PHASE)
    g.v_cmp_ne_u32(S_T0, 0, V_T[1])                                 # S_T0 = lanes in a salt phase (1, 3)
    g.v_mad_u64_u32(V(16, 2), chA.sdum, V_SALT, S_208, V_SALTS)
    g.s_waitcnt(vmcnt=0)
    g.v_and_b32(V_T[0], 0x7FFFFFFF, V_E)
    g.v_mad_u64_u32(V_ADDR, chA.sdum, V_T[0], S_208, V_BASES)
    g.v_cndmask_b32(V_ADDR.lo(), V_ADDR.lo(), V(16), S_T0)
    g.v_cndmask_b32(V_ADDR.hi(), V_ADDR.hi(), V(17), S_T0)
    # E2 = q.x, E3 = q.y (contiguous).  Every lane reads its own row: one wave-wide load touches 64 pages, more than the L1 TLB
    # holds, so each of a row's 13 loads would miss all of its translations again (profiles/r02_affine_rounds_counters.txt:
    # TCP_UTCL1_TRANSLATION_MISS 13 per row).  A part of the wave at a time, all 13 loads of its rows back to back.
    if split > 1:
        g.s_mov_b64(S_SAVE, EXEC)
    for q in range(split):
        if split > 1:
            g.s_bfm_b64(S_T1, 64 // split, (64 // split) * q)
            g.s_and_b64(EXEC, S_SAVE, S_T1)
        for j in range(AFF_BYTES // 16):
            g.global_load_dwordx4(V(E[2].idx + 4 * j, 4), V_ADDR, OFF, offset=16 * j)
    if split > 1:
        g.s_mov_b64(EXEC, S_SAVE)
    # negate q.y on lanes where (entry sign, or phase == 3 for the salt) != sigma
    g.v_lshrrev_b32(V_T[0], 31, V_E)
    g.v_lshrrev_b32(V_T[1], 1, V_PHASE)
    g.v_cndmask_b32(V_T[0], V_T[0], V_T[1], S_T0)
    g.v_xor_b32(V_T[0], V_T[0], V_SNEG)
    g.v_cmp_ne_u32(S_NEGSEL, 0, V_T[0])
    g.s_waitcnt(vmcnt=0)
    if prefetch:
        # Touch the NEXT entry's row (its four 64-byte lines) now, a whole update ahead: the gathers are one row per lane out of a
        # multi-GB table, i.e. 64 address translations per wave instruction; with the lines and translations warm the
        # gather at the top of the next iteration returns from L2 (tools/asm_mb/acc_run: 74.5 K -> 68.7 K cycles per update
        # is the cost of the cold gather).  The loaded words are never read.
        g.v_and_b32(V_T[2], 0x7FFFFFFF, V_ENEXT)
        g.v_mad_u64_u32(V_NADDR, chA.sdum, V_T[2], S_208, V_BASES)
        for j in range(4):
            g.global_load_dword(V_TOUCH, V_NADDR, OFF, offset=min(64 * j, AFF_BYTES - 4))
    run(f.neg_sel(chA, E[3], V_TMP, S_NEGSEL))
    f.zero_or_p_mask(chA, E[0], S_ZERO, S_T0)                       # the running sum is infinity: ZZ = 0 mod p
    g.s_cmp_lg_u64(S_ZERO, 0)
    g.s_cbranch_scc0(L_INIT_RET)
    g.long_branch(L_INIT, S_JMP)
    g.label(L_INIT_RET)

    # ------------------------------------------------------------ the update
    mul27(chA, E[2], E[0], E[4], B_TAB, AR)                         # U2 = q.x ZZ   -> E4
    mul27(chB, E[3], E[1], E[5], B_TAB, AR)                         # S2 = q.y ZZZ  -> E5
    park_get(PARK_X, E[2])
    park_get(PARK_V, E[3])
    g.s_waitcnt(lgkmcnt=0)
    b_p = runv(f.lazy_diff(chA, E[4], [(E[2], 1)], 3, E[4], AR, [B_X]))           # P = U2 - X + 8 p -> E4: (3 p, 9 p)
    b_w = runv(f.lazy_diff(chB, E[5], [(E[3], 1)], 1, E[5], AR, [AR]))            # W = S2 - V + 2 p -> E5: (p, 3 p)
    within(runv(f.sqr27(chA, E[4], E[2], E[6], b_p)), AR)           # PP = P^2      -> E6
    within(runv(f.sqr27(chB, E[5], E[3], E[7], b_w)), AR)           # RR = W^2      -> E7
    # acc == q (P = 0 and W = 0 mod p, i.e. PP and RR in {0, p}, in phase 0): the salt detour.  Nothing is parked yet.
    f.zero_or_p_mask(chA, E[6], S_T0, S_T2)
    f.zero_or_p_mask(chB, E[7], S_T1, S_T2)
    g.v_cmp_eq_u32(S_T2, 0, V_PHASE)
    g.s_and_b64(S_T0, S_T0, S_T1)
    g.s_and_b64(S_DETOUR, S_T0, S_T2)
    g.s_cbranch_scc0(L_DET_RET)
    g.long_branch(L_DETOUR, S_JMP)
    g.label(L_DET_RET)
    park_put(PARK_RR, E[7])
    mul27(chA, E[4], E[6], E[2], b_p, AR, r=E[4])                   # PPP = P PP    -> E4
    mul27(chB, E[0], E[6], E[3], AR, AR, r=E[0])                    # ZZ3 = ZZ PP   -> E0
    park_get(PARK_X, E[2])
    g.s_waitcnt(lgkmcnt=0)
    mul27(chA, E[2], E[6], E[3], B_X, AR, r=E[2])                   # Q = X PP      -> E2
    mul27(chB, E[1], E[4], E[7], AR, AR, r=E[1])                    # ZZZ3 = ZZZ PPP -> E1
    park_get(PARK_RR, E[3])
    g.s_waitcnt(lgkmcnt=0)
    within(runv(f.lazy_diff(chA, E[3], [(E[4], 1), (E[2], 2)], 2, E[3], AR, [AR, AR])), B_X)    # X3 = RR - PPP - 2 Q + 4 p -> E3
    park_put(PARK_X, E[3])
    park_get(PARK_V, E[6])
    b_t = runv(f.lazy_diff(chA, E[3], [(E[2], 1)], 1, E[2], B_X, [AR]))           # T = X3 - Q + 2 p -> E2: (2 p, 7 p)
    g.s_waitcnt(lgkmcnt=0)
    # W T + V PPP = -sigma Y3 -> E7: the new V, sigma flips.  W and T stay lazy: the columns that can pass 2^64 close in two parts
    within(runv(f.dual27(chA, chB, E[5], E[2], E[6], E[4], E[7], b_w, b_t, AR, AR)), AR)
    g.dual_split = f.last_split
    park_put(PARK_V, E[7])
    g.v_xor_b32(V_SNEG, 1, V_SNEG)

    # ------------------------------------------------------------ advance
    g.label(L_ADV)
    g.s_andn2_b64(EXEC, S_ACTIVE, S_DETOUR)
    g.v_cmp_eq_u32(S_T0, 0, V_PHASE)
    g.v_cmp_eq_u32(S_T1, 3, V_PHASE)
    g.s_or_b64(S_T0, S_T0, S_T1)                                    # lanes that move on to the next entry
    g.v_add_u32(V_T[0], 1, V_PHASE)
    g.v_cndmask_b32(V_PHASE, V_T[0], 0, S_T0)
    g.v_cndmask_b32(V_T[0], 0, 1, S_T0)
    g.v_sub_u32(V_LEFT, V_LEFT, V_T[0])
    g.v_lshlrev_b32(V_T[0], 2, V_T[0])
    g.v_add_co_u32(V_CUR.lo(), VCC, V_CUR.lo(), V_T[0])
    g.v_addc_co_u32(V_CUR.hi(), VCC, 0, V_CUR.hi(), VCC)
    g.s_mov_b64(EXEC, S_ACTIVE)
    g.v_subrev_u32(V_GUARD, 1, V_GUARD)
    g.long_branch(L_LOOP, S_JMP)

    # ------------------------------------------------------------ rare: the running sum is infinity -> take q
    g.label(L_INIT)
    g.s_mov_b64(S_SAVE, EXEC)
    g.s_mov_b64(EXEC, S_ZERO)
    run(f.set_const(E[0], c_lazy))                                  # ZZ = ZZZ = 1 in the form R D^2
    run(f.set_const(E[1], c_lazy))
    mul27(chA, E[2], E[0], E[4], B_TAB, B_TAB)                      # X = q.x, V = q.y in the form R D
    mul27(chB, E[3], E[0], E[5], B_TAB, B_TAB)
    park_put(PARK_X, E[4])
    park_put(PARK_V, E[5])
    g.s_andn2_b64(EXEC, S_SAVE, S_ZERO)
    g.s_cbranch_execz(L_ADV)
    g.long_branch(L_INIT_RET, S_JMP)

    # ------------------------------------------------------------ rare: acc == q -> ((q + S) + q) - S through a salt point
    g.label(L_DETOUR)
    g.s_mov_b64(S_SAVE, EXEC)
    g.s_mov_b64(EXEC, S_DETOUR)
    # salt id = (q.x == salts[0].x) ? 1 : 0 ; q.x is read again from the lane's gather address
    for j in range(NL // 2):
        g.global_load_dwordx2(V(E[2].idx + 2 * j, 2), V_ADDR, OFF, offset=8 * j)
    for j in range(NL // 2):
        g.global_load_dwordx2(V(E[3].idx + 2 * j, 2), V_SALTS, OFF, offset=8 * j)
    g.s_waitcnt(vmcnt=0)
    for w in range(NL):
        g.v_xor_b32(E[2].sub(w), E[2].sub(w), E[3].sub(w))
    run(f.is_zero_mask(chA, E[2], S_T0))
    g.v_cndmask_b32(V_SALT, 0, 1, S_T0)
    g.v_mov_b32(V_PHASE, 1)
    g.s_andn2_b64(EXEC, S_SAVE, S_DETOUR)
    g.s_cbranch_execz(L_ADV)
    g.long_branch(L_DET_RET, S_JMP)
    g.hazard_nops = fix_hazards(g)      # isa.py: the gfx950 VALU -> SGPR -> VALU wait states
    g.loop_labels = (L_LOOP, L_ADV)
    return g


def update_counts(g):
    """What one iteration of the list walk issues on its common path (L_LOOP round to the jump back: the running sum is not
    infinity, no low limb passes a zero filter, so every forward s_cbranch_scc0 is taken), counted from the emitted
    instructions: the figures build.py writes into the build record and DESIGN.md section 4 quotes."""
    at = {i.args[0]: n for n, i in enumerate(g.ins) if i.op == "label"}
    n, end = at[g.loop_labels[0]], None
    total = valu = mads = 0
    while end is None:
        i = g.ins[n]
        n += 1
        if i.op in ("label", "comment"):
            continue
        total += 1
        valu += i.op.startswith("v_")
        mads += i.op == "v_mad_u64_u32"
        if i.op == "s_cbranch_scc0" and at[i.args[0]] > n:
            n = at[i.args[0]]
        elif i.op == "long_branch":
            assert i.args[0] == g.loop_labels[0]
            end = n
    return dict(update_instructions=total, update_valu=valu, update_mads=mads)
