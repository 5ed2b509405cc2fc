"""The generated assembly on the card against asmgen/sim.py, word for word (tests/asm_card.py is the runner).

What the suite knows about the hot kernels at their edges it knows from the simulator, a hand-written model of the mnemonics the
generators emit.  Here the same isa.Prog objects run over the same memory image in the simulator and on the GPU:
* every computing mnemonic of build.programs() in a unit program at operand edges (tests/asm_probes.py), compared three ways: card
  against simulator, and both against a Python-integer definition written next to the probe;
* every class of register dependency the shipped programs leave within 5 wait states, at the closest spacing at which it occurs
  (the table is pinned below), in padded probe programs whose register changes in every lane;
* the field routines of test_asmgen.py, test_asmgen_lazy.py and test_asmgen_ntt.py with their operands at the declared bounds:
  those tests' own functions, run once more with the card runner in place of the simulator call;
* 28 of the 29 shipped programs (all but the microbenchmark) on the images of the simulator tests: the G1 accumulation in both
  forms, g1_reduce, the sixteen G2 round kernels, the NTT passes k = 6, 7, 8.  Nothing was shortened: the longest image (the
  two-pass transform, 34 waves) takes the simulator about 40 s on a slow host.
A program is launched only after the simulator has run that very program over that very image at the device addresses to
s_endpgm (strict mode: no read of an unwritten register, no access outside a buffer, nothing touched in flight).

The CPU half (not marked gpu) runs the simulator side of every comparison against the definitions, and pins what has a probe:
emitted mnemonics = probed ones + the control mnemonics that the whole kernels execute.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ginger-lib_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asm_card                                                   # noqa: E402
import asm_probes                                                 # noqa: E402
import pyref                                                      # noqa: E402
import test_asmgen as TA                                          # noqa: E402
import test_asmgen_acc_persist as TP                              # noqa: E402
import test_asmgen_g2 as TG                                       # noqa: E402
import test_asmgen_lazy as TL                                     # noqa: E402
import test_asmgen_ntt as TN                                      # noqa: E402
import test_asmgen_reduce as TR                                   # noqa: E402
from asm_card import Launch                                       # noqa: E402
from asmgen import build as asm_build                             # noqa: E402

# no probe of their own: executed by the whole kernels (asserted from the simulator's histogram below)
CONTROL = {"s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_execz", "s_cbranch_execnz", "long_branch", "s_nop", "s_waitcnt",
           "s_endpgm"}
_UNITS = {}
_SHIPPED = []


def units():
    if not _UNITS:
        for u in asm_probes.mnemonic_units():
            assert u.name not in _UNITS
            _UNITS[u.name] = u
    return _UNITS


UNIT_NAMES = ["valu_bin", "valu_tern", "shifts", "carries", "compares", "mads", "f64s", "readfirstlane", "bpermute", "lds", "s_loads",
              "salu", "mem_x2", "mem_x4", "mem_a64_x1", "mem_a64_x2", "mem_a64_x4", "atomic_noret", "atomic_ret"]


def shipped():
    if not _SHIPPED:
        _SHIPPED.extend(asm_build.programs())
    return _SHIPPED


G2_CURVES = {"mnt4753_g2": "f2", "mnt6753_g2": "f3", "mnt4753_g1": "f1p4", "mnt6753_g1": "f1p6"}


def whole_programs():
    """the Prog objects the simulator tests run, by the name of the shipped program each one restates: these very objects are
    assembled into this module's code object, so that what the simulator ran is what is launched"""
    out = {}
    for cname, tag in (("mnt4753_g1", "p4"), ("mnt6753_g1", "p6")):
        st = TL._state(cname)
        out["gh_asm_acc_g1_" + tag] = st["blk"]
        out["gh_asm_acc_g1_%s_pw" % tag] = st["pw"]
        out["gh_asm_red_g1_" + tag] = TR._prog(cname)
        for k in (6, 7, 8):
            out["gh_asm_ntt_%s_k%d" % (tag, k)] = TN._prog(pyref.FIELDS[tag].p, k)
    for cname, tag in G2_CURVES.items():
        for fwd in (True, False):
            for r0 in (True, False):
                out["gh_asm_aff_%s_%s_%s" % (tag, "fwd" if fwd else "bwd", "r0" if r0 else "rn")] = TG._prog(cname, fwd, r0)[0]
    return out


# the register-level tests of the field routines: the same functions, operands and integer expectations, run once more over the card
FIELD_CASES = {}
for _tag in ("p4", "p6"):
    for _f in (TA.test_field_routines_in_the_simulator, TA.test_tower_field_routines_in_the_simulator, TL.test_products_with_27_digits,
               TL.test_lazy_differences_are_exact_and_normalised, TL.test_the_update_chain_with_the_accumulator_at_its_bounds,
               TL.test_a_zero_difference_squares_to_p, TL.test_zero_or_p):
        FIELD_CASES["%s[%s]" % (_f.__name__[5:], _tag)] = (_f, (_tag,))
FIELD_CASES["add_and_difference_routines_against_integers"] = (TN.test_add_and_difference_routines_against_integers, ())
_REG = []


def register_programs():
    """-> (recorder, first program of each case): every case run once in the simulator with the recorder in place of
    test_asmgen._execute, which wraps each program the case builds (asm_card.wrap_program)"""
    if not _REG:
        rp, starts = asm_card.RegisterPrograms(), {}
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(TA, "_execute", rp.execute)
            for name, (f, args) in FIELD_CASES.items():
                starts[name] = len(rp.progs)
                f(*args)
        _REG.extend([rp, starts])
    return _REG


def replay(name, runner):
    rp, starts = register_programs()
    rp.runner, rp.at = runner, starts[name]
    try:
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(TA, "_execute", rp.execute)
            f, args = FIELD_CASES[name]
            f(*args)
    finally:
        rp.runner = None


# Every register dependency the shipped programs leave within 5 wait states, by class (writer unit, the SGPR-writing VALU
# mnemonic, register file, how the reader uses the register) with the closest spacing at which the class occurs (independent
# instructions in between; a join by its worst predecessor).  asm_card.dependency_table() computes it; it is pinned here: a
# generator change that creates a class or a closer spacing fails test_dependency_table_is_pinned until a probe runs at it.
DEPENDENCIES = {
    ('LDS return', '-', 'VGPR', 'VALU source'): 1,
    ('SALU', '-', 'EXEC', 'EXEC of LDS'): 0,
    ('SALU', '-', 'EXEC', 'EXEC of VALU'): 0,
    ('SALU', '-', 'EXEC', 'EXEC of VMEM'): 0,
    ('SALU', '-', 'EXEC', 'SALU source'): 0,
    ('SALU', '-', 'SCC', 'SALU source'): 0,
    ('SALU', '-', 'SGPR', 'SALU source'): 0,
    ('SALU', '-', 'SGPR', 'VMEM address'): 0,
    ('SALU', '-', 'SGPR', 'scalar constant'): 0,
    ('SALU', '-', 'SGPR', 'select mask'): 0,
    ('SALU', '-', 'VCC', 'SALU source'): 3,
    ('SMEM return', '-', 'SGPR', 'SALU source'): 1,
    ('VALU', '-', 'VGPR', 'LDS address'): 2,
    ('VALU', '-', 'VGPR', 'LDS store data'): 0,
    ('VALU', '-', 'VGPR', 'VALU source'): 0,
    ('VALU', '-', 'VGPR', 'VMEM address'): 0,
    ('VALU', '-', 'VGPR', 'VMEM store data'): 1,
    ('VALU', '-', 'VGPR', 'readfirstlane source'): 1,
    ('VALU', 'v_add_co_u32', 'VCC', 'carry-in'): 2,
    ('VALU', 'v_cmp', 'SGPR', 'SALU source'): 0,
    ('VALU', 'v_cmp', 'SGPR', 'select mask'): 2,
    ('VALU', 'v_cmp', 'VCC', 'SALU source'): 0,
    ('VALU', 'v_readfirstlane_b32', 'SGPR', 'SALU source'): 1,
    ('VALU', 'v_readfirstlane_b32', 'SGPR', 'scalar constant'): 3,
    ('VALU', 'v_sub_co_u32', 'SGPR', 'carry-in'): 2,
    ('VALU', 'v_subb_co_u32', 'SGPR', 'carry-in'): 2,
    ('VALU', 'v_subb_co_u32', 'SGPR', 'select mask'): 2,
    ('VMEM return', '-', 'VGPR', 'VALU source'): 2,
    ('VMEM return', '-', 'VGPR', 'readfirstlane source'): 1,
}
DEP_IDS = ["%s %s %s to %s at %d" % (k + (v,)) for k, v in sorted(DEPENDENCIES.items())]
_DEPS = {}


def dependency_units():
    if not _DEPS:
        for cls, gap in DEPENDENCIES.items():
            u = asm_probes.dependency_unit(cls, gap)
            assert u.name not in _DEPS and u.name not in units()
            _DEPS[cls] = u
    return _DEPS


def emitted():
    return {i.op for p in shipped() for i in p.ins if i.op not in ("label", "comment")}


# ------------------------------------------------------------------ CPU
def test_every_emitted_mnemonic_has_a_probe():
    """the set comes from build.programs() now, not from a list: a generator that starts to emit a mnemonic fails here until a
    probe covers it"""
    assert sorted(units()) == sorted(UNIT_NAMES)
    probed = set().union(*(u.covers for u in units().values()))
    assert probed | CONTROL == emitted(), (sorted(emitted() - probed - CONTROL), sorted((probed | CONTROL) - emitted()))
    assert not probed & CONTROL - {"s_waitcnt"}


@pytest.mark.parametrize("name", UNIT_NAMES)
def test_unit_program_in_the_simulator_equals_its_definition(name):
    """the simulator half of the three-way comparison, at the addresses a stand-in allocator hands out; every mnemonic the unit
    claims to cover was executed, and the padded program is hazard-free"""
    from asmgen.isa import hazard_scan
    u = units()[name]
    r = asm_card.Runner(asm_card.HostCard())
    assert u.check(r) == []
    assert u.covers <= set(r.hist), sorted(u.covers - set(r.hist))
    assert hazard_scan(u.prog, False)[0] == []
    assert r.card.allocs == []


def test_dependency_table_is_pinned():
    table = asm_card.dependency_table(shipped())
    print("\n".join(asm_card.format_table(table)))
    assert table == DEPENDENCIES, ("new classes or spacings", sorted(set(table.items()) - set(DEPENDENCIES.items())),
                                   "gone", sorted(set(DEPENDENCIES.items()) - set(table.items())))
    # the three rules of isa.fix_hazards are among them, at exactly the spacing the rules ask for
    from asmgen.isa import CARRY_OUT_OPS, READLANE_WAIT, SGPR_WAIT
    valu_sgpr = {k: v for k, v in table.items() if k[0] == "VALU" and k[1] != "-" and k[3] in ("select mask", "carry-in", "scalar constant", "64-bit pair")}
    assert min(valu_sgpr.values()) == SGPR_WAIT
    assert {k[1] for k in valu_sgpr} >= {"v_cmp", "v_readfirstlane_b32"} and {k[1] for k in valu_sgpr} & CARRY_OUT_OPS
    assert table[("VALU", "-", "VGPR", "readfirstlane source")] == READLANE_WAIT


@pytest.mark.parametrize("cls", sorted(DEPENDENCIES), ids=DEP_IDS)
def test_dependency_probe_in_the_simulator(cls):
    """writer, the class's closest spacing of independent instructions, reader: the padded probe holds exactly that spacing (the
    scanner finds the class in it, no closer), and computes its definition in the simulator"""
    u = dependency_units()[cls]
    found = asm_card.scan_dependencies(u.prog)
    assert found.get(cls) == DEPENDENCIES[cls], (found.get(cls), asm_card.format_table(found))
    r = asm_card.Runner(asm_card.HostCard())
    assert u.check(r) == []


def test_the_programs_run_on_the_card_are_the_shipped_ones():
    """all 29 shipped programs but the microbenchmark: instruction for instruction the text build.programs() assembles, under
    the simulator tests' names"""
    by_name = {p.name: p for p in shipped()}
    whole = whole_programs()
    assert sorted(whole) == sorted(n for n in by_name if n != "gh_asm_mb_mulpair") and len(by_name) == 29
    for name, g in whole.items():
        assert g.body_text().replace(g.name, "@") == by_name[name].body_text().replace(name, "@"), name
        assert (g.lds_bytes, g.kernarg_bytes, g.wg_id_y, g.max_v, g.max_s) == tuple(
            getattr(by_name[name], k) for k in ("lds_bytes", "kernarg_bytes", "wg_id_y", "max_v", "max_s")), name


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_field_routines_between_prologue_and_epilogue_in_the_simulator(name):
    """the wrapped programs (registers in through memory, registers and SGPR masks out) pass the tests' own integer checks in the
    simulator, strict mode on: what the card tests launch"""
    replay(name, asm_card.Runner(asm_card.HostCard()))


def test_comparison_sees_one_differing_word():
    a = np.arange(4 * 256, dtype=np.uint32)
    assert asm_card.first_difference("buf", a, a.copy(), 256) is None
    for w in (0, 255 + 64, a.size - 1):
        b = a.copy()
        b[w] ^= 1 << 31
        msg = asm_card.first_difference("buf", a, b, 256)
        assert msg is not None and "1 words" in msg and "word %d " % w in msg
        assert "(plane %d, wave %d, lane %d)" % (w // 256, (w % 256) // 64, w % 64) in msg
    assert asm_card.first_difference("buf", a, a[:-1]) is not None
    # ... and through a unit's own check: one word of the definition changed
    u = asm_probes.valu_bin()
    good = u.expect
    u.expect = lambda inp: [[v ^ (l == 77 and k == 3) for l, v in enumerate(p)] for k, p in enumerate(good(inp))]
    d = u.check(asm_card.Runner(asm_card.HostCard()))
    assert len(d) == 1 and "plane 3, wave 1, lane 13" in d[0]


def test_gate_refuses_what_the_simulator_refuses():
    """a program that reads a register nobody wrote, or leaves its buffers, is never launched: run() raises before it uploads"""
    from asmgen.isa import S, V
    from asmgen.sim import MemFault

    class NoLaunch(asm_card.HostCard):
        def upload(self, *a):
            raise AssertionError("reached the card")
    for bad, exc in ((lambda g: g.v_add_u32(asm_card.O(0), V(200), asm_card.I(0)), RuntimeError),
                     (lambda g: (g.v_mov_b32(asm_card.O(0), asm_card.I(0)), g.v_add_u32(asm_card.V_OFF, 4096, asm_card.V_OFF)), MemFault)):
        u = asm_card.Unit("bad", [], 1, 1, bad, [[0] * 256], lambda inp: [[0] * 256])
        r = asm_card.Runner(NoLaunch(), module=object())
        mem = r.memory()
        with pytest.raises(exc):
            r.run(mem, [u.image(mem)])


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def card(gpu, tmp_path_factory):
    """one code object for this module: every unit program and the shipped programs, assembled once; every allocation freed and the
    module unloaded at teardown"""
    c = asm_card.Card()
    progs = ([u.prog for u in units().values()] + [u.prog for u in dependency_units().values()] + list(whole_programs().values())
             + register_programs()[0].progs)
    co, _ = asm_build.assemble(progs, str(tmp_path_factory.mktemp("asm_card")), "gh_asm_card")
    r = asm_card.Runner(c, c.load(co))
    yield r
    c.close()
    assert c.allocs == []
    print("\nsimulator %.1f s, card (copies, launches, comparison) %.1f s" % (r.sim_seconds, r.card_seconds))


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNIT_NAMES)
def test_mnemonics_on_the_card_equal_the_simulator_and_the_definition(card, name):
    assert units()[name].check(card) == []


@pytest.mark.gpu
@pytest.mark.parametrize("cls", sorted(DEPENDENCIES), ids=DEP_IDS)
def test_dependency_at_its_closest_spacing_on_the_card(card, cls):
    """the register's old and new value differ in every lane: a reader that saw the old one differs from the simulator"""
    assert dependency_units()[cls].check(card) == []


# ------------------------------------------------------------------ the field routines at their bounds
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_field_routines_on_the_card(card, name):
    """every register and every SGPR mask the routine leaves, card against simulator word for word; the simulator's words
    against the integers the simulator tests hold (operands at their declared bounds, both primes)"""
    replay(name, card)


# ------------------------------------------------------------------ the whole kernels on the simulator tests' images
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["block", "persistent"])
@pytest.mark.parametrize("cname", TP.CURVES)
def test_g1_accumulation_on_the_card(card, cname, form):
    """the lists of test_asmgen_lazy._state: the special lists, the 60-entry chain, acc == +-q, the ragged second tile; `out` and
    the tile counter (the 16 bytes behind the task table) word for word, and the simulator's words against the group law"""
    st = TL._state(cname)
    nt = len(st["lists"])
    mem, a_karg = TP._memory(st, nt, mem=card.memory())
    try:
        if form == "block":
            launch = Launch(st["blk"], a_karg, (nt + 255) // 256, 256)
        else:
            launch = Launch(st["pw"], a_karg, 3, 64)                 # two tiles for three waves: one finds the counter spent
        assert card.run(mem, [launch]) == []
        TP._check_law(st, mem.get("out").reshape(nt, 78), nt)
        if form == "persistent":
            assert TP._counter(mem, nt) == 2 + 3
    finally:
        mem.release()


@pytest.mark.gpu
@pytest.mark.parametrize("cname", ["mnt4753_g1", "mnt6753_g1"])
def test_g1_reduce_on_the_card(card, cname, monkeypatch):
    """both images of test_asmgen_reduce.py: out, slabs and flag word for word"""
    run = TR._run
    monkeypatch.setattr(TR, "_run", lambda *a: run(*a, card=card))
    TR.test_lean_level_1_at_L4_in_the_simulator(cname)
    TR.test_lean_level_1_at_L2_with_padding_in_the_simulator(cname)


def _g2_card_runner(card):
    def runner(g, bufs, scalars, waves):
        """test_asmgen_g2.sim_runner at device addresses: waves + 1 waves of work in workgroups of four; the waves that fill the
        last workgroup leave at once like the one beyond the work"""
        mem = card.memory()
        try:
            a = {k: mem.add(k, v, writable=k in TG.WRITABLE) for k, v in bufs.items()}
            karg = np.zeros(22, dtype=np.uint32)
            for j, k in enumerate(TG.ARG_ORDER):
                karg[2 * j], karg[2 * j + 1] = a[k] & 0xFFFFFFFF, a[k] >> 32
            karg[18], karg[19], karg[20] = scalars
            assert card.run(mem, [Launch(g, mem.add("karg", karg), (waves + 1 + 3) // 4, 256)]) == [], g.name
            for k in TG.WRITABLE:
                bufs[k][...] = mem.get(k).reshape(bufs[k].shape)
        finally:
            mem.release()
    return runner


@pytest.mark.gpu
@pytest.mark.parametrize("cname", sorted(G2_CURVES))
def test_g2_round_kernels_on_the_card(card, cname, monkeypatch):
    """the four round kernels of the tower on the inputs of test_asmgen_g2.py (the rounds and the rare cases), every writable
    buffer after every launch"""
    rr = TG._run_round
    monkeypatch.setattr(TG, "_run_round", lambda *a, **k: rr(*a, **dict(k, runner=_g2_card_runner(card))))
    TG.test_g2_round_kernels_in_the_simulator(cname)
    TG.test_g2_round_kernels_list_the_rare_cases(cname)


@pytest.mark.gpu
@pytest.mark.parametrize("k", TN.FIRST_PASS)
def test_ntt_first_pass_on_the_card(card, k):
    args, kw, waves = TN.first_pass_case(k)
    got = TN.run_pass(*args, card=card, **kw)
    C = 1 << (8 - k)
    exp = TN.model_pass(*args, columns=[wv * C + c for wv in waves for c in range(C)], **kw)
    assert all(got[i] == e for i, e in enumerate(exp) if e is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("k,inverse,fac", TN.LATER_PASS)
def test_ntt_later_pass_on_the_card(card, k, inverse, fac):
    args, kw, waves = TN.later_pass_case(k, inverse, fac)
    got = TN.run_pass(*args, card=card, **kw)
    C = 1 << (8 - k)
    exp = TN.model_pass(*args, columns=[wv * C + c for wv in waves for c in range(C)], **kw)
    assert all(got[i] == e for i, e in enumerate(exp) if e is not None)


@pytest.mark.gpu
def test_ntt_two_passes_on_the_card(card, monkeypatch):
    run = TN.run_pass
    monkeypatch.setattr(TN, "run_pass", lambda *a, **k: run(*a, **dict(k, card=card)))
    TN.test_two_passes_make_the_transform()


@pytest.mark.gpu
def test_control_mnemonics_were_executed(card):
    """branches, waits, s_nop and long_branch have no probe: the whole kernels above executed them (this test runs last)"""
    assert CONTROL <= set(card.hist), sorted(CONTROL - set(card.hist))
