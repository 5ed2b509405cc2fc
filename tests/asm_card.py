"""asm_card.py -- the card next to the simulator: the same isa.Prog objects over the same memory image, once in asmgen/sim.py and
once on the GPU, compared word for word (tests/test_gpu_asm_sim.py).  Not a test module.

* CardMemory is sim.Memory whose regions sit at device addresses: add() allocates the device buffer first and registers the region
  there, so kernarg words and task tables that embed addresses serve both sides unchanged.
* Runner.run(launches) is the gate: it snapshots the image, simulates every wave of every launch (strict mode, the in-flight
  check, the step limit, every access inside a region) and only when all of them reached s_endpgm uploads the snapshot and
  launches the same programs with the same grid.  A simulator refusal propagates as its exception: nothing is launched.
* unit programs (Unit): a body between the runner's own prologue (lane-indexed loads of the input planes) and epilogue (stores of
  the output planes); the memory probes are variants of that prologue / epilogue, so a unit program has no address arithmetic of
  its own.
* dependency_table(): every register dependency the shipped programs leave within 5 wait states, by class, with the closest
  spacing of each class (CPU only).

Launch ABI, as in the simulator tests: s[0:1] kernarg, s2 workgroup id x (s3 = y where Prog.wg_id_y), v0 work-item id.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ginger-lib_amd"))
from asmgen.isa import EXEC, Ins, Prog, S, V, fix_hazards, roles, unit_of, _wait_states   # noqa: E402
from asmgen.sim import Memory, Wave                               # noqa: E402

vp = ctypes.c_void_p
SIM_STEPS = 20_000_000


# ------------------------------------------------------------------ comparison
def first_difference(name, want, got, lanes=None):
    """None when the arrays agree word for word, else a message naming the first differing word (and, for a buffer of planes
    of `lanes` lanes each, its plane, wave and lane)"""
    want, got = np.asarray(want).reshape(-1), np.asarray(got).reshape(-1)
    if want.shape != got.shape:
        return "%s: %d words against %d" % (name, want.size, got.size)
    d = np.nonzero(want != got)[0]
    if d.size == 0:
        return None
    w = int(d[0])
    where = "word %d" % w
    if lanes:
        where += " (plane %d, wave %d, lane %d)" % (w // lanes, (w % lanes) // 64, w % 64)
    return "%s differs in %d words; first at %s: %08x against %08x" % (name, d.size, where, int(want[w]), int(got[w]))


# ------------------------------------------------------------------ the HIP runtime through ctypes
class Card:
    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        h = self.hip
        h.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        h.hipFree.argtypes = [vp]
        h.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
        h.hipModuleLoadData.argtypes = [ctypes.POINTER(vp), vp]
        h.hipModuleUnload.argtypes = [vp]
        h.hipModuleGetFunction.argtypes = [ctypes.POINTER(vp), vp, ctypes.c_char_p]
        h.hipModuleLaunchKernel.argtypes = [vp] + [ctypes.c_uint] * 7 + [vp, vp, vp]
        self.allocs = []
        self.modules = []

    def chk(self, e, what):
        if e != 0:
            raise RuntimeError("%s failed: hip error %d" % (what, e))

    def malloc(self, nbytes):
        d = vp()
        self.chk(self.hip.hipMalloc(ctypes.byref(d), max(nbytes, 4)), "hipMalloc")
        self.allocs.append(d.value)
        return d.value

    def free(self, addr):
        self.allocs.remove(addr)
        self.chk(self.hip.hipFree(vp(addr)), "hipFree")

    def upload(self, addr, arr):
        self.chk(self.hip.hipMemcpy(vp(addr), arr.ctypes.data_as(vp), arr.nbytes, 1), "hipMemcpy to the device")

    def download(self, addr, arr):
        self.chk(self.hip.hipMemcpy(arr.ctypes.data_as(vp), vp(addr), arr.nbytes, 2), "hipMemcpy from the device")

    def load(self, co_path):
        with open(co_path, "rb") as f:
            blob = f.read()
        m = vp()
        self.chk(self.hip.hipModuleLoadData(ctypes.byref(m), blob), "hipModuleLoadData")
        self.modules.append(m.value)
        return m.value

    def function(self, module, name):
        fn = vp()
        self.chk(self.hip.hipModuleGetFunction(ctypes.byref(fn), vp(module), name.encode()), "hipModuleGetFunction " + name)
        return fn

    def launch(self, fn, grid, threads, karg):
        """grid: (x, y) workgroups of `threads` work-items; karg: the kernarg bytes as a uint32 array"""
        size = ctypes.c_size_t(karg.nbytes)
        extra = (vp * 5)(vp(1), karg.ctypes.data_as(vp), vp(2), ctypes.cast(ctypes.pointer(size), vp), vp(3))
        self.chk(self.hip.hipModuleLaunchKernel(fn, grid[0], grid[1], 1, threads, 1, 1, 0, None, None,
                                                ctypes.cast(extra, vp)), "hipModuleLaunchKernel")
        self.chk(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def close(self):
        for a in list(self.allocs):
            self.free(a)
        for m in self.modules:
            self.hip.hipModuleUnload(vp(m))
        self.modules = []


class HostCard:
    """Stands in for the card where there is none: addresses out of a counter, no launches.  The CPU tests use it to run the
    simulator half of every comparison."""

    def __init__(self):
        self.next = 0x7E0000000000
        self.allocs = []

    def malloc(self, nbytes):
        a = self.next
        self.next += (max(nbytes, 4) + 0xFFF) // 0x1000 * 0x1000 + 0x1000
        self.allocs.append(a)
        return a

    def free(self, addr):
        self.allocs.remove(addr)

    def close(self):
        self.allocs = []


class CardMemory(Memory):
    """sim.Memory with every region at the address of a device allocation made for it"""

    def __init__(self, card):
        Memory.__init__(self)
        self.card = card

    def add(self, name, arr_u32, writable=False, base=None):
        if base is None:
            base = self.card.malloc(np.asarray(arr_u32).size * 4)
        return Memory.add(self, name, arr_u32, writable, base=base)

    def release(self):
        """frees the device buffers; the simulator's words stay readable through get()"""
        for base, _, _, _, _ in self.regions:
            if base in self.card.allocs:
                self.card.free(base)


class Launch:
    """One kernel launch: prog over grid = (x, y) workgroups of `threads` work-items, kernarg = the first prog.kernarg_bytes of
    the region at a_karg"""

    def __init__(self, prog, a_karg, grid, threads, lds_fill=0xDEADBEEF):
        self.prog, self.a_karg, self.threads, self.lds_fill = prog, a_karg, threads, lds_fill
        self.grid = grid if isinstance(grid, tuple) else (grid, 1)
        assert threads in (64, 128, 192, 256) and (self.grid[1] == 1 or prog.wg_id_y)


class Runner:
    def __init__(self, card, module=None):
        self.card, self.module = card, module
        self.hist = {}                       # mnemonic -> executed count over everything simulated
        self.sim_seconds = 0.0
        self.card_seconds = 0.0

    def memory(self):
        return CardMemory(self.card)

    def simulate(self, mem, launches):
        import time
        t0 = time.time()
        for L in launches:
            for wy in range(L.grid[1]):
                for wx in range(L.grid[0]):
                    for wv in range(L.threads // 64):
                        w = Wave(L.prog, mem, lds_words=L.prog.lds_bytes // 4, strict=True)
                        w.S[0], w.S[1], w.S[2] = L.a_karg & 0xFFFFFFFF, L.a_karg >> 32, wx
                        if L.prog.wg_id_y:
                            w.S[3] = wy
                        w.V[0] = np.arange(64, dtype=np.uint32) + 64 * wv
                        w.lds[:] = L.lds_fill
                        w.run(max_steps=SIM_STEPS)               # raises on MemFault, in-flight, unwritten register, step limit
                        for k, n in w.hist.items():
                            self.hist[k] = self.hist.get(k, 0) + n
        self.sim_seconds += time.time() - t0

    def run(self, mem, launches):
        """-> list of differences (empty: the card and the simulator agree on every writable region).  mem holds the
        simulator's result afterwards; the card's words are returned in .card_words[name]."""
        snap = [(base, arr.copy(), name, wr) for base, _, arr, name, wr in mem.regions]
        self.simulate(mem, launches)                             # the gate: an exception here launches nothing
        self.card_words = {}
        if self.module is None:
            return []
        import time
        t0 = time.time()
        for base, arr, _, _ in snap:
            self.card.upload(base, arr)
        for L in launches:
            karg = next(a for b, a, _, _ in snap if b == L.a_karg)
            assert karg.nbytes >= L.prog.kernarg_bytes
            karg = np.ascontiguousarray(karg[:(L.prog.kernarg_bytes + 3) // 4])
            self.card.launch(self.card.function(self.module, L.prog.name), L.grid, L.threads, karg)
        diffs = []
        for base, arr, name, wr in snap:
            if wr:
                got = np.empty_like(arr)
                self.card.download(base, got)
                self.card_words[name] = got
                d = first_difference(name, mem.get(name), got)
                if d:
                    diffs.append(d)
        self.card_seconds += time.time() - t0
        return diffs


# ------------------------------------------------------------------ unit programs
IN0, OUT0 = 10, 60            # first input / output VGPR
S_IN, S_OUT = S(4, 2), S(6, 2)
V_OFF, V_ADR = V(1), V(2)


def I(k, n=1):
    return V(IN0 + k, n)


def O(k, n=1):
    return V(OUT0 + k, n)


class Unit:
    """body(g) between the prologue and the epilogue.  inputs: nin planes of `lanes` words (lane = workgroup * threads + v0);
    expect(inputs) -> nout planes of Python integers: the plain definition of what the body computes.
    load / store: dwords per lane and memory instruction (1, 2, 4: the widths in use); addr64: a 64-bit VGPR address instead of
    SGPR base + VGPR offset; atomic: None, or (returning?) -- the epilogue then adds plane 0 into the output instead of storing."""

    def __init__(self, name, covers, nin, nout, body, inputs, expect, grid=1, threads=256, load=1, store=1, addr64=False,
                 atomic=None, lds_bytes=0, out_init=0, extra_out=0):
        self.name, self.covers, self.nin, self.nout = name, set(covers), nin, nout
        self.grid, self.threads, self.lanes = grid, threads, grid * threads
        self.inputs, self.expect, self.atomic, self.out_init = inputs, expect, atomic, out_init
        self.extra_out = extra_out                               # planes behind the epilogue's that the body stores itself
        assert len(inputs) == nin and all(len(p) == self.lanes for p in inputs)
        assert nin % load == 0 and nout % store == 0
        g = self.prog = Prog("gh_unit_" + name)
        g.lds_bytes = lds_bytes
        g.add_arg(8, "ptr")
        g.add_arg(8, "ptr")
        L = self.lanes
        g.s_load_dwordx4(S(4, 4), S(0, 2), 0)
        g.s_lshl_b32(S(8), S(2), threads.bit_length() - 1 + 2)
        g.v_lshl_add_u32(V_OFF, V(0), 2, S(8))                   # byte offset of this lane in a plane
        g.s_waitcnt(lgkmcnt=0)
        # input planes: `load` consecutive planes are interleaved per lane in memory so that one wide load brings them
        for k in range(0, nin, load):
            self._address(g, k * L * 4, load, S_IN, addr64)
            op = getattr(g, "global_load_dword" + ("" if load == 1 else "x%d" % load))
            if addr64:
                op(I(k, load), V(4, 2), "off")
            else:
                op(I(k, load), V_ADR, S_IN)
        if nin:
            g.s_waitcnt(vmcnt=0)
        body(g)
        for k in range(0, nout, store):
            self._address(g, k * L * 4, store, S_OUT, addr64)
            if atomic is not None:
                if atomic:
                    g.global_atomic_add(O(nout + k), V_ADR, O(k), S_OUT, sc0=True)
                else:
                    g.global_atomic_add(V_ADR, O(k), S_OUT)
                continue
            op = getattr(g, "global_store_dword" + ("" if store == 1 else "x%d" % store))
            if addr64:
                op(V(4, 2), O(k, store), "off")
            else:
                op(V_ADR, O(k, store), S_OUT)
        if atomic:                                               # the values before the add: a second set of planes
            g.s_waitcnt(vmcnt=0)
            for k in range(nout):
                g.v_add_u32(V_ADR, (nout + k) * L * 4, V_OFF)
                g.global_store_dword(V_ADR, O(nout + k), S_OUT)
        g.s_endpgm()
        fix_hazards(g)
        self.load, self.store = load, store

    @staticmethod
    def _address(g, plane_bytes, width, s_base, addr64):
        if width == 1:
            g.v_add_u32(V_ADR, plane_bytes, V_OFF)
        else:
            g.v_lshlrev_b32(V_ADR, width.bit_length() - 1, V_OFF)
            g.v_add_u32(V_ADR, plane_bytes, V_ADR)
        if addr64:
            g.v_mov_b32(V(3), 0)
            g.v_mov_b32(V(4), s_base.lo())
            g.v_mov_b32(V(5), s_base.hi())
            g.v_lshl_add_u64(V(4, 2), V(2, 2), 0, V(4, 2))

    # ---- the image
    def _pack(self, planes, width):
        """planes -> words as they lie in memory: `width` consecutive planes interleaved per lane"""
        a = np.array([[x & 0xFFFFFFFF for x in p] for p in planes], dtype=np.uint64).astype(np.uint32).reshape(-1, width, self.lanes)
        return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1)

    def _unpack(self, words, nplanes, width):
        a = np.asarray(words).reshape(nplanes // width, self.lanes, width).transpose(0, 2, 1)
        return a.reshape(nplanes, self.lanes)

    def image(self, mem):
        a_in = mem.add(self.name + ".in", self._pack(self.inputs, self.load) if self.nin else np.zeros(1, dtype=np.uint32))
        nplanes = self.nout * (2 if self.atomic else 1) + self.extra_out
        out = np.full(nplanes * self.lanes, self.out_init, dtype=np.uint32)
        a_out = mem.add(self.name + ".out", out, writable=True)
        karg = np.array([a_in & 0xFFFFFFFF, a_in >> 32, a_out & 0xFFFFFFFF, a_out >> 32], dtype=np.uint32)
        return Launch(self.prog, mem.add(self.name + ".karg", karg), self.grid, self.threads)

    def planes(self, words):
        """output words -> planes (the returned old values of an atomic behind the sums)"""
        n = self.nout
        if self.atomic is None:
            return self._unpack(words, n + self.extra_out, self.store)
        if not self.atomic:
            return self._unpack(words, n, 1)
        return np.concatenate([self._unpack(words[:n * self.lanes], n, 1), self._unpack(words[n * self.lanes:], n, 1)])

    def check(self, runner):
        """card against simulator, and both against the plain definition -> list of differences"""
        mem = runner.memory()
        try:
            diffs = runner.run(mem, [self.image(mem)])
            want = np.array([[int(x) & 0xFFFFFFFF for x in p] for p in self.expect(self.inputs)], dtype=np.uint64).astype(np.uint32)
            d = first_difference(self.name + ": simulator against the definition", want, self.planes(mem.get(self.name + ".out")), self.lanes)
            if d:
                diffs.append(d)
            if runner.card_words:
                d = first_difference(self.name + ": card against the definition", want,
                                     self.planes(runner.card_words[self.name + ".out"]), self.lanes)
                if d:
                    diffs.append(d)
            return diffs
        finally:
            mem.release()


# ------------------------------------------------------------------ the dependency scanner
WINDOW = 5
FILE_OF = {"v": "VGPR", "a": "VGPR", "s": "SGPR", "vcc": "VCC", "exec": "EXEC", "scc": "SCC"}
WRITER_OF = {"VALU": "VALU", "SALU": "SALU", "VMEM": "VMEM return", "LDS": "LDS return", "SMEM": "SMEM return"}
BRANCHES = ("s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz",
            "s_cbranch_execnz", "long_branch")


def _keys(r):
    if r.kind == "scc":
        return (("SCC", 0),)
    if r.kind == "exec":
        return (("EXEC", 0),)
    if r.kind == "vcc":
        return (("VCC", 0),)
    f = FILE_OF[r.kind]
    base = r.idx + (256 if r.kind == "a" else 0)
    return tuple((f, base + j) for j in range(r.n))


def scan_dependencies(prog, table=None, passes=3):
    """every (writer unit, writer mnemonic class, register file, reader use) with the reader at most WINDOW wait states behind the
    writer -> the closest spacing (independent wait states in between).  A label is a join: the state behind it is the worst
    (closest) of the fall-through and of every branch that names it, the branch itself being one wait state -- the rule of
    isa.hazard_scan, over the real predecessors."""
    table = {} if table is None else table
    at_branch = {}                      # label -> {register key: (distance of the write at the target, writer class)}
    for _ in range(passes):
        state = {}                      # register key -> (position of the write, writer class)
        pos = 0
        reachable = True
        changed = False
        for i in prog.ins:
            if i.op == "comment":
                continue
            if i.op == "label":
                inc = at_branch.get(i.args[0], {})
                if not reachable:
                    state = {}
                for k, (dist, cls) in inc.items():
                    cur = state.get(k)
                    if cur is None or pos - cur[0] > dist:
                        state[k] = (pos - dist, cls)
                reachable = True
                continue
            dests, srcs = roles(i)
            u = unit_of(i)
            for r, role in srcs:
                for k in _keys(r):
                    w = state.get(k)
                    if w is None:
                        continue
                    gap = pos - w[0] - 1
                    if 0 <= gap < WINDOW:
                        use = {"src": "%s source" % ("VALU" if u == "VALU" else "SALU"), "scc": "SALU source",
                               "mask": "select mask", "carry": "carry-in", "const": "scalar constant", "pair": "64-bit pair",
                               "addr": "%s address" % u, "data": "%s store data" % u, "rfl": "readfirstlane source",
                               "exec": "EXEC of %s" % u}[role]
                        cls = (w[1][0], w[1][1], k[0], use)
                        if gap < table.get(cls, WINDOW):
                            table[cls] = gap
            wu = WRITER_OF[unit_of(i)]
            for r in dests:
                wc = "-"                                         # a VALU instruction that writes an SGPR: by mnemonic (every v_cmp_* as one)
                if unit_of(i) == "VALU" and r.kind in ("s", "vcc"):
                    wc = "v_cmp" if i.op.startswith("v_cmp_") else i.op
                for k in _keys(r):
                    state[k] = (pos, (wu, wc))
            pos += _wait_states(i)
            if i.op in BRANCHES:
                tgt = i.args[0]
                inc = at_branch.setdefault(tgt, {})
                for k, (p0, cls) in state.items():
                    dist = pos - p0                      # wait states from the write to the first instruction at the target
                    if dist - 1 < WINDOW and (k not in inc or inc[k][0] > dist):
                        inc[k] = (dist, cls)
                        changed = True
                if i.op in ("s_branch", "long_branch"):
                    reachable = False
            elif i.op == "s_endpgm":
                reachable = False
        if not changed:
            break
    return table


def dependency_table(progs):
    table = {}
    for p in progs:
        scan_dependencies(p, table)
    return table


def format_table(table):
    return ["%-12s %-19s %-5s -> %-22s %d" % (k + (v,)) for k, v in sorted(table.items())]


# ------------------------------------------------------------------ register-level programs (the field routines' tests)
R0 = 4                        # V(R0 ..) and the SGPRs the body writes travel through memory; V(0 .. 3), s[0:7] are the wrapper's


class Registers:
    """what a register-level test sees of a run: the VGPRs, the SGPRs the body wrote, the executed-mnemonic histogram of the body"""

    def __init__(self):
        self.V = np.zeros((512, 64), dtype=np.uint32)
        self.S = [0] * 128
        self.hist = {}

    def rd_smask(self, o):
        return self.S[o.idx] | (self.S[o.idx + 1] << 32)


def wrap_program(name, g):
    """g: a one-wave program over registers that a test fills by hand (ends in s_endpgm, touches no memory) -> the same body between
    a prologue that loads V(R0 .. 255) and an epilogue that stores them and every SGPR the body wrote; padded by fix_hazards"""
    own = ".L%s_" % g.name                                         # the body's labels, under the wrapper's name: one code object holds many
    body = [Ins(i.op, tuple(".L%s_%s" % (name, a[len(own):]) if isinstance(a, str) and a.startswith(own) else a for a in i.args),
                i.mods, i.comment) for i in g.ins if i.op != "s_endpgm"]
    sgprs = set()
    for i in body:
        dests, srcs = roles(i)
        for r in list(dests) + [r for r, _ in srcs]:
            if r.kind in ("v", "a"):
                assert r.kind == "v" and r.idx >= R0, "%s uses a register of the wrapper" % i.text().strip()
            elif r.kind == "s":
                assert r.idx >= 8, "%s uses a register of the wrapper" % i.text().strip()
        assert unit_of(i) in ("VALU", "SALU") or i.op in ("ds_bpermute_b32", "s_waitcnt"), i.op
        sgprs.update(r.idx + j for r in dests if r.kind == "s" for j in range(r.n))
    w = Prog(name)
    w.add_arg(8, "ptr")
    w.add_arg(8, "ptr")
    w.s_load_dwordx4(S(4, 4), S(0, 2), 0)
    w.v_lshlrev_b32(V_OFF, 2, V(0))
    w.s_waitcnt(lgkmcnt=0)
    for r in range(R0, 256):
        w.v_add_u32(V_ADR, (r - R0) * 256, V_OFF)
        w.global_load_dword(V(r), V_ADR, S_IN)
    w.s_waitcnt(vmcnt=0)
    w.ins += body
    w.max_v, w.max_s, w._uniq = 256, max(g.max_s, 8), g._uniq
    w.s_mov_b64(EXEC, -1)
    for r in range(R0, 256):
        w.v_add_u32(V_ADR, (r - R0) * 256, V_OFF)
        w.global_store_dword(V_ADR, V(r), S_OUT)
    w.sgprs = sorted(sgprs)
    for k, r in enumerate(w.sgprs):
        w.v_mov_b32(V(3), S(r))
        w.v_add_u32(V_ADR, (256 - R0 + k) * 256, V_OFF)
        w.global_store_dword(V_ADR, V(3), S_OUT)
    w.s_endpgm()
    fix_hazards(w)
    return w


class RegisterPrograms:
    """Records the register-level programs the simulator tests build (record=True: each is wrapped and kept, in order), then
    replays the same tests over the card: execute(g, fill) stands in for the tests' own `Wave(g, Memory()); fill(w); w.run()`."""

    def __init__(self):
        self.progs = []
        self.runner = None
        self.at = 0

    def execute(self, g, fill):
        if self.runner is None:                                   # recording: wrap, keep, and let the test go on in the simulator
            self.progs.append(wrap_program("gh_reg_%d" % len(self.progs), g))
            w = Wave(g, Memory())
            fill(w)
            w.run()
            return w
        wp = self.progs[self.at]
        self.at += 1
        regs = Registers()
        fill(regs)
        mem = self.runner.memory()
        try:
            a_in = mem.add("regs.in", regs.V[R0:256])
            nrows = 256 - R0 + len(wp.sgprs)
            a_out = mem.add("regs.out", np.full(nrows * 64, 0xDEADBEEF, dtype=np.uint32), writable=True)
            karg = np.array([a_in & 0xFFFFFFFF, a_in >> 32, a_out & 0xFFFFFFFF, a_out >> 32], dtype=np.uint32)
            before = dict(self.runner.hist)
            diffs = self.runner.run(mem, [Launch(wp, mem.add("regs.karg", karg), 1, 64)])
            assert diffs == [], (wp.name, diffs)
            out = mem.get("regs.out").reshape(nrows, 64)
            regs.V[R0:256] = out[:256 - R0]
            for k, r in enumerate(wp.sgprs):
                assert len(set(int(x) for x in out[256 - R0 + k])) == 1
                regs.S[r] = int(out[256 - R0 + k][0])
            regs.hist = {k: n - before.get(k, 0) for k, n in self.runner.hist.items() if n != before.get(k, 0)}
            return regs
        finally:
            mem.release()
