"""acc_timeline.py -- where the wave-slot time of the G1 bucket accumulation goes: a CPU model and the card's own stamps.

    python3 tools/acc_timeline.py model
        The schedule model of DESIGN.md section 9: list lengths of the 2^20 merged buckets of a 2^20-pair MNT4-753 MSM at
        c = 21 (35 windows of 21 bits, a 17-bit top window), tasks longest first, 256 CUs x 4 SIMDs x 2 wave slots; a wave
        that is alone on its SIMD runs 1.74 x as fast as one of a pair (tools/asm_mb mb_mul_pair).  Block-granular: a
        block of 4 waves (256 tasks) takes a slot pair of its CU only when all four waves of its predecessor have drained.
        Wave-granular: a wave takes the next tile of 64 tasks the moment it is done.  Prints the share of wave-slot time
        that does no work.  No GPU needed.

    GH_ASM_HSACO=<diagnostic code object> GH_ACC_STAMPS=1 [GH_ACC_PERSIST=0|1] [GH_ACC_TILES=K] [GH_ACC_ALT=0|1] python3 tools/acc_timeline.py run [LOG_N]
        One MSM alone, then the last MSM of a batch of 8, through the stamped kernels (code object built with GH_ASM_DEBUG=1:
        `GH_ASM_DEBUG=1 python -m asmgen.build DIR` from ginger-lib_amd/): per wave slot the busy time, the gaps between
        consecutive tiles / blocks on the slot, the time before its first and after its last record.  One process per variant.
"""
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONE = 1.74          # speed of a wave alone on its SIMD relative to one of a pair
CUS, SIMDS = 256, 4
RT_HZ = 100e6        # s_memrealtime: the constant-rate counter


# ------------------------------------------------------------------------------------------------ the model
def list_lengths(rng, log_n=20, c=21, bits=753):
    """entries per merged bucket, descending: full windows spread over 2^(c-1) buckets (a zero digit files nothing), the
    top window's remaining bits over the first of them"""
    n, nb = 1 << log_n, 1 << (c - 1)
    full, top_bits = divmod(bits - 1, c)
    cnt = rng.poisson(full * n * (1 - 1 / (2 * nb + 1)) / nb, nb)
    if top_bits:
        tb = min(1 << top_bits, nb)
        cnt[:tb] += rng.poisson(n / tb, tb)
    return np.sort(cnt)[::-1]


def schedule(cnt, per_unit):
    """makespan in units of one update of a paired wave.  per_unit: waves per scheduling unit (4 = block, 1 = tile).
    A unit's waves go to distinct SIMDs of one CU; a wave's length is its longest list = its first task's."""
    waves = cnt[::64].astype(np.float64)                            # 64 tasks per wave, longest first
    units = [waves[i:i + per_unit] for i in range(0, len(waves), per_unit)]
    nxt = 0
    # per CU: rem[simd][slot] work left (0 = free), unit_of[simd][slot]; a block occupies slot b of each SIMD
    rem = np.zeros((CUS, SIMDS, 2))
    heap = []
    now = np.zeros(CUS)

    def place(cu):
        nonlocal nxt
        placed = False
        if per_unit == 4:
            for b in range(2):
                if nxt < len(units) and not rem[cu, :, b].any():
                    u = units[nxt]; nxt += 1
                    rem[cu, :len(u), b] = u
                    placed = True
        else:
            for sd in range(SIMDS):
                for b in range(2):
                    if nxt < len(units) and rem[cu, sd, b] == 0:
                        rem[cu, sd, b] = units[nxt][0]; nxt += 1
                        placed = True
        return placed

    def next_event(cu):
        r = rem[cu]
        busy = (r > 0).sum(axis=1)
        best = None
        for sd in range(SIMDS):
            if busy[sd]:
                rate = 1.0 if busy[sd] == 2 else LONE
                t = r[sd][r[sd] > 0].min() / rate
                best = t if best is None or t < best else best
        return best

    def advance(cu, dt):
        r = rem[cu]
        for sd in range(SIMDS):
            k = (r[sd] > 0).sum()
            if k:
                r[sd][r[sd] > 0] -= dt * (1.0 if k == 2 else LONE)
                r[sd][r[sd] < 1e-9] = 0

    # fill round-robin over the CUs, one unit at a time, as a dispatcher would
    filled = True
    while filled and nxt < len(units):
        filled = False
        for cu in range(CUS):
            if per_unit == 4:
                for b in range(2):
                    if nxt < len(units) and not rem[cu, :, b].any():
                        u = units[nxt]; nxt += 1
                        rem[cu, :len(u), b] = u
                        filled = True
                        break
            else:
                done = False
                for b in range(2):
                    for sd in range(SIMDS):
                        if nxt < len(units) and rem[cu, sd, b] == 0:
                            rem[cu, sd, b] = units[nxt][0]; nxt += 1
                            filled = done = True
                            break
                    if done:
                        break
    for cu in range(CUS):
        t = next_event(cu)
        if t is not None:
            heapq.heappush(heap, (t, cu))
    end = 0.0
    while heap:
        t, cu = heapq.heappop(heap)
        advance(cu, t - now[cu])
        now[cu] = t
        end = max(end, t)
        place(cu)
        dt = next_event(cu)
        if dt is not None:
            heapq.heappush(heap, (t + dt, cu))
    return end, float(waves.sum())


def model(seeds=(1, 2, 3)):
    print("schedule model: 2^20 pairs, c = 21, %d CUs x %d SIMDs x 2 slots, lone wave %.2f x" % (CUS, SIMDS, LONE))
    for seed in seeds:
        cnt = list_lengths(np.random.default_rng(seed))
        line = "seed %d: %d entries, longest list %d, shortest %d;" % (seed, cnt.sum(), cnt[0], cnt[-1])
        for name, per in (("block", 4), ("wave", 1)):
            span, work = schedule(cnt, per)
            line += "  %s-granular: makespan %.1f updates, empty slot time %.2f %%" % (name, span, 100 * (1 - work / (CUS * SIMDS * 2 * span)))
        print(line)


# ------------------------------------------------------------------------------------------------ the card
def analyse(rec, title, acc_ms):
    rec = rec[(rec[:, 4] != 0) | (rec[:, 5] != 0)]                   # records that were written
    if not len(rec):
        print("%s: no records" % title)
        return
    u64 = lambda lo, hi: rec[:, lo].astype(np.uint64) | (rec[:, hi].astype(np.uint64) << np.uint64(32))
    clk0, rt0, clk1, rt1 = u64(0, 1), u64(2, 3), u64(4, 5), u64(6, 7)
    hw, xcc = rec[:, 8], rec[:, 9] & 0xF
    slot = (xcc.astype(np.int64) << 16) | (hw & 0xFF3F).astype(np.int64)      # XCC | SE, SH, CU | SIMD, wave id (pipe id left out)
    t0 = (rt0 - rt0.min()).astype(np.float64) / RT_HZ * 1e3                     # ms
    t1 = (rt1 - rt0.min()).astype(np.float64) / RT_HZ * 1e3
    span = t1.max()
    mhz = float(np.median((clk1 - clk0).astype(np.float64) / np.maximum((rt1 - rt0).astype(np.float64), 1))) * RT_HZ / 1e6
    order = np.lexsort((t0, slot))
    s_, a_, b_ = slot[order], t0[order], t1[order]
    first = np.r_[True, s_[1:] != s_[:-1]]
    last = np.r_[first[1:], True]
    gaps = (a_[1:] - b_[:-1])[~first[1:]]
    n_slots = int(first.sum())
    busy, head, tail = (b_ - a_).sum(), a_[first].sum(), (span - b_[last]).sum()
    total = n_slots * span
    print("%s: %d records on %d wave slots (%d XCCs), span %.3f ms (event-timed accumulation %.3f ms), shader clock %.0f MHz"
          % (title, len(rec), n_slots, len(np.unique(xcc)), span, acc_ms, mhz))
    print("    slot time: busy %.2f %%, before the first record %.2f %%, between records %.2f %%, after the last %.2f %%"
          % (100 * busy / total, 100 * head / total, 100 * gaps.sum() / total, 100 * tail / total))
    if len(gaps):
        print("    gap between consecutive records on a slot: median %.1f us, mean %.1f us, p99 %.1f us, max %.1f us (%d gaps)"
              % (np.median(gaps) * 1e3, gaps.mean() * 1e3, np.percentile(gaps, 99) * 1e3, gaps.max() * 1e3, len(gaps)))
    dur = b_ - a_
    print("    record length: median %.3f ms, longest %.3f ms; first start %.1f us .. last first-start %.1f us; tail per slot: mean %.3f ms, max %.3f ms"
          % (np.median(dur), dur.max(), a_[first].min() * 1e3, a_[first].max() * 1e3, (span - b_[last]).mean(), (span - b_[last]).max()))


def run(log_n):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pyref
    import support as S
    from __graft_entry__ import _load_pkg
    gl = _load_pkg()
    gl.load_library()
    gl.init()
    curve, n = "mnt4753_g1", 1 << log_n
    C = pyref.CURVES[curve]
    rng = pyref.Rng(1)
    xy, _ = S.bases_array(C, [C.mul(rng.next_u64() | 1, C.G), C.mul(rng.next_u64() | 1, C.G)])
    rb = gl.ResidentBases.chain(curve, xy[0], xy[1], n)
    sc = S.random_scalars_np(n, seed=1000, below=C.order)
    ds = gl.DeviceBuffer(n * 96).upload(sc)
    variant = "block"
    if os.environ.get("GH_ACC_PERSIST", "1") != "0":
        k = int(os.environ.get("GH_ACC_TILES", "1"))
        variant = "persistent, " + ("%d tile%s per wave" % (k, "" if k == 1 else "s") if k else "resident grid")
        if os.environ.get("GH_ACC_ALT", "1") != "0":
            variant += ", alternating streams"
    try:
        c = rb.precompute(0)
        gl.msm_batch_dev([(rb, ds, n)] * 4)                          # buffers of both pipeline slots
        rb.msm_dev(ds, n)
        analyse(gl.acc_stamps(), "[%s] 2^%d pairs, c = %d, one MSM alone" % (variant, log_n, c), gl.msm_last_timing()["accumulate_ms"])
        gl.msm_batch_dev([(rb, ds, n)] * 8)
        analyse(gl.acc_stamps(), "[%s] 2^%d pairs, c = %d, last MSM of a batch of 8" % (variant, log_n, c), gl.msm_batch_timing(7)["accumulate_ms"])
    finally:
        ds.free()
        rb.free()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    else:
        model()
