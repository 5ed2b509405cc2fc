// msm_schedule.h -- the integer side of the MSM's bucket kernels, free of HIP: which list entries an accumulation task owns and
// where its sum goes (msm_kernels.h 4), and the step schedule and detour state of the bucket reduction's wave program
// (msm_reduce_kernels.h).  The kernels call these functions; tests/test_msm_host.py runs the same text with g++ alone
// (tests/host_shim/msm_host_shim.cpp).
#pragma once
#include <stdint.h>
#include "fp29.h"   // GH_HD

namespace gh {

// ---------------------------------------------------------------- accumulation tasks
// The task list of the bucket accumulation: [0, n_chunks) are the chunks of the heavy buckets order[0 .. n_heavy) (the longest
// tasks, scheduled first; heavy bucket h owns the chunks chunk_start[h] .. chunk_start[h + 1], each `chunk` list entries but
// the last), then one task per bucket order[n_heavy ..].  A task adds the list entries [beg, beg + cnt) into dst: partials + t
// (a chunk) or buckets + g.  AFFIN: task t is bucket g_first + t of the affine rounds' output list, which starts at list_base.
// Ptr: a pointer to the kernel's point type (on the host, in the tests: anything an index can be added to).
template <class Ptr> struct AccTaskSpan {
    uint32_t beg, cnt;
    Ptr dst;
};
GH_HD uint32_t acc_heavy_of_chunk(const uint32_t* chunk_start, uint32_t n_heavy, uint32_t t) {   // largest h with chunk_start[h] <= t
    uint32_t lo = 0, hi = n_heavy;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (chunk_start[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}
template <bool AFFIN, class Ptr>
GH_HD AccTaskSpan<Ptr> acc_task_decode(uint32_t t, const uint32_t* starts, const uint32_t* counts, const uint32_t* order, Ptr buckets,
                                       const uint32_t* chunk_start, uint32_t n_heavy, uint32_t n_chunks, uint32_t chunk, Ptr partials,
                                       uint32_t g_first, uint32_t list_base) {
    uint32_t beg, cnt;
    Ptr dst;
    if constexpr (AFFIN) {
        const uint32_t g = g_first + t;
        beg = starts[g] - list_base; cnt = counts[g];
        dst = buckets + g;
    } else if (t >= n_chunks) {
        const uint32_t g = order[n_heavy + (t - n_chunks)];
        beg = starts[g]; cnt = counts[g];
        dst = buckets + g;
    } else {
        const uint32_t h = acc_heavy_of_chunk(chunk_start, n_heavy, t);
        const uint32_t g = order[h], j = t - chunk_start[h];
        beg = starts[g] + j * chunk;
        cnt = counts[g] - j * chunk;
        if (cnt > chunk) cnt = chunk;
        dst = partials + t;
    }
    return AccTaskSpan<Ptr>{beg, cnt, dst};
}

// ---------------------------------------------------------------- reduction schedule
// The steps of the wave program (msm_reduce_kernels.h has the sums they form).  TPW = 2^LT groups per wave, L items per group.
//   ITEM       run  += item i of the group              WACC       wacc += run
//   TREE_WACC  wacc += wacc of group g + off (g < off)   SCAN       run  += run of group g + off (g + off < TPW)
//   TREE_RUN   run  += run of group g + off (g < off)
// mode 0: (ITEM, WACC) for i = L-1 .. 0 without the last WACC, TREE_WACC, SCAN, TREE_RUN, LT steps each; before the first
// TREE_RUN step (`publish`) group 0's run, the sum of all items, is stored and zeroed, so that the tree sums groups >= 1 only.
// mode 1: ITEM for i = L-1 .. 0, then TREE_RUN.  mode 2: the serial part of mode 0 and nothing else.
enum WaveStepKind { WS_ITEM = 0, WS_WACC = 1, WS_TREE_WACC = 2, WS_SCAN = 3, WS_TREE_RUN = 4 };
struct WaveStep {
    int kind, off, i;
    bool publish;
};
GH_HD int wave_serial_steps(uint32_t mode, int L) { return mode == 1 ? L : 2 * L - 1; }
GH_HD int wave_total_steps(uint32_t mode, int L, int LT) {
    return wave_serial_steps(mode, L) + (mode == 1 ? LT : (mode == 2 ? 0 : 3 * LT));
}
GH_HD WaveStep wave_step(uint32_t mode, int L, int LT, int step) {
    const int NS1 = wave_serial_steps(mode, L), t = step - NS1, half = 1 << (LT - 1);
    if (step < NS1) {
        if (mode == 1) return WaveStep{WS_ITEM, 0, L - 1 - step, false};
        return WaveStep{(step & 1) ? WS_WACC : WS_ITEM, 0, L - 1 - (step >> 1), false};
    }
    if (mode == 1) return WaveStep{WS_TREE_RUN, half >> t, 0, false};
    if (t < LT) return WaveStep{WS_TREE_WACC, half >> t, 0, false};
    if (t < 2 * LT) return WaveStep{WS_SCAN, 1 << (t - LT), 0, false};
    return WaveStep{WS_TREE_RUN, half >> (t - 2 * LT), 0, t == 2 * LT};
}
// Which groups take part in a step, given that group g's item i exists.
GH_HD bool wave_step_active(const WaveStep& s, int g, int TPW, bool has_item) {
    if (s.kind == WS_ITEM) return has_item;
    if (s.kind == WS_WACC) return true;
    return s.kind == WS_SCAN ? g + s.off < TPW : g < s.off;
}

// Where the program stands: `step` of the schedule, and inside it the detour that replaces an addition of equal operands
// p + q in the lanes `mydet` by (p + S) + q - S over the scratch slot: det 1: tmp = p + S, 2: tmp += q, 3: dst = tmp - S.
// S = salts[salt_id], chosen by the kernel so that p + S is no doubling either.  det 0 is the step itself.
struct WaveCursor {
    int step = 0, det = 0, salt_id = 0;
    bool mydet = false;
    GH_HD bool salted() const { return det == 1 || det == 3; }   // the second operand is S (det 1) or -S (det 3)
    GH_HD bool detour_reads_tmp() const { return det >= 2; }
    GH_HD bool detour_writes_tmp() const { return det < 3; }
    // after the addition: same = this lane's operands were equal, any_same = some lane's were
    GH_HD void advance(bool same, bool any_same) {
        if (det == 0) {
            if (any_same) { mydet = same; det = 1; } else step++;
        } else if (det == 3) { det = 0; mydet = false; step++; }
        else det++;
    }
};

}  // namespace gh
