// Host build (g++) of the MSM's HIP-free code -- the plans of msm_plan.h, the window folds of msm_fold.h and the accumulation's
// task decode, msm_schedule.h -- exported for
// ctypes so that tests/test_msm_host.py can check them without a GPU.  Test infrastructure only; not part of the product library.
// Points go in and out as ABI Montgomery limbs (3 x DEG x 12 u64 per projective point), which is the host curve's own form.
// The plans are made with the knobs' defaults (MsmKnobs{}), whatever the environment holds.
#include <string.h>
#include <vector>
#include "../../ginger-lib_amd/csrc/msm_plan.h"
#include "../../ginger-lib_amd/csrc/msm_fold.h"
#include "../../ginger-lib_amd/csrc/msm_schedule.h"

using namespace gh;
using namespace gh_rt;

template <class HC> static std::vector<Proj<HC>> load_points(const uint64_t* pts, int count) {
    std::vector<Proj<HC>> v((size_t)count);
    memcpy(v.data(), pts, (size_t)count * sizeof(Proj<HC>));
    return v;
}
// mode 0: fold_generic; 1: lean_reslot, then fold_generic; 2: fold_merged_generic (a = Wp_all, b = q, d = sets)
template <class HC> static void fold_op(int mode, const uint64_t* pts, int RW, int c, int u, int sw, int a, int b, uint64_t* out) {
    std::vector<Proj<HC>> hw = load_points<HC>(pts, 9 * RW);
    if (mode == 1) lean_reslot<HC>(hw, RW);
    const Proj<HC> r = mode == 2 ? fold_merged_generic<HC>(hw, RW, b, u, sw, a, c) : fold_generic<HC>(hw, RW, c, u, sw, a);
    memcpy(out, &r, sizeof r);
}

extern "C" {
// curve: 0 mnt4753_g1, 1 mnt4753_g2, 2 mnt6753_g1, 3 mnt6753_g2
// modes 0 / 1: a = top_unsigned; mode 2: a = sets, b = q
int t_fold(int curve, int mode, const uint64_t* pts, int RW, int c, int u, int sw, int a, int b, uint64_t* out) {
    switch (curve) {
        case 0: fold_op<HostMnt4G1>(mode, pts, RW, c, u, sw, a, b, out); return 0;
        case 1: fold_op<HostMnt4G2>(mode, pts, RW, c, u, sw, a, b, out); return 0;
        case 2: fold_op<HostMnt6G1>(mode, pts, RW, c, u, sw, a, b, out); return 0;
        case 3: fold_op<HostMnt6G2>(mode, pts, RW, c, u, sw, a, b, out); return 0;
    }
    return -1;
}

int t_auto_window(uint64_t n, int deg, int override_c) { return auto_window((size_t)n, deg, override_c); }
int t_precompute_window(uint64_t n, int deg, int override_c) { return precompute_window((size_t)n, deg, override_c); }
int t_const(int which) {
    const int v[6] = {MSM_REDUCE_L, MSM_MAX_HEAVY_THRESHOLD, MSM_SIZE_BINS, MSM_PART_MAX_BINS, (int)MSM_DUP_CHUNK, AFF_MAX_ROUNDS};
    return v[which];
}

// out[25]: status, merged, c, W, top_unsigned, sets, nb, entries, total, RW, Q, segs_per_window, tpw, sw, L1, L2, lean, lane_buf,
// tree, heavy_thr, heavy_chunk, max_heavy, max_chunks, fold_u, fold_lq  (from heavy_thr on only with status 0)
void t_plan_msm(uint64_t n, int deg, int has_table, int pre_c, int pre_G, int solo, int last, int window_override, int affine_mode,
                int64_t* out) {
    const MsmPlan p = plan_msm((size_t)n, deg, has_table != 0, pre_c, pre_G, solo != 0, last != 0, window_override, affine_mode, MsmKnobs{});
    const int64_t v[25] = {p.status, p.merged, p.c, p.W, p.top_unsigned, p.sets, p.nb, (int64_t)p.entries, (int64_t)p.total, p.RW, p.Q,
                           p.segs_per_window, p.tpw, p.sw, p.L1, p.L2, p.lean, p.lane_buf, p.tree, p.heavy_thr, p.heavy_chunk,
                           (int64_t)p.max_heavy, (int64_t)p.max_chunks, fold_u(p.sw, p.L1), fold_lq(p.Q)};
    memcpy(out, v, sizeof v);
}

// out[5]: tile, bin_shift, n_bins, n_blocks, part
void t_plan_sort(uint64_t entries, uint64_t n, uint64_t total, uint32_t* out) {
    const SortPlan s = plan_sort((size_t)entries, (size_t)n, (size_t)total, MsmKnobs{});
    out[0] = s.tile; out[1] = s.bin_shift; out[2] = s.n_bins; out[3] = s.n_blocks; out[4] = s.part;
}

// out[4]: R, stride, room, K
void t_tree_plan(uint32_t n0, uint64_t total, uint32_t maxc, int deg, int lanes, uint64_t free_b, uint64_t have, uint64_t* out) {
    const MsmKnobs k;
    TreePlan tp(n0, (size_t)total, maxc, deg, 64u / (uint32_t)lanes, 1024, 2048, k);
    out[0] = (uint64_t)tp.R; out[1] = tp.stride;
    out[2] = tp.set_chunks(n0, lanes, (size_t)free_b, (size_t)have, k) ? 1 : 0;
    out[3] = tp.K;
}
// out[6]: first tile, waves, aw, Bq, nA, split
void t_tree_piece(uint32_t n_piece, uint32_t o0, uint32_t tpw, uint32_t max_waves, uint32_t asm_max_waves, int aff_asm, uint64_t* out) {
    const TreePlan tp(1, 1, 1, 1, tpw, max_waves, asm_max_waves, MsmKnobs{});
    const PieceGeom g = tp.piece(n_piece, o0);
    const RoundSplit s = tp.split(n_piece, aff_asm != 0);
    out[0] = g.t0; out[1] = g.waves; out[2] = g.aw; out[3] = g.Bq; out[4] = s.nA; out[5] = s.split;
}

// the accumulation's task decode (msm_schedule.h) with numbers for pointers: bucket g is g, the sum of chunk t is 2^32 + t.
// out[4]: beg, cnt, index, 1 for a chunk sum
void t_acc_task(int affin, uint32_t t, const uint32_t* starts, const uint32_t* counts, const uint32_t* order, const uint32_t* chunk_start,
                uint32_t n_heavy, uint32_t n_chunks, uint32_t chunk, uint32_t g_first, uint32_t list_base, uint32_t* out) {
    const uint64_t buckets = 0, partials = 1ull << 32;
    const AccTaskSpan<uint64_t> k =
        affin ? acc_task_decode<true>(t, starts, counts, order, buckets, chunk_start, n_heavy, n_chunks, chunk, partials, g_first, list_base)
              : acc_task_decode<false>(t, starts, counts, order, buckets, chunk_start, n_heavy, n_chunks, chunk, partials, g_first, list_base);
    out[0] = k.beg; out[1] = k.cnt; out[2] = (uint32_t)k.dst; out[3] = (uint32_t)(k.dst >> 32);
}

// the reduction's step schedule (msm_schedule.h).  out[6]: serial steps, total steps; kind, off, i, publish of `step`
void t_wave_step(uint32_t mode, int L, int LT, int step, int* out) {
    const WaveStep s = wave_step(mode, L, LT, step);
    out[0] = wave_serial_steps(mode, L); out[1] = wave_total_steps(mode, L, LT);
    out[2] = s.kind; out[3] = s.off; out[4] = s.i; out[5] = s.publish ? 1 : 0;
}
int t_wave_step_active(int kind, int off, int g, int tpw, int has_item) {
    return wave_step_active(WaveStep{kind, off, 0, false}, g, tpw, has_item != 0) ? 1 : 0;
}
}
