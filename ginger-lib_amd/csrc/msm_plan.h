// msm_plan.h -- the integer arithmetic of the MSM's launch sequence, free of HIP: the environment knobs, the window choosers,
// and what one MSM / its bucket sort / its affine rounds look like as plain values (MsmPlan, SortPlan, TreePlan).  msm_impl.h
// turns these into buffers and launches; tests/test_msm_host.py checks them with g++ alone (tests/host_shim/msm_host_shim.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace gh {

// ---- constants the plans and the kernels share (msm_kernels.h, aff_kernels.h)
constexpr int MSM_REDUCE_L = 16;               // buckets folded serially per lane in reduce level 1
constexpr int MSM_MAX_HEAVY_THRESHOLD = 1024;  // upper bound of the run-time heavy threshold
constexpr int MSM_SIZE_BINS = MSM_MAX_HEAVY_THRESHOLD + 2;
constexpr int MSM_PART_MAX_BINS = 2048;        // (1024 unless the buckets need more: plan_sort)
constexpr uint32_t MSM_DUP_CHUNK = 4096;       // members of a group of equal bases summed per block (msm_merge_scalars_kernel)
constexpr int AFF_MAX_ROUNDS = 26;

}  // namespace gh

namespace gh_rt {
using namespace gh;

// an integer / real knob from the environment: dflt when unset, atoi / atof of the value otherwise
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
inline double env_double(const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; }

// ---- environment knobs of the MSM host code (DESIGN.md, table of switches).  Read ONCE per process, at the first MSM or table
// build (msm_knobs()): a test that wants another value starts a child process.  Two more are read on every call, where they
// are used (msm_key.h precompute_bases): GH_TABLE_ROWS and GH_TEST_TABLE_NOMEM.
struct MsmKnobs {
    int dedup = 1;                  // GH_DEDUP=0: do not add up the scalars of a key's equal bases (A/B)
    int reduce_l = 0;               // GH_REDUCE_L: segment length of the reduction programs (a power of two in 4..128; 0 = chosen)
    int reduce_lean = -1;           // GH_REDUCE_LEAN=0 / 1: segment form / lane-level form of a G1 reduction everywhere (-1 = chosen)
    int reduce_waves = 0;           // GH_REDUCE_WAVES=1 / 2: the 512- / 256-register build of the G1 reduction program (0 = by `solo`)
    int reduce_asm = 1;             // GH_REDUCE_ASM=0: lean level 1 of a G1 reduction on the C++ kernel instead of the generated one (A/B)
    bool reduce_debug = false;      // GH_REDUCE_DEBUG (set): per lean level 1, programs run / computed again (stderr; synchronises)
    int affine = -1;                // GH_AFFINE=0 / 1 / 2: overrides gh_msm_set_affine (-1 = unset)
    int agg_iters = 12;             // GH_AGG_ITERS: keys a wave folds into one atomic in the small-input histogram / scatter
    int sort = 0;                   // GH_SORT=atomic (1) / part (2): bucket lists by device-scope atomics / by the LDS counting sort
    int aff_rounds = 0;             // GH_AFF_ROUNDS: depth of the affine rounds (0 = chosen)
    int aff_bmin = 8;               // GH_AFF_BMIN: elements per lane group and inversion, at least
    int aff_finish_max = 64;        // GH_AFF_FINISH_MAX: no bucket is left to the projective finish with more points than this
    bool aff_leftover_set = false;  // GH_AFF_LEFTOVER: points left per bucket on average for the projective finish;
    double aff_leftover = 0;        //   unset: by the degree of the curve's field (leftover())
    double aff_scratch_gb = 64.0;   // GH_AFF_SCRATCH_GB: scratch budget of the rounds per buffer slot (chunks of buckets)
    int aff_split = 1;              // GH_AFF_SPLIT=0: affine rounds in one piece instead of two halves on two streams
    int aff_split_b = 32;           // GH_AFF_SPLIT_B: the smallest batch per lane group at which a round is split
    bool aff_debug = false;         // GH_AFF_DEBUG (set): per affine round, exceptions listed / round redone (stderr; synchronises)
    // launch form of the assembly G1 accumulation (DESIGN.md section 9 "Launch form of the accumulation", profiles/acc_persist_ab.json)
    int acc_persist = 1;            // GH_ACC_PERSIST=0: blocks of 256 tasks instead of one-wave workgroups that draw tiles of 64 tasks (A/B)
    int acc_waves = 0;              // GH_ACC_WAVES=N: grid of the persistent form (0 = by the budget, or 8 per CU without one); for tests and sweeps
    int acc_tiles = 1;              // GH_ACC_TILES=K: a persistent wave ends after K tiles, the grid is tiles / K (0 = no limit: a resident grid,
                                    //   which keeps the sort and the reduction of the neighbouring MSMs of a batch off the card: +4.4 ms per MSM)
    int acc_alt = 1;                // GH_ACC_ALT=0: the persistent G1 accumulations of a batch all on one stream instead of two in turn (A/B)

    // (round 3, profiles/r03_g2_knobs.txt: on the towers the projective finish costs 11 tower products per point against the rounds' 6,
    //  so fewer points are left to it: Fq3 1.5 (MNT6 G2 2^19: 5.75 -> 5.95 M/s together with the one-chunk scratch budget), Fq2 2.5)
    double leftover(int deg) const { return aff_leftover_set ? aff_leftover : (deg == 3 ? 1.5 : (deg == 2 ? 2.5 : 4.5)); }

    static MsmKnobs from_env() {
        MsmKnobs k;
        k.dedup = env_int("GH_DEDUP", k.dedup);
        k.reduce_l = env_int("GH_REDUCE_L", k.reduce_l);
        k.reduce_lean = env_int("GH_REDUCE_LEAN", k.reduce_lean);
        k.reduce_waves = env_int("GH_REDUCE_WAVES", k.reduce_waves);
        k.reduce_asm = env_int("GH_REDUCE_ASM", k.reduce_asm);
        k.reduce_debug = getenv("GH_REDUCE_DEBUG") != nullptr;
        k.affine = env_int("GH_AFFINE", k.affine);
        const int agg = env_int("GH_AGG_ITERS", -1);
        if (agg >= 0) k.agg_iters = agg;
        const char* sort = getenv("GH_SORT");
        k.sort = sort && !strcmp(sort, "atomic") ? 1 : (sort && !strcmp(sort, "part") ? 2 : 0);
        k.aff_rounds = env_int("GH_AFF_ROUNDS", k.aff_rounds);
        k.aff_bmin = env_int("GH_AFF_BMIN", k.aff_bmin);
        k.aff_finish_max = env_int("GH_AFF_FINISH_MAX", k.aff_finish_max);
        k.aff_leftover_set = getenv("GH_AFF_LEFTOVER") != nullptr;
        k.aff_leftover = env_double("GH_AFF_LEFTOVER", 0);
        k.aff_scratch_gb = env_double("GH_AFF_SCRATCH_GB", k.aff_scratch_gb);
        k.aff_split = env_int("GH_AFF_SPLIT", k.aff_split);
        k.aff_split_b = env_int("GH_AFF_SPLIT_B", k.aff_split_b);
        k.aff_debug = getenv("GH_AFF_DEBUG") != nullptr;
        k.acc_persist = env_int("GH_ACC_PERSIST", k.acc_persist);
        k.acc_waves = env_int("GH_ACC_WAVES", k.acc_waves);
        k.acc_tiles = env_int("GH_ACC_TILES", k.acc_tiles);
        k.acc_alt = env_int("GH_ACC_ALT", k.acc_alt);
        return k;
    }
};
inline const MsmKnobs& msm_knobs() {
    static const MsmKnobs k = MsmKnobs::from_env();
    return k;
}

// ---- window choice.  override_c > 0 (gh_msm_set_window) wins in both.
inline int floor_log2(size_t n) {
    int lg = 0;
    while (((size_t)1 << (lg + 1)) <= n) lg++;
    return lg;
}

// Without a table.  Measured on MI355X (profiles/r01_window_sweep.txt): besides the usual trade of
// accumulate work (n * ceil(754/c) additions) against bucket-reduction work (2^(c-1) buckets per
// window), what matters is how full the TOP window is -- c = 13 (58 * 13 = 754), 18 (42 * 18 = 756),
// 19 and 21 leave no sparsely populated top window whose few buckets become over-long.
inline int auto_window(size_t n, int deg, int override_c) {
    if (override_c > 0) return override_c;
    const int lg = floor_log2(n);
    if (deg > 1) {   // G2: the host fold and the reduction weigh more per window -> fewer, larger windows
        int c = lg - 4;
        return c < 4 ? 4 : (c > 20 ? 20 : c);
    }
    if (lg >= 23) return 19;
    if (lg >= 21) return 18;
    if (lg >= 19) return 16;
    if (lg >= 15) return 13;
    int c = lg - 3;
    return c < 4 ? 4 : c;
}

// With a precomputed shift table (msm_key.h precompute_bases).
inline int precompute_window(size_t n, int deg, int override_c) {
    if (override_c > 0) return override_c;
    const int lg = floor_log2(n);
    // Measured on MI355X (profiles/r01_precompute_sweep.txt).  Only window sizes whose top window
    // is well filled are used: 752 mod c = 14 (c = 18), 12 (20), 17 (21), 16 (23).  With 752 mod c = 4
    // (c = 17, 22) the top window's n digits land on 16 counters and the bucket sort's atomics
    // serialise (sort time x 2.5); c = 16 divides 752 and would add a carry-only window.
    // G2: with the affine rounds the accumulation costs 6 tower products per addition instead of 11, while the bucket
    // reduction (2^(c-1) buckets, projective) keeps its price: c = 21 at 2^20 pairs left 26 ms of reduction next to 80 ms
    // of accumulation; c = 19 has a quarter of the buckets for 11 % more additions.
    // (round 3, profiles/r03_shard_sweep.txt: MNT6 G2 2^19 c = 19 5.77 M/s vs c = 18 5.63; 2^22 c = 21 7.26 vs c = 19 6.74 -- at 4 M pairs the
    //  accumulation is long enough to carry the 2^20-bucket reduction)
    if (deg > 1) return lg <= 18 ? 18 : (lg <= 21 ? 19 : 21);
    if (lg <= 17) return 18;
    if (lg == 18) return 20;
    if (lg <= 22) return 21;
    return 23;
}

// ---- the host fold's exponents (msm_fold.h): 2^u = slots per level-1 program, 2^lq = slots per pseudo-window
inline int fold_u(int sw, int L1) {
    int u = sw;
    while ((1 << (u - sw)) < L1) u++;
    return u;
}
inline int fold_lq(uint32_t Q) {
    int lq = 0;
    while ((1u << lq) < Q) lq++;            // RW > sets only with Q = 2^15; for one pseudo-window per set the term is empty
    return lq;
}

// ---- one MSM
enum MsmPlanStatus { MSM_PLAN_OK = 0, MSM_PLAN_TOO_LARGE = 1 };   // too large: W n or the bucket count does not fit 31-bit list entries

struct MsmPlan {
    int status = MSM_PLAN_OK;
    bool merged = false;            // the key carries a precomputed shift table -> all windows of a set share one bucket set
    int c = 0, W = 0, top_unsigned = 0;
    int sets = 1;                   // bucket sets (window w -> set w % sets, table row w / sets): 1 with a full table, pre_G with a
                                    // partial one, W without
    uint32_t nb = 0;                // slots of a bucket set; also the stride of a set in the bucket array
    size_t entries = 0, total = 0;  // list entries W n; buckets sets * nb
    // what the reduction sees: RW windows of Q slots (merged: every set is cut into pseudo-windows of Q slots); RW * Q == total
    int RW = 0;
    uint32_t Q = 0, segs_per_window = 0;
    int tpw = 64, sw = 6;           // items per wave of the reduction programs (G2 lane groups: 32 / 16) and their log2
    int L1 = 0, L2 = 0;             // items per lane (group) of a level-1 / level-2 program
    bool lean = false;              // bucket reduction in its lane-level form (launch_reduce)
    bool lane_buf = false;          // the slot holds the lean form's buffer (also for a batch's last MSM, which does not use it)
    bool tree = false;              // bucket sums by affine rounds (aff_kernels.h)
    uint32_t heavy_thr = 0, heavy_chunk = 0;
    size_t max_heavy = 0, max_chunks = 0;
};

// n > 0 pairs on a curve whose base field has degree `deg`; has_table / pre_c / pre_G: the key's shift table; solo: a batch of
// one; last: the last MSM of its batch; affine_mode: gh_msm_set_affine.
inline MsmPlan plan_msm(size_t n, int deg, bool has_table, int pre_c, int pre_G, bool solo, bool last, int window_override,
                        int affine_mode, const MsmKnobs& k) {
    MsmPlan p;
    p.merged = has_table && (window_override == 0 || window_override == pre_c);
    p.c = p.merged ? pre_c : auto_window(n, deg, window_override);
    const int c = p.c;
    // after sign folding the scalar magnitudes are below 2^752 (msm_kernels.h, digits kernel)
    p.W = 752 / c + 1;
    p.top_unsigned = (!p.merged && 752 % c == 0 && p.W >= 2) ? 1 : 0;
    p.nb = (1u << (c - 1)) + (p.merged ? 0u : 1u);   // merged: slot = |digit| - 1 (msm_kernels.h, digits kernel), weight slot + 1
    const uint32_t q = 15;
    p.Q = p.merged && p.nb > (1u << q) ? (1u << q) : p.nb;     // nb is a power of two when merged: Q divides it
    p.sets = p.merged ? pre_G : p.W;
    p.RW = p.merged ? p.sets * (int)(p.nb / p.Q) : p.W;
    p.entries = (size_t)p.W * n;
    p.total = (size_t)p.sets * p.nb;
    // items per lane, level 1 (power of two).  The wave programs are latency chains (2 L1 + 17 steps,
    // then 2 L2 + 17): as long as the launch stays within one wave per SIMD (1024 on MI355X) a shorter
    // L1 only shortens the chain; beyond that the steps of co-resident waves add up again
    // (measured at 2^20 + 1 buckets: L1 = 16 -> 6.2 ms, 8 -> 6.8, 4 -> 8.2, 32 -> 7.9 -- the one bucket beyond the power of two
    //  added a 1025th / 2049th / 4097th wave program, which ran beside or after another one on its SIMD and doubled the
    //  launch; with the merged set at exactly 2^(c-1) slots level 1 takes 4.3 ms (L1 = 16), level 2 1.1 ms).
    p.tpw = deg == 2 ? 32 : (deg == 3 ? 16 : 64);   // lane pairs / lane triples (48 lanes busy) on G2 (msm_reduce_kernels.h)
    p.sw = p.tpw == 64 ? 6 : (p.tpw == 32 ? 5 : 4);
    auto programs = [&](int l1) { return (size_t)p.RW * ((p.Q + (uint32_t)p.tpw * l1 - 1) / ((uint32_t)p.tpw * l1)); };
    p.L1 = MSM_REDUCE_L;
    while (p.L1 > 4 && programs(p.L1 / 2) <= 1024) p.L1 >>= 1;
    // more programs than SIMDs even at L1 = 16 (the per-window path: 48 windows x 32 segments at 2^20 pairs; every path at
    // 2^24): twice the segment length halves the programs -- 768 instead of 1536 at 2^20, so that no SIMD carries two -- and
    // the tree / scan steps per bucket (round 3: reduce 6.7 -> 5.9 ms at 2^20 per-window, 32.3 -> 29.8 ms at 2^24)
    if (p.L1 == MSM_REDUCE_L && programs(p.L1) > 1024) p.L1 = 2 * MSM_REDUCE_L;
    if (k.reduce_l >= 4 && k.reduce_l <= 128 && (k.reduce_l & (k.reduce_l - 1)) == 0) p.L1 = k.reduce_l;
    // Lean reduction (G1, inside a batch): level 1 stops after its serial part and hands every LANE's two sums to level 2
    // (msm_reduce_kernels.h, mode 2) -- 2 L1 - 1 steps per segment instead of 2 L1 + 17, a third fewer wave instructions for
    // the reduction, which inside a batch cost the accumulation beside it 3.2 of its 23.4 ms per MSM at 2^20 (measured by
    // leaving the reduction out).  The chain is longer (level 2 then folds 64 x as many items per window: 6.5 + 8.3 ms inside
    // a batch at 2^20 against 8.8 + 3.0), so an MSM that runs alone and the last one of a batch keep the segment form, and
    // so do short accumulations the longer chain would not fit behind (2^18 pairs: 12.8 instead of 8.0 ms per MSM).
    const bool long_list = p.entries >= ((size_t)1 << 25);
    p.lean = deg == 1 && (k.reduce_lean >= 0 ? k.reduce_lean != 0 : (!solo && !last && long_list));
    p.lane_buf = p.lean || (deg == 1 && !solo && long_list);
    const uint32_t seg_slots = (uint32_t)p.tpw * (uint32_t)p.L1;
    p.segs_per_window = (p.Q + seg_slots - 1) / seg_slots;
    p.L2 = (int)((p.segs_per_window + p.tpw - 1) / p.tpw);     // one wave per window
    if (p.entries >= ((size_t)1 << 31) || p.total >= ((size_t)1 << 31)) {
        p.status = MSM_PLAN_TOO_LARGE;
        return p;
    }
    // Bucket sums by affine rounds (aff_kernels.h): mode 0 = never, 1 = always, 2 = where they are measured
    // faster: on G2 (6 tower products per addition instead of 11: MNT4 G2 2^20 119 -> 80 ms, MNT6 G2 2^19 200 -> 130 ms)
    // once the list is long enough to fill the chip (a round costs at least one inversion's latency, ~0.3 ms).  On G1
    // the rounds tie with the projective kernel alone (22.9 vs 22.6 ms at 2^20: 0.7 x the instructions, but round 0 is
    // bound by its table gathers and every round pays an inversion per lane) and lose inside a pipelined batch
    // (30.4 vs 28.0 ms per MSM), so G1 stays projective unless asked.
    const int mode = k.affine >= 0 ? k.affine : affine_mode;
    p.tree = mode == 1 || (mode == 2 && deg >= 2 && p.entries >= ((size_t)1 << 21));
    // Heavy threshold.  Buckets are walked longest first, one per thread at ~78 us per addition
    // (2 waves / SIMD), so a bucket of s entries is free as long as s * 78 us stays well inside the
    // kernel's own duration (~ W n / 1.65e9 s); beyond that it would be the tail, and is split.
    // (merged windows: at least twice the mean bucket W n / 2^(c-1), so that chunking stays the exception)
    p.heavy_thr = p.merged ? (uint32_t)(((2 * p.entries) / (size_t)p.sets) >> (c - 1)) : (uint32_t)((4 * n) >> (c - 1));
    const uint32_t by_duration = (uint32_t)((double)p.W * (double)n * 3.1e-6);
    if (p.heavy_thr < by_duration) p.heavy_thr = by_duration;
    if (p.heavy_thr < 128) p.heavy_thr = 128;
    if (p.heavy_thr > (uint32_t)MSM_MAX_HEAVY_THRESHOLD) p.heavy_thr = MSM_MAX_HEAVY_THRESHOLD;
    p.max_heavy = p.entries / (p.heavy_thr + 1) + 1;            // buckets with > thr entries
    p.heavy_chunk = p.heavy_thr;                                // chunk = a bucket of threshold size
    p.max_chunks = p.entries / p.heavy_chunk + p.max_heavy + 1;
    return p;
}

// ---- the bucket sort of one MSM.  Large inputs: two-level counting sort with LDS atomics only (msm_kernels.h 2a); small ones:
// histogram + scatter with device-scope atomics (fewer launches).  GH_SORT forces one of them where it applies.
struct SortPlan {
    uint32_t tile = 0, bin_shift = 0, n_bins = 0, n_blocks = 0;
    bool part = false;              // the two-level counting sort
};
inline SortPlan plan_sort(size_t entries, size_t n, size_t total, const MsmKnobs& k) {
    SortPlan s;
    s.tile = entries > ((size_t)1 << 27) ? 65536u : 16384u;
    s.bin_shift = 8;
    auto bins_at = [&](uint32_t sh) { return (total + ((size_t)1 << sh) - 1) >> sh; };
    while (bins_at(s.bin_shift) > 1024) s.bin_shift++;
    // more than 2^23 buckets (2^24 pairs per window at c = 19: 40 x 2^18): up to MSM_PART_MAX_BINS bins of 2^13 buckets rather
    // than the device-scope atomics (sort 65 ms there)
    if (s.bin_shift > 13 && bins_at(13) <= (size_t)MSM_PART_MAX_BINS) s.bin_shift = 13;
    s.part = entries >= ((size_t)1 << 22) && n >= s.tile && s.bin_shift <= 13;
    if (k.sort == 1) s.part = false;
    if (k.sort == 2 && n >= s.tile && s.bin_shift <= 13) s.part = true;
    s.n_bins = (uint32_t)bins_at(s.bin_shift);
    s.n_blocks = (uint32_t)((entries + s.tile - 1) / s.tile);
    return s;
}

// ---- the affine rounds of one MSM (aff_kernels.h; msm_impl.h launch_tree)
struct PieceGeom {                  // one piece of a round: outputs [o0, o0 + n_piece), o0 a multiple of the tile size
    size_t t0;                      // first tile of the piece in every list
    uint32_t waves;                 // the C++ round kernel's waves
    uint32_t aw, Bq;                // the assembly kernels' waves and their batch per lane group
};
struct RoundSplit { uint32_t nA; bool split; };   // a round as two halves: outputs [0, nA) and [nA, n_out)

struct TreePlan {
    int R = 1;                      // rounds
    size_t stride = 0;              // words per round in the per-round count / offset arrays
    uint32_t K = 1;                 // chunks of buckets (the scratch lists are sized per chunk)
    uint32_t tpw = 64;              // lane groups per wave
    uint32_t max_waves = 0, asm_max_waves = 0, bmin = 8;
    int split_knob = 1, split_b = 32;

    // tpw = 64 / lanes per element; max_waves / asm_max_waves: what the C++ / the assembly round kernels may fill the card with
    TreePlan(uint32_t n0, size_t total, uint32_t maxc, int deg, uint32_t tpw_, uint32_t max_waves_, uint32_t asm_max_waves_,
             const MsmKnobs& k)
        : stride((total + 63) & ~(size_t)63), tpw(tpw_), max_waves(max_waves_), asm_max_waves(asm_max_waves_),
          bmin((uint32_t)k.aff_bmin), split_knob(k.aff_split), split_b(k.aff_split_b) {
        // rounds: down to ~leftover points per bucket on average (the late rounds are short batches -- one inversion per
        // lane and round -- while the projective finish is dense work), and no bucket left with more than aff_finish_max points
        const double left = k.leftover(deg), mean = (double)n0 / (double)(total > 1 ? total - 1 : 1);
        while (R < AFF_MAX_ROUNDS && (double)(1u << R) * left < mean) R++;
        if (k.aff_rounds > 0) R = k.aff_rounds;
        while (R < AFF_MAX_ROUNDS && (maxc >> R) > (uint32_t)k.aff_finish_max) R++;
    }

    // Chunks of buckets: the scratch lists of the rounds are sized per chunk, so that a 2^24-pair key (or a G2 key with
    // its shift table) does not need 300 GB of them.  ~420 bytes x lanes per list entry: the staged inputs, the two
    // output lists, the running products and the descriptors of a chunk.
    // (default 64 GB since round 3: a 2^20-pair G2 MSM then runs as ONE chunk -- 14.0 -> 14.4 M/s on MNT4 G2; the budget is cut to what
    //  is free next to the key anyway)
    // free_b: free device memory; have: what the slot's lists hold already.  False: no room at all, the projective kernel runs.
    bool set_chunks(uint32_t n0, int lanes, size_t free_b, size_t have, const MsmKnobs& k) {
        double budget = k.aff_scratch_gb * 1073741824.0;
        const double avail = ((double)free_b + (double)have - 3.0 * 1073741824.0) * 0.9;     // what this slot may hold at most
        if (budget > avail) budget = avail;
        const double need = 430.0 * lanes * (double)n0 * 1.13;                                // incl. the pool's 1/8 slack
        if (budget < 256.0 * 1048576.0) return false;
        K = 1;
        while ((double)K * budget < need && K < 4096) K++;
        return true;
    }

    PieceGeom piece(uint32_t n_piece, uint32_t o0) const {
        PieceGeom p;
        p.t0 = o0 / tpw;
        const uint32_t want = (n_piece + tpw * bmin - 1) / (tpw * bmin);
        p.waves = ((want > max_waves ? max_waves : want) + 3u) & ~3u;
        p.aw = ((want > asm_max_waves ? asm_max_waves : want) + 3u) & ~3u;
        p.Bq = (n_piece + p.aw * tpw - 1) / (p.aw * tpw);
        if (p.Bq < bmin) p.Bq = bmin;
        return p;
    }

    // A round = forward kernel, tower inversion of the lane groups' running products, backward kernel.  The inversion is
    // 0.4 ms of latency with the card nearly idle.  A large round therefore goes out as two halves of its output range on two
    // streams, the second half one kernel behind the first: the inversion of either half runs beside a forward / backward
    // kernel of the other (GH_AFF_SPLIT=0: one piece; halves are whole tiles, the first one a multiple of four tiles, so every
    // list keeps its layout).  Only the assembly rounds (aff_asm) are split.
    RoundSplit split(uint32_t n_out, bool aff_asm) const {
        RoundSplit s;
        s.nA = ((n_out / 2 + 4 * tpw - 1) / (4 * tpw)) * (4 * tpw);
        s.split = aff_asm && split_knob != 0 && s.nA < n_out;
        if (s.split) {   // batch per lane group if the round went out in one piece
            const uint32_t whole = (uint32_t)(((size_t)n_out + (size_t)asm_max_waves * tpw - 1) / ((size_t)asm_max_waves * tpw));
            s.split = whole >= (uint32_t)split_b;
        }
        return s;
    }
};

}  // namespace gh_rt
