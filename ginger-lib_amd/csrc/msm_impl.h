// msm_impl.h -- host-side launch sequence of the MSM (templated on the curve policy): one job, its stages, the batch.
// Included by the four msm_<curve>.hip translation units.  The arithmetic behind the launches is in msm_plan.h, the host
// fold of the window sums in msm_fold.h, the resident key (bases, shift table, equal bases) in msm_key.h.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <memory>
#include <type_traits>
#include <vector>
#include "runtime.h"
#include "msm_kernels.h"
#include "asm_kernels.h"
#include "msm_plan.h"
#include "msm_fold.h"
#include "msm_key.h"

namespace gh_rt {
using namespace gh;

// generator constants (ABI Montgomery limbs): curves/mnt{4,6}753/{g1,g2}.rs AFFINE_GENERATOR_COEFFS
template <class C> struct GenConst;
template <> struct GenConst<Mnt4G1> { static void get(uint64_t* xy) { static const uint64_t x[12] = GH_MNT4753_G1_GX0_M_64, y[12] = GH_MNT4753_G1_GY0_M_64; memcpy(xy, x, 96); memcpy(xy + 12, y, 96); } };
template <> struct GenConst<Mnt6G1> { static void get(uint64_t* xy) { static const uint64_t x[12] = GH_MNT6753_G1_GX0_M_64, y[12] = GH_MNT6753_G1_GY0_M_64; memcpy(xy, x, 96); memcpy(xy + 12, y, 96); } };
template <> struct GenConst<Mnt4G2> { static void get(uint64_t* xy) {
    static const uint64_t x0[12] = GH_MNT4753_G2_GX0_M_64, x1[12] = GH_MNT4753_G2_GX1_M_64, y0[12] = GH_MNT4753_G2_GY0_M_64, y1[12] = GH_MNT4753_G2_GY1_M_64;
    memcpy(xy, x0, 96); memcpy(xy + 12, x1, 96); memcpy(xy + 24, y0, 96); memcpy(xy + 36, y1, 96); } };
template <> struct GenConst<Mnt6G2> { static void get(uint64_t* xy) {
    static const uint64_t x0[12] = GH_MNT6753_G2_GX0_M_64, x1[12] = GH_MNT6753_G2_GX1_M_64, x2[12] = GH_MNT6753_G2_GX2_M_64;
    static const uint64_t y0[12] = GH_MNT6753_G2_GY0_M_64, y1[12] = GH_MNT6753_G2_GY1_M_64, y2[12] = GH_MNT6753_G2_GY2_M_64;
    memcpy(xy, x0, 96); memcpy(xy + 12, x1, 96); memcpy(xy + 24, x2, 96); memcpy(xy + 36, y0, 96); memcpy(xy + 48, y1, 96); memcpy(xy + 60, y2, 96); } };

// scalar-field modulus of the curve (MNT4: r = p6, MNT6: r = p4) as 24 LE 32-bit words
template <class C> MsmModulus scalar_modulus() {
    static const uint32_t r4[24] = GH_P6_P_32, r6[24] = GH_P4_P_32;
    const bool mnt4 = CurveId<C>::id == GH_MNT4753_G1 || CurveId<C>::id == GH_MNT4753_G2;
    MsmModulus m;
    memcpy(m.w, mnt4 ? r4 : r6, sizeof m.w);
    return m;
}

template <class C> int make_salts(Aff<C>* out) {
    typedef typename C::F F;
    uint64_t xy[72];
    GenConst<C>::get(xy);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(xy);
    out[0].x = F::from_abi(w);
    out[0].y = F::from_abi(w + 24 * F::DEG);
    Proj<C> g2 = proj_dbl<C>(Proj<C>{out[0].x, out[0].y, F::one()});
    typename F::T zi = host_inv<F>(g2.z);
    out[1].x = F::mul(g2.x, zi);
    out[1].y = F::mul(g2.y, zi);
    return GH_OK;
}

// salt points S0 = G, S1 = 2G (internal affine form) for the accumulate kernels' detour, resident once per curve
template <class C> int device_salts(Aff<C>** out) {
    static Aff<C>* d_salts = nullptr;
    if (!d_salts) {
        Aff<C> hs[2];
        if (int src = make_salts<C>(hs)) return src;
        HIPCHK(hipMalloc((void**)&d_salts, sizeof(hs)));
        HIPCHK(hipMemcpy(d_salts, hs, sizeof(hs), hipMemcpyHostToDevice));
        g.at_shutdown.push_back([] { if (d_salts) hipFree(d_salts); d_salts = nullptr; });
    }
    *out = d_salts;
    return GH_OK;
}

// lane-group field of a curve's kernels: one lane per element (G1), lane pairs with the dual product (Fq2), lane triples with
// the single-reduction triple product (Fq3: six product sites per addition, where the projective kernel's eleven did
// not get through hipcc unrolled)
template <class C> struct SplitFS {
    typedef typename std::conditional<C::F::DEG == 1, F1S<typename C::PF>,
            typename std::conditional<C::F::DEG == 2, F2S<P4, 13>, F3S<P6, 11>>::type>::type type;
};

// The bucket-sum kernels over `total` lists: out[g] = sum of points[sorted[starts[g] + k] & 0x7FFFFFFF] (bit 31: negated),
// k < counts[g], in the order `order` names them, the chunks of the n_heavy longest lists first (their sums go to `partials`).
// AFFIN: the lists are runs of the affine rounds' T64 output `points` instead (no index list, no order, no chunks): list
// bucket0 + g starts at starts[g] - in_base.
template <class C> struct BucketSumArgs {
    const void* points = nullptr;
    const uint32_t *sorted = nullptr, *starts = nullptr, *counts = nullptr, *order = nullptr;
    uint32_t total = 0;
    const Aff<C>* salts = nullptr;
    Proj<C>* out = nullptr;
    const uint32_t* chunk_start = nullptr;
    uint32_t n_heavy = 0, n_chunks = 0, heavy_chunk = 0;
    Proj<C>* partials = nullptr;
    uint32_t bucket0 = 0, in_base = 0;
};
// One launch: G1 on XYZZ accumulators (msm_kernels.h 4a: 10 multiplications / 9 reductions per update) -- by the assembly
// kernel (asmgen/g1_xyzz.py: the same updates on a fixed register plan, 0 B of scratch; it needs a task table, pooled as
// `task_pool`) where it is enabled and the lists are index lists -- G2 one coefficient per lane, 2 (Fq2) / 3 (Fq3) lanes
// per list (msm_kernels.h 4b).
template <class C, bool AFFIN>
int launch_bucket_sums(const BucketSumArgs<C>& a, const std::string& task_pool, hipStream_t st) {
    const size_t tasks = (size_t)a.n_chunks + (a.total - a.n_heavy);
    if constexpr (C::F::DEG == 1) {
        if (!AFFIN && gh_asm::enabled()) {
            gh_asm::AccTask* tk = nullptr;
            // 16 bytes behind the table: the tile counter of the persistent form
            if (int rc = pool_get(task_pool.c_str(), tasks * sizeof(gh_asm::AccTask) + 16, (void**)&tk)) return rc;
            uint32_t* const counter = (uint32_t*)(tk + tasks);
            GH_LAUNCH((msm_acc_tasks_kernel<C>), dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, st, a.starts, a.counts, a.order,
                      a.total, a.out, a.chunk_start, a.n_heavy, a.n_chunks, a.heavy_chunk, a.partials, (AccTaskRec*)tk, counter);
            return gh_asm::acc_g1_launch(std::is_same<typename C::PF, P6>::value ? 6 : 4, a.points, a.sorted, tk, a.salts, (uint32_t)tasks,
                                         counter, st);
        }
        GH_LAUNCH((msm_accumulate_xyzz_kernel<C, AFFIN>), dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, st,
                  (const Aff<C>*)a.points, a.sorted, a.starts, a.counts, a.order, a.total, a.salts, a.out, a.chunk_start, a.n_heavy,
                  a.n_chunks, a.heavy_chunk, a.partials, a.bucket0, a.in_base);
    } else {
        typedef typename SplitFS<C>::type FS;
        constexpr int LANES = FS::LANES;
        const size_t waves = (tasks + (64 / LANES) - 1) / (64 / LANES);
        GH_LAUNCH((msm_accumulate_split_kernel<C, FS, LANES, AFFIN>), dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, st,
                  (const Aff<C>*)a.points, a.sorted, a.starts, a.counts, a.order, a.total, a.salts, a.out, a.chunk_start, a.n_heavy,
                  a.n_chunks, a.heavy_chunk, a.partials, a.bucket0, a.in_base);
    }
    return GH_OK;
}

// ---- affine rounds (aff_kernels.h): what one MSM's rounds share, and one piece of a round
template <class C> struct TreeLists {
    const Aff<C>* rows = nullptr;          // the bases / the shift table
    const uint32_t* sorted = nullptr;
    uint32_t* desc = nullptr;
    void *ptsA = nullptr, *ptsB = nullptr, *prefix = nullptr, *stage1 = nullptr, *stage2 = nullptr;     // T64 lists (aff_kernels.h)
    // the assembly rounds' control data, two copies: a large round is issued as two halves (MsmJob::issue_round)
    void* asm_accs = nullptr;
    uint32_t* asm_flag = nullptr;          // per half: control block + exception list
    size_t accs_half = 0, flag_words = 0;
};

// one piece of a round: outputs [o0, o0 + n_piece) (o0 a multiple of the tile size); which: 0 / 1 = control block, stream role
template <class C> struct Piece {
    AffRoundArgs<C> a;                     // the C++ round kernel's arguments
    gh_asm::AffArgs q;                     // the assembly kernels'
    uint32_t waves_cpp, aw, Bq;
    uint32_t* flag;
    void* accs;
    // in / out: the round's input (null in round 0) and output list; desc: the piece's descriptors; in_base: first element of the
    // chunk in the round's input list
    Piece(const TreePlan& tp, const TreeLists<C>& L, int r, const void* in, void* out, const uint32_t* desc, uint32_t o0,
          uint32_t n_piece, uint32_t in_base, int which) {
        const PieceGeom geo = tp.piece(n_piece, o0);
        auto off = [&](void* base, int chunks) { return (void*)((char*)base + t64_bytes(geo.t0, chunks)); };
        a.rows = L.rows; a.in = in; a.sorted = r == 0 ? L.sorted : nullptr; a.desc = desc; a.n_out = n_piece; a.in_base = in_base;
        a.prefix = off(L.prefix, T64_FP_CHUNKS); a.out = off(out, T64_PT_CHUNKS);
        a.stage1 = off(L.stage1, T64_PT_CHUNKS); a.stage2 = off(L.stage2, T64_PT_CHUNKS);
        a.groups = geo.waves * tp.tpw; a.bmin = tp.bmin;
        a.run_if = nullptr;
        waves_cpp = geo.waves; aw = geo.aw; Bq = geo.Bq;
        flag = L.asm_flag ? L.asm_flag + (size_t)which * L.flag_words : nullptr;
        accs = L.asm_accs ? (void*)((char*)L.asm_accs + (size_t)which * L.accs_half) : nullptr;
        q.in = r == 0 ? (const void*)L.rows : in; q.sorted = L.sorted; q.desc = a.desc; q.prefix = a.prefix;
        q.stage1 = a.stage1; q.stage2 = a.stage2; q.out = a.out; q.accs = accs; q.flag = flag;
        q.n_out = n_piece; q.in_base = in_base; q.B = Bq; q.pad = 0;
    }
};

// The second stream of a split round: fork() lets g.stream_acc2 start behind what `st` holds so far, join() makes `st` wait for
// it.  Whatever way the scope is left after fork() -- an error return between the two included -- the destructor joins, so
// that nothing still runs on the second stream, on pooled buffers, when the caller's error path releases them.
struct RoundFork {
    hipStream_t st, st2;
    bool open = false;
    RoundFork(hipStream_t st_, hipStream_t st2_) : st(st_), st2(st2_) {}
    RoundFork(const RoundFork&) = delete;
    RoundFork& operator=(const RoundFork&) = delete;
    int fork() {
        HIPCHK(hipEventRecord(g.tev[0], st));
        HIPCHK(hipStreamWaitEvent(st2, g.tev[0], 0));
        open = true;
        return GH_OK;
    }
    int join() {
        open = false;
        HIPCHK(hipEventRecord(g.tev[1], st2));
        HIPCHK(hipStreamWaitEvent(st, g.tev[1], 0));
        return GH_OK;
    }
    ~RoundFork() {      // an error is on its way out: join without touching its message
        if (!open) return;
        (void)hipEventRecord(g.tev[1], st2);
        (void)hipStreamWaitEvent(st, g.tev[1], 0);
    }
};

// One MSM as a sequence of stages, so that several MSMs can be pipelined over HIP streams
// (msm_batch below): sort -> [host reads the chunk plan] -> accumulate -> reduce -> [host fold].
// Every stage works on the buffers of one of two slots.
template <class C>
struct MsmJob {
    typedef typename SplitFS<C>::type FS;
    static constexpr int DEG = C::F::DEG;

    BasesBase* h = nullptr;
    const void* d_scalars = nullptr;
    uint64_t* out_xyz = nullptr;
    size_t n = 0;
    int slot = 0;
    bool solo = false;               // a batch of one (set by msm_batch): nothing runs beside this MSM
    bool last = false;               // the last MSM of its batch: its reduction has nothing to hide behind
    int es = 0;                      // event set (g.pev[es]): the job's index in its batch mod 4, so that the sort of job k+1 can be
                                     // issued while job k-1 (same buffer slot) still waits for its window sums
    MsmPlan p;                       // window, bucket sets, reduction geometry, thresholds (msm_plan.h)
    bool tree = false;               // bucket sums by affine rounds: p.tree, until their scratch turns out not to fit
    uint32_t n_heavy = 0, n_chunks = 0;
    int32_t* digits = nullptr;
    uint32_t *counts = nullptr, *starts = nullptr, *cursor = nullptr, *sorted = nullptr, *order = nullptr, *size_hist = nullptr,
             *size_cursor = nullptr, *chunk_start = nullptr, *plan = nullptr;
    Proj<C>*buckets = nullptr, *seg_out = nullptr, *win_out = nullptr, *partials = nullptr, *lane_out = nullptr;
    uint32_t* red_flag = nullptr;                        // lean level 1 by the generated kernel: per program, "compute it again"
    uint32_t *aff_cnt = nullptr, *aff_st = nullptr;      // affine rounds: per round, the buckets' sizes and offsets
    bool aff_sticky_pending = false;
    uint32_t* hplan = nullptr;      // pinned
    Proj<C>* hw = nullptr;          // pinned, 9 RW points
    Aff<C>* salts = nullptr;
    std::chrono::steady_clock::time_point t_begin;
    gh_msm_timing_t tm{};

    // staging buffers per job in flight (set = the job's event set, k & 3): job k+1 is prepared while job k-1 -- same buffer slot --
    // still has its window sums on the way, so the two must not share (or re-allocate) a pinned buffer
    static int pinned(int slot, int which, size_t bytes, void** out) {
        static void* p[4][2] = {};
        static size_t cap[4][2] = {};
        static bool registered = false;
        if (!registered) {   // gh_shutdown releases the staging buffers
            registered = true;
            g.at_shutdown.push_back([] {
                for (auto& sl : p) for (auto& q : sl) { if (q) hipHostFree(q); q = nullptr; }
                for (auto& sl : cap) for (auto& q : sl) q = 0;
                registered = false;
            });
        }
        if (cap[slot][which] < bytes) {
            if (p[slot][which]) HIPCHK(hipHostFree(p[slot][which]));
            p[slot][which] = nullptr; cap[slot][which] = 0;
            HIPCHK(hipHostMalloc(&p[slot][which], bytes + 256, hipHostMallocDefault));
            cap[slot][which] = bytes + 256;
        }
        *out = p[slot][which];
        return GH_OK;
    }

    int prepare(BasesBase* h_, const void* d_scalars_, size_t n_scalars, uint64_t* out, int slot_) {
        h = h_; d_scalars = d_scalars_; out_xyz = out; slot = slot_;
        n = h->n < n_scalars ? h->n : n_scalars;
        t_begin = std::chrono::steady_clock::now();
        if (n == 0) return GH_OK;
        p = plan_msm(n, DEG, h->d_table != nullptr, h->pre_c, h->pre_G, solo, last, g.window_override, g.affine_mode, msm_knobs());
        if (p.status == MSM_PLAN_TOO_LARGE) {
            g_err = "MSM too large for 31-bit list entries";
            return GH_E_UNSUPPORTED;
        }
        tree = p.tree;
        if (int src = device_salts<C>(&salts)) return src;
        int rc;
        if ((rc = slot_buf("digits", slot, p.entries * 4, &digits)) ||
            (rc = slot_buf("counts", slot, p.total * 4, &counts)) ||
            (rc = slot_buf("starts", slot, p.total * 4, &starts)) ||
            (rc = slot_buf("cursor", slot, p.total * 4, &cursor)) ||
            (rc = slot_buf("sorted", slot, p.entries * 4, &sorted)) ||
            (rc = slot_buf("order", slot, p.total * 4, &order)) ||
            (rc = slot_buf("size_hist", slot, MSM_SIZE_BINS * 4, &size_hist)) ||
            (rc = slot_buf("size_cursor", slot, MSM_SIZE_BINS * 4, &size_cursor)) ||
            (rc = slot_buf("chunk_start", slot, (p.max_heavy + 2) * 4, &chunk_start)) ||
            (rc = slot_buf("plan", slot, 64, &plan)) ||
            (rc = slot_buf("buckets", slot, p.total * sizeof(Proj<C>), &buckets)) ||
            (rc = slot_buf("seg_out", slot, (size_t)p.RW * p.segs_per_window * 3 * sizeof(Proj<C>), &seg_out)) ||
            (rc = slot_buf("win_out", slot, (size_t)3 * p.RW * 3 * sizeof(Proj<C>), &win_out)))
            return rc;
        // (also for the last MSM of a batch, which does not use it: a buffer that is first allocated in the middle of a later batch
        //  costs that batch a device-wide wait -- 9 ms at 2^20)
        if (p.lane_buf && (rc = slot_buf("lane_out", slot, (size_t)p.RW * p.segs_per_window * 64 * 2 * sizeof(Proj<C>), &lane_out))) return rc;
        if (p.lane_buf && (rc = slot_buf("reduce_flag", slot, (size_t)p.RW * p.segs_per_window * 4 + 64, &red_flag))) return rc;
        if ((rc = pinned(es, 0, 512, (void**)&hplan))) return rc;
        if ((rc = pinned(es, 1, (size_t)9 * p.RW * sizeof(Proj<C>), (void**)&hw))) return rc;
        return GH_OK;
    }

    // the scalars of equal bases, added up (msm_kernels.h "equal bases"): the MSM sees the distinct bases only
    int merge_equal_bases(hipStream_t st) {
        int rc;
        uint32_t *merged_s = nullptr, *partial = nullptr;
        if ((rc = slot_buf("merged_scalars", slot, n * 96, &merged_s))) return rc;
        HIPCHK(hipMemcpyAsync(merged_s, d_scalars, n * 96, hipMemcpyDeviceToDevice, st));
        if ((rc = slot_buf("merged_partial", slot, (size_t)h->n_dup_chunks * 96 + 96, &partial))) return rc;
        GH_LAUNCH(msm_merge_scalars_kernel, dim3(h->n_dup_chunks), dim3(256), 0, st, (const uint32_t*)d_scalars, merged_s, n,
                  (const uint32_t*)h->d_dup_starts, (const uint32_t*)h->d_dup_members, (const uint32_t*)h->d_dup_chunks, h->n_dup_chunks,
                  partial, scalar_modulus<C>());
        GH_LAUNCH(msm_merge_groups_kernel, dim3((h->n_dup_groups + 63) / 64), dim3(64), 0, st, merged_s, n, (const uint32_t*)h->d_dup_starts,
                  (const uint32_t*)h->d_dup_members, (const uint32_t*)(h->d_dup_chunks + 3 * (size_t)h->n_dup_chunks), h->n_dup_groups,
                  (const uint32_t*)partial, scalar_modulus<C>());
        d_scalars = merged_s;
        return GH_OK;
    }

    // digits of every scalar (and, with `hist`, the buckets' histogram by device-scope atomics)
    int launch_digits(uint32_t* hist, hipStream_t st) {
        GH_LAUNCH(msm_digits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_scalars, (const uint8_t*)h->d_inf,
                  n, p.c, p.W, p.nb, p.top_unsigned, scalar_modulus<C>(), digits, hist, msm_knobs().agg_iters, p.merged ? 1u : 0u, (uint32_t)p.sets);
        return GH_OK;
    }

    // bucket lists by the two-level counting sort (msm_kernels.h 2a): counts / starts / sorted
    int sort_partitioned(const SortPlan& sp, hipStream_t st) {
        int rc;
        MsmPartArgs a;
        a.digits = digits; a.entries = p.entries; a.n = n;
        a.win_stride = p.nb; a.row_stride = p.merged ? (uint32_t)h->n : 0u; a.slot_shift = p.merged ? 1u : 0u;
        a.sets = (uint32_t)p.sets;
        a.bin_shift = sp.bin_shift; a.n_bins = sp.n_bins;
        a.tile = sp.tile; a.n_blocks = sp.n_blocks;
        const size_t cells = (size_t)a.n_bins * a.n_blocks + 1;
        uint32_t *block_hist = nullptr, *block_off = nullptr;
        uint2* part = nullptr;
        if ((rc = slot_buf("part_hist", slot, cells * 4, &block_hist)) ||
            (rc = slot_buf("part_off", slot, cells * 4, &block_off)) ||
            (rc = slot_buf("part_pairs", slot, p.entries * 8, &part))) return rc;
        if ((rc = launch_digits(nullptr, st))) return rc;
        HIPCHK(hipMemsetAsync(block_hist + (cells - 1), 0, 4, st));
        GH_LAUNCH(msm_part_hist_kernel, dim3(a.n_blocks), dim3(MSM_PART_THREADS), 0, st, a, block_hist);
        HIPCHK(hipGetLastError());
        if ((rc = device_scan(block_hist, block_off, cells, slot_name("scan_tmp3", slot).c_str(), st))) return rc;
        GH_LAUNCH(msm_part_scatter_kernel, dim3(a.n_blocks), dim3(MSM_PART_THREADS), 0, st, a, (const uint32_t*)block_off, part);
        GH_LAUNCH(msm_bin_sort_kernel, dim3(a.n_bins), dim3(MSM_BIN_THREADS), (size_t)4 << sp.bin_shift, st, (const uint2*)part,
                  (const uint32_t*)block_off, a.n_blocks, sp.bin_shift, (uint32_t)p.total, counts, starts, sorted);
        HIPCHK(hipGetLastError());
        return GH_OK;
    }

    // stage 1 (stream st): digits + histogram, scan, bucket order by size, heavy plan, scatter; plan -> host
    int launch_sort(hipStream_t st) {
        if (n == 0) return GH_OK;
        int rc;
        const size_t total = p.total;
        HIPCHK(hipEventRecord(g.pev[es][0], st));
        HIPCHK(hipMemsetAsync(size_hist, 0, MSM_SIZE_BINS * 4, st));
        HIPCHK(hipMemsetAsync(plan, 0, 64, st));
        if (h->n_dup_groups && (rc = merge_equal_bases(st))) return rc;
        const SortPlan sp = plan_sort(p.entries, n, total, msm_knobs());
        if (sp.part) {
            if ((rc = sort_partitioned(sp, st))) return rc;
        } else {      // histogram by device-scope atomics, scan; the scatter follows the heavy plan
            HIPCHK(hipMemsetAsync(counts, 0, total * 4, st));
            if ((rc = launch_digits(counts, st))) return rc;
            HIPCHK(hipGetLastError());
            if ((rc = device_scan(counts, starts, total, "scan_tmp", st))) return rc;
            HIPCHK(hipMemcpyAsync(cursor, starts, total * 4, hipMemcpyDeviceToDevice, st));
        }
        GH_LAUNCH(msm_size_hist_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, counts, total, p.heavy_thr, size_hist, plan + 4);
        if ((rc = device_scan(size_hist, size_cursor, MSM_SIZE_BINS, "scan_tmp2", st))) return rc;
        GH_LAUNCH(msm_size_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, counts, total, p.heavy_thr, size_cursor, order);
        GH_LAUNCH(msm_heavy_plan_kernel, dim3(1), dim3(1), 0, st, (const uint32_t*)size_hist, (const uint32_t*)counts,
                  (const uint32_t*)order, (const uint32_t*)starts, (uint32_t)total, p.heavy_chunk, chunk_start, plan);
        if (!sp.part)
            GH_LAUNCH(msm_scatter_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)p.W), dim3(256), 0, st,
                      (const int32_t*)digits, n, p.W, p.nb, p.merged ? (uint32_t)h->n : 0u, cursor, sorted, msm_knobs().agg_iters,
                      p.merged ? 1u : 0u, (uint32_t)p.sets);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hplan, plan, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(g.pev[es][1], st));
        return GH_OK;
    }

    // stage 2 (stream st): waits on the host for the plan of stage 1, then the accumulation launch
    int launch_accumulate(hipStream_t st) {
        if (n == 0) return GH_OK;
        int rc;
        HIPCHK(hipEventSynchronize(g.pev[es][1]));
        n_heavy = hplan[0]; n_chunks = hplan[1];
        tm.accumulate_madds = hplan[2];
        if (n_heavy > p.max_heavy || n_chunks > p.max_chunks) { g_err = "internal: heavy-bucket plan out of range"; return GH_E_HIP; }
        partials = nullptr;
        if (n_heavy > 0 && (rc = slot_buf("partials", slot, (size_t)n_chunks * sizeof(Proj<C>), &partials))) return rc;
        HIPCHK(hipEventRecord(g.pev[es][2], st));
        if (tree) {   // may clear `tree` when its scratch does not fit next to the key: the projective kernel takes over
            if ((rc = launch_tree(st))) return rc;
        }
        if (!tree) {
            // one launch: the chunks of the heavy buckets first, then every other bucket, longest first
            BucketSumArgs<C> a;
            a.points = p.merged ? h->d_table : h->d_points;
            a.sorted = sorted; a.starts = starts; a.counts = counts; a.order = order; a.total = (uint32_t)p.total;
            a.salts = salts; a.out = buckets;
            a.chunk_start = chunk_start; a.n_heavy = n_heavy; a.n_chunks = n_chunks; a.heavy_chunk = p.heavy_chunk; a.partials = partials;
            if ((rc = launch_bucket_sums<C, false>(a, slot_name("acc_tasks", slot), st))) return rc;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(g.pev[es][3], st));
        if (n_heavy > 0) {   // one wave per heavy bucket adds its chunk sums
            GH_LAUNCH((msm_heavy_combine_kernel<C>), dim3(n_heavy), dim3(64), 64 * sizeof(Proj<C>), st, (const Proj<C>*)partials,
                      (const uint32_t*)order, (const uint32_t*)chunk_start, buckets);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(g.pev[es][4], st));
        return GH_OK;
    }

    // ---- Bucket sums by affine rounds (aff_kernels.h) on stream st: plan (per-round bucket sizes and offsets: R small
    // scans), R rounds per chunk of buckets (descriptor kernel + round kernels), then the projective kernel over what is left
    // per bucket.
    struct TreeRun {
        TreePlan tp;
        TreeLists<C> L;
        std::vector<uint32_t> bq, tab;     // per chunk boundary: the first bucket; the first element of every round's list
        bool aff_asm = false;              // the assembly round kernels (asmgen/g2_rounds.py) with the C++ kernel as their fallback
        int asm_kind = 0;
        uint32_t T(uint32_t j, int r) const { return tab[(size_t)j * (tp.R + 1) + r]; }
    };
    const uint32_t* round_starts(const TreeRun& t, int r) const { return r == 0 ? starts : aff_st + (size_t)(r - 1) * t.tp.stride; }
    const uint32_t* round_counts(const TreeRun& t, int r) const { return r == 0 ? counts : aff_cnt + (size_t)(r - 1) * t.tp.stride; }

    // the buckets' sizes and offsets in every round's list
    int tree_counts(const TreePlan& tp, hipStream_t st) {
        int rc;
        const size_t total = p.total;
        if ((rc = slot_buf("aff_cnt", slot, (size_t)tp.R * tp.stride * 4, &aff_cnt)) ||
            (rc = slot_buf("aff_st", slot, (size_t)tp.R * tp.stride * 4, &aff_st))) return rc;
        GH_LAUNCH(aff_counts_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                  (const uint32_t*)counts, (uint32_t)total, tp.R, tp.stride, aff_cnt);
        const std::string scan_nm = slot_name("aff_scan", slot);
        for (int r = 1; r <= tp.R; r++)
            if ((rc = device_scan(aff_cnt + (size_t)(r - 1) * tp.stride, aff_st + (size_t)(r - 1) * tp.stride, total, scan_nm.c_str(), st))) return rc;
        return GH_OK;
    }

    // the chunks' boundaries: first bucket (bq) and first element of every round's list (tab), computed on the device
    int tree_chunk_tables(TreeRun& t, uint32_t n0, hipStream_t st) {
        int rc;
        const uint32_t K = t.tp.K;
        const int R = t.tp.R;
        uint32_t *d_bq, *d_tab;
        if ((rc = slot_buf("aff_bq", slot, ((size_t)K + 2) * 4, &d_bq)) ||
            (rc = slot_buf("aff_tab", slot, ((size_t)K + 2) * (R + 1) * 4, &d_tab))) return rc;
        GH_LAUNCH(aff_chunks_kernel, dim3((K + 1 + 63) / 64), dim3(64), 0, st, (const uint32_t*)starts, (const uint32_t*)counts,
                  (const uint32_t*)aff_st, (const uint32_t*)aff_cnt, (uint32_t)p.total, R, t.tp.stride, K, d_bq, d_tab);
        HIPCHK(hipGetLastError());
        t.bq.resize((size_t)K + 1);
        t.tab.resize(((size_t)K + 1) * (R + 1));
        HIPCHK(hipMemcpyAsync(t.bq.data(), d_bq, t.bq.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(t.tab.data(), d_tab, t.tab.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (t.T(K, 0) != n0) { g_err = "internal: affine plan disagrees with the sort stage"; return GH_E_HIP; }
        return GH_OK;
    }

    // the lists of the rounds, sized by the largest chunk.  GH_E_NOMEM: they do not fit
    int tree_lists(TreeRun& t) {
        int rc;
        const int R = t.tp.R;
        uint32_t max_n1 = 0, max_n2 = 0;
        size_t max_desc = 0;
        for (uint32_t j = 0; j < t.tp.K; j++) {
            const uint32_t n1 = t.T(j + 1, 1) - t.T(j, 1), n2 = R >= 2 ? t.T(j + 1, 2) - t.T(j, 2) : 0;
            if (n1 > max_n1) max_n1 = n1;
            if (n2 > max_n2) max_n2 = n2;
            size_t dsum = 0;
            for (int r = 1; r <= R; r++) dsum += t.T(j + 1, r) - t.T(j, r);
            if (dsum > max_desc) max_desc = dsum;
        }
        auto tiles = [&](uint32_t n_el) { return ((size_t)n_el + t.tp.tpw - 1) / t.tp.tpw + 1; };
        TreeLists<C>& L = t.L;
        if ((rc = slot_buf("aff_desc", slot, (max_desc + 64) * 4, &L.desc)) ||
            (rc = slot_buf("aff_ptsA", slot, t64_bytes(tiles(max_n1), T64_PT_CHUNKS), &L.ptsA)) ||
            (rc = slot_buf("aff_ptsB", slot, t64_bytes(tiles(max_n2), T64_PT_CHUNKS), &L.ptsB)) ||
            (rc = slot_buf("aff_prefix", slot, t64_bytes(tiles(max_n1), T64_FP_CHUNKS), &L.prefix)) ||
            (rc = slot_buf("aff_stage1", slot, t64_bytes(tiles(max_n1), T64_PT_CHUNKS), &L.stage1)) ||
            (rc = slot_buf("aff_stage2", slot, t64_bytes(tiles(max_n1), T64_PT_CHUNKS), &L.stage2))) return rc;
        return GH_OK;
    }

    // The assembly kernels (asmgen/g2_rounds.py): forward pass, tower inversion of the lane groups' running products, backward
    // pass -- 256 registers, two waves per SIMD, no scratch, no out-of-line product.  Elements on the group law's rare branches
    // go through an exception list (aff_fix_kernel); only if the list overflowed, the whole piece once more on the C++ kernel.
    static int issue_fwd(const TreeRun& t, Piece<C>& P, int r, hipStream_t s) {
        HIPCHK(hipMemsetAsync(P.flag, 0, 16, s));
        return gh_asm::aff_launch(t.asm_kind, true, r == 0, P.q, P.aw, s);
    }
    static int issue_rest(const TreeRun& t, Piece<C>& P, int r, hipStream_t s) {
        GH_LAUNCH((aff_inv_kernel<FS>), dim3(P.aw / 4), dim3(256), 0, s, P.accs, P.aw, P.a.n_out, P.Bq, (const uint32_t*)P.flag);
        if (int rc = gh_asm::aff_launch(t.asm_kind, false, r == 0, P.q, P.aw, s)) return rc;
        if (r == 0) GH_LAUNCH((aff_fix_kernel<C, FS, true>), dim3(16), dim3(256), 0, s, P.a, (const uint32_t*)P.flag);
        else GH_LAUNCH((aff_fix_kernel<C, FS, false>), dim3(16), dim3(256), 0, s, P.a, (const uint32_t*)P.flag);
        P.a.run_if = P.flag;
        return GH_OK;
    }
    static int issue_cpp(Piece<C>& P, int r, hipStream_t s) {   // the C++ round kernel: the whole piece, or (run_if) its fallback
        if (r == 0) GH_LAUNCH((aff_round_kernel<C, FS, true>), dim3(P.waves_cpp / 4), dim3(256), 0, s, P.a);
        else GH_LAUNCH((aff_round_kernel<C, FS, false>), dim3(P.waves_cpp / 4), dim3(256), 0, s, P.a);
        return GH_OK;
    }
    // GH_AFF_DEBUG: how many elements of the round went through the exception list / whether it overflowed
    static int debug_round(const Piece<C>& P, uint32_t j, int r, uint32_t n_out, hipStream_t st) {
        uint32_t fw[4] = {0, 0, 0, 0};
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(fw, P.flag, 16, hipMemcpyDeviceToHost));
        fprintf(stderr, "[gh aff] chunk %u round %d n_out %u waves %u B %u in_base %u redo %u exceptions %u\n", j, r, n_out, P.aw, P.Bq,
                P.q.in_base, fw[0], fw[1]);
        return GH_OK;
    }

    // round r of chunk j: n_out outputs from list `in` (null: round 0, the sorted list) to list `out`; desc: the round's descriptors
    int issue_round(const TreeRun& t, uint32_t j, int r, uint32_t n_out, const void* in, void* out, uint32_t* desc, hipStream_t st) {
        int rc;
        unsigned dgrid = (n_out + 255) / 256;
        if (dgrid > 16384) dgrid = 16384;
        GH_LAUNCH(aff_desc_kernel, dim3(dgrid), dim3(256), 0, st, round_starts(t, r), round_counts(t, r),
                  (const uint32_t*)(aff_st + (size_t)r * t.tp.stride), (uint32_t)p.total, t.T(j, r + 1), n_out, desc);
        const uint32_t in_base = t.T(j, r);
        const RoundSplit sp = t.tp.split(n_out, t.aff_asm);
        if (!sp.split) {
            Piece<C> P(t.tp, t.L, r, in, out, desc, 0, n_out, in_base, 0);
            if (t.aff_asm) {
                if ((rc = issue_fwd(t, P, r, st)) || (rc = issue_rest(t, P, r, st))) return rc;
                if (msm_knobs().aff_debug && (rc = debug_round(P, j, r, n_out, st))) return rc;
            }
            return issue_cpp(P, r, st);
        }
        Piece<C> A(t.tp, t.L, r, in, out, desc, 0, sp.nA, in_base, 0);
        Piece<C> B(t.tp, t.L, r, in, out, desc + sp.nA, sp.nA, n_out - sp.nA, in_base, 1);
        RoundFork fk(st, g.stream_acc2);
        if ((rc = issue_fwd(t, A, r, st))) return rc;
        if ((rc = fk.fork())) return rc;                 // the round's inputs are complete and A's forward pass is out
        if ((rc = issue_fwd(t, B, r, fk.st2)) ||
            (rc = issue_rest(t, A, r, st)) || (rc = issue_rest(t, B, r, fk.st2)) ||
            (rc = issue_cpp(A, r, st)) || (rc = issue_cpp(B, r, fk.st2))) return rc;
        return fk.join();                                // the next round reads both halves
    }

    int launch_tree(hipStream_t st) {
        constexpr int LANES = FS::LANES;
        int rc;
        const MsmKnobs& knobs = msm_knobs();
        const uint32_t n0 = hplan[2], maxc = hplan[4];
        TreeRun t{TreePlan(n0, p.total, maxc, DEG, 64 / LANES, (uint32_t)g.num_cus * 4u * (uint32_t)FS::WAVES,
                           (uint32_t)g.num_cus * 4u * 2u /* the assembly kernels run two waves per SIMD */, knobs)};
        const int R = t.tp.R;
        if ((rc = tree_counts(t.tp, st))) return rc;
        {
            size_t free_b = 0, total_b = 0;
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
            size_t have = 0;
            const char* names[6] = {"aff_desc", "aff_ptsA", "aff_ptsB", "aff_prefix", "aff_stage1", "aff_stage2"};
            for (const char* nm : names) have += pool_cap(slot_name(nm, slot).c_str());
            if (!t.tp.set_chunks(n0, LANES, free_b, have, knobs)) {       // no room at all: the projective kernel runs
                for (const char* nm : names) pool_release(slot_name(nm, slot).c_str());
                tree = false;
                return GH_OK;
            }
        }
        if ((rc = tree_chunk_tables(t, n0, st))) return rc;
        if ((rc = tree_lists(t))) {
            if (rc != GH_E_NOMEM) return rc;
            (void)hipGetLastError();         // the lists do not fit: the projective kernel runs
            tree = false;
            return GH_OK;
        }
        TreeLists<C>& L = t.L;
        L.rows = (const Aff<C>*)(p.merged ? h->d_table : h->d_points);
        L.sorted = sorted;
        t.aff_asm = (DEG >= 2 ? gh_asm::aff_enabled() : gh_asm::aff_g1_enabled()) && !h->aff_asm_off;
        t.asm_kind = std::is_same<C, Mnt4G2>::value ? 0 : (std::is_same<C, Mnt6G2>::value ? 1 : (std::is_same<C, Mnt6G1>::value ? 3 : 2));
        if (t.aff_asm) {
            L.accs_half = t64_bytes((size_t)t.tp.asm_max_waves + 4, T64_FP_CHUNKS);
            L.flag_words = 16 + (size_t)AFF_FIX_CAP;
            if ((rc = slot_buf("aff_accs", slot, 2 * L.accs_half, &L.asm_accs))) return rc;
            if ((rc = slot_buf("aff_flag", slot, 2 * 4 * L.flag_words, &L.asm_flag))) return rc;
            HIPCHK(hipMemsetAsync(L.asm_flag, 0, 64, st));                    // word 4: "a round of this MSM was redone" (sticky)
            HIPCHK(hipMemsetAsync(L.asm_flag + L.flag_words, 0, 64, st));
        }
        for (uint32_t j = 0; j < t.tp.K; j++) {
            size_t doff = 0;
            const void* in = nullptr;
            for (int r = 0; r < R; r++) {
                const uint32_t n_out = t.T(j + 1, r + 1) - t.T(j, r + 1);
                void* out = (r & 1) ? L.ptsB : L.ptsA;
                if (n_out > 0 && (rc = issue_round(t, j, r, n_out, in, out, L.desc + doff, st))) return rc;
                doff += n_out;
                in = out;
            }
            // what is left of the chunk's buckets (a few points each): projective, one bucket per thread / lane group
            BucketSumArgs<C> a;
            a.total = t.bq[j + 1] - t.bq[j];
            if (a.total == 0) continue;
            a.points = in; a.starts = round_starts(t, R); a.counts = round_counts(t, R);
            a.salts = salts; a.out = buckets; a.heavy_chunk = p.heavy_chunk;
            a.bucket0 = t.bq[j]; a.in_base = t.T(j, R);
            if ((rc = launch_bucket_sums<C, true>(a, std::string(), st))) return rc;
        }
        HIPCHK(hipGetLastError());
        if (t.aff_asm) {        // read with the window sums in finish(): a key that overflows the exception list leaves the assembly rounds
            HIPCHK(hipMemcpyAsync(&hplan[16], L.asm_flag + 4, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&hplan[17], L.asm_flag + L.flag_words + 4, 4, hipMemcpyDeviceToHost, st));
            aff_sticky_pending = true;
        }
        n_heavy = 0;   // no chunk sums to combine
        return GH_OK;
    }

    // one level of the bucket reduction: `grid` wave programs (msm_reduce_kernels.h) over up to three inputs.  G1: the 512-register
    // build of the program (one_wave) or the 256-register one; G2: the lane-group program.
    int reduce_level(unsigned grid, const WaveReduceIn<C>& i0, const WaveReduceIn<C>& i1, const WaveReduceIn<C>& i2, uint32_t per_input,
                     uint32_t n_inputs, uint32_t segs, int L, Proj<C>* out, uint32_t* slabs, bool one_wave, hipStream_t st,
                     const uint32_t* run_if = nullptr) {
        if constexpr (DEG >= 2) {
            GH_LAUNCH((msm_wave_reduce_split_kernel<C, FS, FS::LANES, DEG == 2 ? 32 : 16>), dim3(grid), dim3(64), 64 * sizeof(P3), st,
                      i0, i1, i2, per_input, n_inputs, segs, L, (const Aff<C>*)salts, out, slabs);
        } else if (one_wave) {
            GH_LAUNCH((msm_wave_reduce_kernel<C, 1>), dim3(grid), dim3(64), 64 * sizeof(Proj<C>), st,
                      i0, i1, i2, per_input, n_inputs, segs, L, (const Aff<C>*)salts, out, slabs, run_if);
        } else {
            GH_LAUNCH((msm_wave_reduce_kernel<C, 2>), dim3(grid), dim3(64), 64 * sizeof(Proj<C>), st,
                      i0, i1, i2, per_input, n_inputs, segs, L, (const Aff<C>*)salts, out, slabs, run_if);
        }
        return GH_OK;
    }

    // Lean level 1.  G1: the generated kernel (asmgen/g1_reduce.py: the common path of the addition, no scratch) on the 256-register
    // side, i.e. unless GH_REDUCE_WAVES=1 asks for the 512-register build of the C++ program; behind it the C++ program in its
    // 256-register build over the same programs with run_if = the generated kernel's flags: a program that met a doubling is
    // computed again, whole, from the buckets and overwrites its rows of lane_out -- the C++ kernel stays the one place that
    // knows the salt detour.
    int lean_level1(const WaveReduceIn<C>& i0, unsigned nb1, uint32_t segs, uint32_t* slabs, bool one_wave, hipStream_t st) {
        const WaveReduceIn<C> none{nullptr, 0, 0, 0, 0, 0};
        if constexpr (DEG == 1) {
            if (msm_knobs().reduce_waves != 1 && p.L1 >= 2 && red_flag && gh_asm::reduce_enabled()) {
                gh_asm::RedArgs a;
                a.items = i0.base; a.out = lane_out; a.slabs = slabs; a.flag = red_flag;
                a.count = i0.count; a.valid = i0.valid; a.segs = segs; a.L = (uint32_t)p.L1; a.n_programs = nb1; a.pad = 0;
                int rc;
                if ((rc = gh_asm::red_g1_launch(std::is_same<C, Mnt6G1>::value ? 6 : 4, a, (uint32_t)p.RW, st)) ||
                    (rc = reduce_level(nb1, i0, none, none, nb1, 1u, segs, p.L1, lane_out, slabs, false, st, red_flag))) return rc;
                if (msm_knobs().reduce_debug) {   // GH_REDUCE_DEBUG: how many programs the C++ kernel computed again
                    std::vector<uint32_t> fw(nb1);
                    HIPCHK(hipStreamSynchronize(st));
                    HIPCHK(hipMemcpy(fw.data(), red_flag, (size_t)nb1 * 4, hipMemcpyDeviceToHost));
                    unsigned redone = 0;
                    for (uint32_t v : fw) redone += v != 0;
                    fprintf(stderr, "reduce: programs %u redone %u\n", nb1, redone);
                }
                return GH_OK;
            }
        }
        return reduce_level(nb1, i0, none, none, nb1, 1u, segs, p.L1, lane_out, slabs, one_wave, st);
    }

    // stage 3 (stream st): the two wave-program levels of the bucket reduction; window sums -> host
    int launch_reduce(hipStream_t st) {
        if (n == 0) return GH_OK;
        int rc;
        const uint32_t RW = (uint32_t)p.RW, segs = p.segs_per_window, all = 0xFFFFFFFFu;
        const unsigned nb1 = RW * segs, nb2 = 3 * RW;
        const WaveReduceIn<C> none{nullptr, 0, 0, 0, 0, 0};
        // the programs' accumulators live in a slab of global memory each (msm_reduce_kernels.h, WaveSlab)
        uint32_t* slabs = nullptr;
        size_t slab_words;
        if constexpr (DEG >= 2) slab_words = WaveSlab<P3>::WORDS; else slab_words = WaveSlab<Proj<C>>::WORDS;
        if ((rc = slot_buf("reduce_slabs", slot, (size_t)(nb1 > nb2 ? nb1 : nb2) * slab_words * 4, &slabs))) return rc;
        // A stand-alone G1 MSM has the chip to itself: the 512-register build of the program (one wave per SIMD, 88 B of spills
        // per lane instead of 680) -- inside a batch the reduction must fit beside the accumulation's waves (256 registers).
        const int env_w = msm_knobs().reduce_waves;
        const bool one_wave = env_w ? env_w == 1 : solo;
        if (p.lean) {
            // level 1: serial part only, (run, wacc) per lane; level 2 per window: the weighted program over the lanes' run (item =
            // segment * 64 + lane, so its A = sum segment * run and Bv = sum lane * run) and the plain sum of their wacc
            const uint32_t lanes_per_window = segs * 64u;
            const WaveReduceIn<C> i0{buckets, 1, 0, p.Q, 2, (uint32_t)p.total};
            const WaveReduceIn<C> l0{lane_out, 2, 0, lanes_per_window, 0, all}, l1{lane_out, 2, 1, lanes_per_window, 1, all};
            if ((rc = lean_level1(i0, nb1, segs, slabs, one_wave, st)) ||
                (rc = reduce_level(2 * RW, l0, l1, none, RW, 2u, 1u, (int)segs, win_out, slabs, one_wave, st))) return rc;
        } else {
            // level 1: one wave per segment of tpw * L1 bucket slots -> (runW, A, Bv) per segment
            // level 2: one wave per window and per array: weighted program on runW, plain sums of A and Bv
            const WaveReduceIn<C> i0{buckets, 1, 0, p.Q, 0, (uint32_t)p.total};
            const WaveReduceIn<C> r0{seg_out, 3, 0, segs, 0, all}, r1{seg_out, 3, 1, segs, 1, all}, r2{seg_out, 3, 2, segs, 1, all};
            if ((rc = reduce_level(nb1, i0, none, none, nb1, 1u, segs, p.L1, seg_out, slabs, one_wave, st)) ||
                (rc = reduce_level(nb2, r0, r1, r2, RW, 3u, 1u, p.L2, win_out, slabs, one_wave, st))) return rc;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(g.pev[es][5], st));
        HIPCHK(hipMemcpyAsync(hw, win_out, (size_t)9 * RW * sizeof(Proj<C>), hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(g.pev[es][6], st));
        return GH_OK;
    }

    // stage 4 (host): wait for the window sums, fold (msm_fold.h)
    int finish() {
        if (n == 0) {
            proj_to_abi_host<C>(out_xyz, proj_zero<C>());
            g.last_msm = gh_msm_timing_t{};
            g.batch_tm.push_back(g.last_msm);
            return GH_OK;
        }
        HIPCHK(hipEventSynchronize(g.pev[es][6]));
        if (aff_sticky_pending && (hplan[16] != 0 || hplan[17] != 0)) h->aff_asm_off = 1;
        auto t_fold0 = std::chrono::steady_clock::now();
        auto hwv = to_host_curve<C>(hw, (size_t)9 * p.RW);
        if (p.lean) lean_reslot(hwv, p.RW);
        const int u = fold_u(p.sw, p.L1);
        if (p.merged) fold_merged<C>(hwv, p.RW, fold_lq(p.Q), u, p.sw, p.sets, p.c, out_xyz);
        else fold_windows<C>(hwv, p.W, p.c, u, p.sw, p.top_unsigned, out_xyz);
        auto t_end = std::chrono::steady_clock::now();
        HIPCHK(hipEventElapsedTime(&tm.sort_ms, g.pev[es][0], g.pev[es][1]));
        HIPCHK(hipEventElapsedTime(&tm.accumulate_ms, g.pev[es][2], g.pev[es][3]));   // brackets exactly the accumulation launch
        HIPCHK(hipEventElapsedTime(&tm.heavy_ms, g.pev[es][3], g.pev[es][4]));
        HIPCHK(hipEventElapsedTime(&tm.reduce_ms, g.pev[es][4], g.pev[es][5]));
        tm.heavy_buckets = n_heavy;
        tm.fold_ms = std::chrono::duration<float, std::milli>(t_end - t_fold0).count();
        tm.total_ms = std::chrono::duration<float, std::milli>(t_end - t_begin).count();
        tm.window_bits = p.c;
        tm.num_windows = p.W;
        g.last_msm = tm;
        g.batch_tm.push_back(tm);
        return GH_OK;
    }
};

// The accumulation kernels over caller-made lists (fixed_base.hip: one "bucket" per scalar, its list the table entries its
// digits select): out[g] = sum of points[sorted[starts[g] + k] & 0x7FFFFFFF] (bit 31: negated), k < counts[g], for the
// `total` lists in the order `order` names them; no heavy-bucket chunks.  Same kernels, same complete addition (doubling through
// the salt detour, P + (-P), infinity) as the MSM's projective path.
template <class C>
int accumulate_lists(const void* points, const uint32_t* sorted, const uint32_t* starts, const uint32_t* counts,
                     const uint32_t* order, uint32_t total, void* out_proj, hipStream_t st) {
    if (total == 0) return GH_OK;
    Aff<C>* salts = nullptr;
    if (int rc = device_salts<C>(&salts)) return rc;
    BucketSumArgs<C> a;
    a.salts = salts; a.points = points; a.sorted = sorted; a.starts = starts; a.counts = counts; a.order = order; a.total = total;
    a.out = (Proj<C>*)out_proj;
    if (int rc = launch_bucket_sums<C, false>(a, "acc_tasks#lists", st)) return rc;
    HIPCHK(hipGetLastError());
    return GH_OK;
}

// `count` MSMs back to back.  With count > 1 the stages are pipelined over three streams and two
// buffer slots: while MSM k accumulates (stream_acc), the bucket sort of MSM k+1 (g.stream) and the
// bucket reduction + host fold of MSM k-1 (stream_red, host) run beside it -- the sort is
// atomics/memory bound and the reduction's wave programs are latency chains, so both fit into the
// issue slots the accumulation leaves.  Slot reuse is ordered by events (one event set per job in flight, g.pev[k & 3]):
//   sort(k+1) waits for acc(k-1) (lists of that slot), acc(k+1) for reduce(k-1) (its buckets).
// Not free: leaving the reduction out of a batch (measurement only) takes the 2^20-pair G1 MSM from 23.4 to 20.1 ms -- the
// reduction's instructions are issued at the accumulation's expense.  Hence the lean form of the reduction for the MSMs
// of a batch that have a successor to hide its longer chain behind (MsmJob::prepare).
template <class C>
int msm_batch(BasesBase* const* hs, const void* const* d_scalars, const size_t* n_scalars, int count, uint64_t* out_xyz) {
    const size_t out_stride = (size_t)36 * C::F::DEG;
    std::vector<MsmJob<C>> jobs((size_t)count);
    int rc;
    auto issue_sort = [&](int k) -> int {
        MsmJob<C>& j = jobs[(size_t)k];
        j.solo = count == 1;
        j.last = k == count - 1;
        j.es = k & 3;
        if ((rc = j.prepare(hs[k], d_scalars[k], n_scalars[k], out_xyz + (size_t)k * out_stride, k & 1))) return rc;
        if (k >= 2) {
            HIPCHK(hipStreamWaitEvent(g.stream, g.pev[(k - 2) & 3][4], 0));   // acc(k-2) has consumed this slot's lists
        }
        return j.launch_sort(g.stream);
    };
    g.batch_tm.clear();
    if (count <= 0) return GH_OK;
    if ((rc = issue_sort(0))) return rc;
    for (int k = 0; k < count; k++) {
        MsmJob<C>& j = jobs[(size_t)k];
        // GH_ACC_ALT (G1, persistent form): the odd jobs accumulate on a stream of their own, so that acc(k+1) no longer queues behind the last
        // wave of acc(k) -- its workgroups take the slots acc(k)'s waves leave.  Stream and buffer slot alternate together (k & 1),
        // so acc(k) still follows acc(k-2), the previous occupant of its slot, in stream order; it waits for its own sort on the
        // host (launch_accumulate) and for reduce(k-2) by event, as before.  Every cleanup path waits for the stream with the
        // others (runtime.h sync_msm_streams).
        const bool alt = C::F::DEG == 1 && g.stream_acc_alt && gh_asm::enabled() && msm_knobs().acc_persist && (k & 1);
        const hipStream_t st_acc = alt ? g.stream_acc_alt : g.stream_acc;
        if (k >= 2 && j.n) HIPCHK(hipStreamWaitEvent(st_acc, g.pev[(k - 2) & 3][6], 0));   // reduce(k-2) is done with this slot's buckets
        if ((rc = j.launch_accumulate(st_acc))) return rc;
        if (j.n) HIPCHK(hipStreamWaitEvent(g.stream_red, g.pev[k & 3][4], 0));
        if ((rc = j.launch_reduce(g.stream_red))) return rc;
        // sort(k+1) goes out before the host waits for the window sums of k-1: the two share a buffer slot but no buffer
        // (lists and plan of the slot were consumed by acc(k-1); buckets, segment sums and the pinned window sums are the
        // reduction's) and, since round 3, no events -- so the sort of the next MSM no longer starts only when the
        // reduction of the previous one has ended (11 ms into acc(k), more with the lean reduction's longer chain).
        if (k + 1 < count && (rc = issue_sort(k + 1))) return rc;
        if (k >= 1 && (rc = jobs[(size_t)k - 1].finish())) return rc;
    }
    return jobs[(size_t)count - 1].finish();
}

template <class C>
int msm_run(BasesBase* h, const void* d_scalars, size_t n_scalars, uint64_t* out_xyz) {
    return msm_batch<C>(&h, &d_scalars, &n_scalars, 1, out_xyz);
}

template <class C>
int msm_host(const uint64_t* bases, const uint8_t* infinity, size_t n_bases, const uint64_t* scalars, size_t n_scalars,
             uint64_t* out_xyz) {
    size_t n = n_bases < n_scalars ? n_bases : n_scalars;
    BasesBase* uploaded = nullptr;
    int rc = upload_bases<C>(bases, infinity, n, 0, &uploaded);
    if (rc) return rc;
    const std::unique_ptr<BasesBase> h(uploaded);      // the key of this one call
    void* d_s = nullptr;
    if (n > 0) {
        if ((rc = pool_get("scalars", n * 96, &d_s))) return rc;
        hipError_t e = hipMemcpyAsync(d_s, scalars, n * 96, hipMemcpyHostToDevice, g.stream);
        if (e != hipSuccess) { g_err = hipGetErrorString(e); return GH_E_HIP; }
    }
    return msm_run<C>(h.get(), d_s, n, out_xyz);
}


#define GH_DEFINE_MSM_OPS(CURVE, NAME)                                                        \
    namespace gh_rt {                                                                          \
    const MsmOps* NAME() {                                                                     \
        static const MsmOps ops = {&upload_bases<CURVE>, &msm_run<CURVE>, &msm_host<CURVE>,    \
                                   &proj_add_host<CURVE>, &to_affine_host<CURVE>,              \
                                   &precompute_bases<CURVE>, &msm_batch<CURVE>,                \
                                   &proj_mul_host<CURVE>, &proj_neg_host<CURVE>, &accumulate_lists<CURVE>};           \
        return &ops;                                                                           \
    }                                                                                          \
    }

}  // namespace gh_rt
