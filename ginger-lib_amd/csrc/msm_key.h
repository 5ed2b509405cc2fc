// msm_key.h -- a resident key of the MSM: upload of the bases, the precomputed shift table, the groups of equal bases.
// Included by msm_impl.h (one instance per curve).
#pragma once
#include <algorithm>
#include <memory>
#include <vector>
#include "runtime.h"
#include "msm_kernels.h"

namespace gh_rt {
using namespace gh;

template <class C>
int upload_bases(const uint64_t* bases, const uint8_t* infinity, size_t n, int canonical, BasesBase** out) {
    typedef typename C::F F;
    std::unique_ptr<BasesBase> h(new BasesBase());     // an early return frees the key and what it holds by then
    h->curve = CurveId<C>::id;
    h->n = n;
    if (n > 0) {
        const size_t in_bytes = n * (size_t)(48 * F::DEG) * 4;
        DevMem points, d_in, inf;
        int rc;
        if ((rc = points.alloc(n * sizeof(Aff<C>))) || (rc = d_in.alloc(in_bytes))) return rc;
        h->d_points = points.release();
        HIPCHK(hipMemcpyAsync(d_in.get(), bases, in_bytes, hipMemcpyHostToDevice, g.stream));
        GH_LAUNCH((msm_convert_bases_kernel<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g.stream,
                           d_in.as<const uint32_t>(), (Aff<C>*)h->d_points, n, canonical);
        HIPCHK(hipGetLastError());
        if (infinity) {
            bool any = false;
            for (size_t i = 0; i < n && !any; i++) any = infinity[i] != 0;
            if (any) {
                if ((rc = inf.alloc(n))) return rc;
                h->d_inf = (uint8_t*)inf.release();
                HIPCHK(hipMemcpyAsync(h->d_inf, infinity, n, hipMemcpyHostToDevice, g.stream));
            }
        }
        HIPCHK(hipStreamSynchronize(g.stream));
    }
    *out = h.release();
    return GH_OK;
}

// Groups of equal bases (msm_kernels.h "equal bases"): hashed on the device, grouped on the host, verified limb for limb on the
// device.  Optional: any failure leaves the key without groups (every base its own) and the caller ignores the status.  Called
// when the shift table is built -- a key that gets a table is a key that is used again.  GH_DEDUP=0 switches it off (A/B).
template <class C>
int dedup_bases(BasesBase* h) {
    dev_free(h->d_dup_starts);
    dev_free(h->d_dup_members);
    dev_free(h->d_dup_chunks);
    h->n_dup_groups = h->n_dup_members = h->n_dup_chunks = 0;
    const size_t n = h->n;
    if (msm_knobs().dedup == 0 || !g.dedup_mode || n < 2 || n >= ((size_t)1 << 31)) return GH_OK;
    hipStream_t st = g.stream;
    uint64_t* d_hash = nullptr;
    int rc;
    if ((rc = pool_get("dedup_hash", n * 16, (void**)&d_hash))) return rc;
    GH_LAUNCH((msm_base_hash_kernel<C>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const Aff<C>*)h->d_points, (const uint8_t*)h->d_inf, n, d_hash);
    std::vector<uint64_t> hh(2 * n);
    HIPCHK(hipMemcpyAsync(hh.data(), d_hash, n * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // group by hash: indices sorted by (h1, h2, index); runs of equal hashes with at least two members are groups
    std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        if (hh[2 * (size_t)a] != hh[2 * (size_t)b]) return hh[2 * (size_t)a] < hh[2 * (size_t)b];
        if (hh[2 * (size_t)a + 1] != hh[2 * (size_t)b + 1]) return hh[2 * (size_t)a + 1] < hh[2 * (size_t)b + 1];
        return a < b;
    });
    std::vector<uint32_t> starts, members;
    for (size_t i = 0; i < n;) {
        size_t j = i + 1;
        const uint64_t a1 = hh[2 * (size_t)idx[i]], a2 = hh[2 * (size_t)idx[i] + 1];
        while (j < n && hh[2 * (size_t)idx[j]] == a1 && hh[2 * (size_t)idx[j] + 1] == a2) j++;
        if (j - i >= 2 && !(a1 == 0 && a2 == 0)) {            // (0, 0): infinity bases -- the digits stage skips them anyway
            starts.push_back((uint32_t)members.size());
            for (size_t k = i; k < j; k++) members.push_back(idx[k]);      // ascending: the canonical base is the smallest index
        }
        i = j;
    }
    if (starts.empty()) return GH_OK;
    starts.push_back((uint32_t)members.size());
    DevMem d_st, d_mem, d_ch;          // become the key's lists at the very end; any return before that frees them
    uint8_t* d_flags = nullptr;
    if ((rc = d_st.alloc(starts.size() * 4)) || (rc = d_mem.alloc(members.size() * 4)) ||
        (rc = pool_get("dedup_flags", members.size() + 16, (void**)&d_flags))) return rc;
    const uint32_t ng = (uint32_t)starts.size() - 1;
    HIPCHK(hipMemcpyAsync(d_st.get(), starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_mem.get(), members.data(), members.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_flags, 0, members.size(), st));
    hipLaunchKernelGGL((msm_dup_verify_kernel<C>), dim3(ng), dim3(256), 0, st, (const Aff<C>*)h->d_points, d_st.as<const uint32_t>(), ng,
                       d_mem.as<uint32_t>(), d_flags);
    HIPCHK(hipGetLastError());
    std::vector<uint8_t> flags(members.size());
    HIPCHK(hipMemcpyAsync(flags.data(), d_flags, members.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(members.data(), d_mem.get(), members.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool collision = false;
    for (uint8_t f : flags) collision |= f != 0;
    if (collision) {      // equal 128-bit hashes over different abscissae: drop those members and rebuild the lists
        std::vector<uint32_t> st2, mem2;
        for (uint32_t gi = 0; gi < ng; gi++) {
            const size_t b0 = mem2.size();
            for (uint32_t j = starts[gi]; j < starts[gi + 1]; j++) if (!flags[j]) mem2.push_back(members[j]);
            if (mem2.size() - b0 >= 2) st2.push_back((uint32_t)b0); else mem2.resize(b0);
        }
        if (st2.empty()) return GH_OK;
        st2.push_back((uint32_t)mem2.size());
        if ((rc = d_st.alloc(st2.size() * 4)) || (rc = d_mem.alloc(mem2.size() * 4))) return rc;
        HIPCHK(hipMemcpy(d_st.get(), st2.data(), st2.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_mem.get(), mem2.data(), mem2.size() * 4, hipMemcpyHostToDevice));
        starts.swap(st2); members.swap(mem2);
    }
    // chunks of at most MSM_DUP_CHUNK members for the summation (msm_merge_scalars_kernel), then the chunk offsets per group
    const uint32_t ngf = (uint32_t)starts.size() - 1;
    std::vector<uint32_t> ch, goff(ngf + 1);
    for (uint32_t gi = 0; gi < ngf; gi++) {
        goff[gi] = (uint32_t)(ch.size() / 3);
        for (uint32_t lo = starts[gi]; lo < starts[gi + 1]; lo += MSM_DUP_CHUNK) {
            const uint32_t hi = starts[gi + 1] - lo > MSM_DUP_CHUNK ? lo + MSM_DUP_CHUNK : starts[gi + 1];
            ch.push_back(lo); ch.push_back(hi); ch.push_back(gi);
        }
    }
    goff[ngf] = (uint32_t)(ch.size() / 3);
    const uint32_t nch = goff[ngf];
    ch.insert(ch.end(), goff.begin(), goff.end());
    if ((rc = d_ch.alloc(ch.size() * 4))) return rc;
    HIPCHK(hipMemcpy(d_ch.get(), ch.data(), ch.size() * 4, hipMemcpyHostToDevice));
    h->d_dup_starts = (uint32_t*)d_st.release();
    h->d_dup_members = (uint32_t*)d_mem.release();
    h->d_dup_chunks = (uint32_t*)d_ch.release();
    h->n_dup_groups = ngf;
    h->n_dup_members = (uint32_t)members.size();
    h->n_dup_chunks = nch;
    return GH_OK;
}

// Precomputed shift table for a resident key (msm_kernels.h section 0): rows w = 0 .. W-1 of
// 2^(c w) P_i.  c == 0 picks the window from n.  The table costs W x the bases' footprint
// (n = 2^20 G1, c = 21: 36 x 218 MB = 7.8 GB of the 288 GB), built once per key in slabs.
template <class C>
int precompute_bases(BasesBase* h, int c_req, int max_rows) {
    typedef typename C::FC::T FT;
    dev_free(h->d_table);
    h->pre_c = h->pre_W = 0;
    h->pre_G = 1;
    const size_t n = h->n;
    if (n == 0) return GH_OK;
    // Partial table (max_rows > 0, or GH_TABLE_ROWS for every table of the process): at most that many rows, row j = 2^(c G j) P with
    // G = ceil(windows / max_rows) bucket sets -- window w = j G + g reads row j and files into set g; the G set sums are
    // folded with c doublings each (finish()).  For keys whose full table does not fit next to the others (four 2^24-base
    // G1 queries: 4 x 126 GB at c = 21): 8 rows are 28 GB.  A capped table keeps its sets at 2^20 buckets (c = 21) where the
    // full table of a large key would take c = 23: the sets multiply the bucket reduction.
    const int env_rows = env_int("GH_TABLE_ROWS", 0);          // read on every call, not once per process like MsmKnobs
    const int cap = max_rows > 0 ? max_rows : env_rows;
    int c = c_req > 0 ? c_req : precompute_window(n, C::F::DEG, g.window_override);
    if (c_req <= 0 && cap > 0 && cap < 752 / c + 1 && c > 21) c = 21;
    if (c < 2 || c > 24) { g_err = "precompute window must be in [2, 24]"; return GH_E_BAD_ARG; }
    const int windows = 752 / c + 1;
    const int G = cap > 0 && cap < windows ? (windows + cap - 1) / cap : 1;
    const int W = (windows + G - 1) / G;          // rows of the table
    const int c_row = c * G;                      // doublings from one row to the next
    if ((size_t)W * n >= ((size_t)1 << 31)) { g_err = "precomputed table too large for 31-bit entries"; return GH_E_UNSUPPORTED; }
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t slab = n < ((size_t)1 << 20) ? n : ((size_t)1 << 20);
    const size_t need = (size_t)W * n * sizeof(Aff<C>) + 2 * (size_t)(W - 1) * slab * sizeof(FT) + ((size_t)1 << 30);
    if (need > free_b) {   // the scratch caches of earlier calls (bucket lists, affine-round lists) are only caches: drop them
        HIPCHK(sync_msm_streams());
        pool_release("");
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
    }
    if (need > free_b) { g_err = "not enough device memory for the precomputed table"; return GH_E_NOMEM; }
    if (env_int("GH_TEST_TABLE_NOMEM", 0) != 0) {
        // (read on every call: tests/test_gpu_parity.py sets it in the middle of a process)
        // fault injection (include/ginger_hip.h gh_test_hooks): the path a table build takes when the card is full -- every pooled
        // scratch buffer is dropped, the key stays on the per-window path.  tests/test_gpu_parity.py runs gh_msm_cached through it
        // on every GPU run (the round-3 fault: a pooled scalar buffer freed here under a running copy).
        HIPCHK(sync_msm_streams());
        pool_release("");
        g_err = "not enough device memory for the precomputed table (GH_TEST_TABLE_NOMEM)";
        return GH_E_NOMEM;
    }
    DevMem table_mem;                 // becomes h->d_table once every row is built
    FT *zs = nullptr, *zp = nullptr;
    uint32_t* bad = nullptr;
    int rc;
    if ((rc = table_mem.alloc((size_t)W * n * sizeof(Aff<C>))) ||
        (rc = pool_get("pre_zs", (size_t)(W - 1) * slab * sizeof(FT) + 8, (void**)&zs)) ||
        (rc = pool_get("pre_zp", (size_t)(W - 1) * slab * sizeof(FT) + 8, (void**)&zp)) ||
        (rc = pool_get("pre_bad", 16, (void**)&bad))) return rc;
    Aff<C>* const table = table_mem.as<Aff<C>>();
    hipStream_t st = g.stream;
    hipError_t e = hipMemcpyAsync(table, h->d_points, n * sizeof(Aff<C>), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 4, st);
    for (size_t i0 = 0; i0 < n && e == hipSuccess; i0 += slab) {
        const size_t cnt = n - i0 < slab ? n - i0 : slab;
        {   // the table builders carry 2-9 KB of stack per lane: no dispatch the card cannot back with scratch (runtime.h scratch_guard)
            const void* kfn = C::F::DEG == 1 ? (const void*)(msm_precompute_jac_kernel<C, typename C::F>)
                                             : (const void*)(msm_precompute_jac_kernel<C, typename C::FC>);
            if (int grc = scratch_guard(kfn, (cnt + 255) / 256 * 256)) return grc;
        }
        if constexpr (C::F::DEG == 1)
            hipLaunchKernelGGL((msm_precompute_jac_kernel<C, typename C::F>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st,
                               table, (const uint8_t*)h->d_inf, n, i0, cnt, slab, c_row, W, zs, zp, bad);
        else
            hipLaunchKernelGGL((msm_precompute_jac_kernel<C, typename C::FC>), dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, st,
                               table, (const uint8_t*)h->d_inf, n, i0, cnt, slab, c_row, W, zs, zp, bad);
        e = hipGetLastError();
    }
    uint32_t hbad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { g_err = std::string("precompute failed: ") + hipGetErrorString(e); return GH_E_HIP; }
    if (hbad) {   // a base of 2-power order: 2^(c w) P hits infinity, which an affine table cannot hold
        g_err = "precompute: a base has 2-power order; the key stays on the per-window path";
        return GH_E_UNSUPPORTED;
    }
    h->d_table = table_mem.release();
    h->pre_c = c;
    h->pre_W = W;
    h->pre_G = G;
    // equal bases of the key: their scalars are added up before every MSM (optional: a failure leaves none, and no pending HIP error)
    if (dedup_bases<C>(h)) (void)hipGetLastError();
    return GH_OK;
}

}  // namespace gh_rt
