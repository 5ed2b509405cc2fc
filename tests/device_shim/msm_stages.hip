// msm_stages.hip -- the integer kernels of the MSM's sort stage (ginger-lib_amd/csrc/msm_kernels.h, scan_kernels.h), one host
// launcher per kernel, so that every array the point kernels later dereference -- digits, counts, starts, sorted, order,
// chunk_start, the task table, the equal-bases lists -- can be read back and compared with a Python-integer model before any
// point kernel sees it (tests/test_gpu_msm_stages.py, tests/msm_sort_ref.py).
// Test infrastructure: built by the test into build/libmsm_stages.so (hipcc -shared), never linked into the product, no ABI.
// Most of these kernels are `static __global__`: a code object would drop them, a host launcher keeps them.
//
// Every launcher takes plain values and device pointers, launches on the null stream with the grid and block shape the product
// uses (msm_impl.h launch_sort / sort_partitioned / merge_equal_bases / the task table's launch, msm_key.h dedup_bases,
// ginger_hip.hip device_scan), synchronises and returns the hipError_t.  Moduli are 24 host words.  `curve`: 0 = Mnt4G1
// (one-field-element coordinates), 1 = Mnt4G2 (two).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../ginger-lib_amd/csrc/msm_kernels.h"
#include "../../ginger-lib_amd/csrc/scan_kernels.h"

using namespace gh;

static int finish() {
    hipError_t e = hipGetLastError();
    const hipError_t s = hipDeviceSynchronize();
    if (e == hipSuccess) e = s;
    return (int)e;
}
static MsmModulus modulus(const uint32_t* r) {
    MsmModulus m;
    memcpy(m.w, r, sizeof m.w);
    return m;
}
static MsmPartArgs part_args(const int32_t* digits, size_t n, uint32_t W, uint32_t win_stride, uint32_t row_stride, uint32_t slot_shift,
                             uint32_t sets, uint32_t bin_shift, uint32_t n_bins, uint32_t tile) {
    MsmPartArgs a;
    a.digits = digits; a.entries = (size_t)W * n; a.n = n;
    a.win_stride = win_stride; a.row_stride = row_stride; a.slot_shift = slot_shift; a.sets = sets;
    a.bin_shift = bin_shift; a.n_bins = n_bins; a.tile = tile;
    a.n_blocks = (uint32_t)((a.entries + tile - 1) / tile);
    return a;
}

extern "C" {

// what the model has to know of the point types: which 0 = sizeof(Aff<C>), 1 = sizeof(Proj<C>), 2 = sizeof(AccTaskRec)
uint32_t st_sizeof(int curve, int which) {
    if (which == 2) return (uint32_t)sizeof(AccTaskRec);
    if (curve == 0) return (uint32_t)(which ? sizeof(Proj<Mnt4G1>) : sizeof(Aff<Mnt4G1>));
    return (uint32_t)(which ? sizeof(Proj<Mnt4G2>) : sizeof(Aff<Mnt4G2>));
}

int st_digits(const uint32_t* scalars, const uint8_t* infinity, uint64_t n, int c, int W, uint32_t win_stride, int top_unsigned,
              const uint32_t* r, int32_t* digits, uint32_t* counts, int agg_iters, uint32_t slot_shift, uint32_t sets) {
    msm_digits_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(scalars, infinity, (size_t)n, c, W, win_stride, top_unsigned,
                                                                        modulus(r), digits, counts, agg_iters, slot_shift, sets);
    return finish();
}

// the three kernels of device_scan; sums: (n + 2047) / 2048 + 1 words of scratch
int st_scan(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* sums) {
    const size_t per_block = (size_t)SCAN_BLOCK * SCAN_ITEMS;
    const size_t nblocks = ((size_t)n + per_block - 1) / per_block;
    scan_partials_kernel<<<dim3((unsigned)nblocks), dim3(SCAN_BLOCK)>>>(in, sums, (size_t)n);
    scan_block_sums_kernel<<<dim3(1), dim3(1024)>>>(sums, nblocks);
    scan_final_kernel<<<dim3((unsigned)nblocks), dim3(SCAN_BLOCK)>>>(in, sums, out, (size_t)n);
    return finish();
}

int st_scatter(const int32_t* digits, uint64_t n, int W, uint32_t win_stride, uint32_t row_stride, uint32_t* cursor, uint32_t* sorted,
               int agg_iters, uint32_t slot_shift, uint32_t sets) {
    msm_scatter_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)W), dim3(256)>>>(digits, (size_t)n, W, win_stride, row_stride, cursor,
                                                                                    sorted, agg_iters, slot_shift, sets);
    return finish();
}

// block_hist / block_off: n_bins * n_blocks + 1 words, n_blocks = ceil(W n / tile)
int st_part_hist(const int32_t* digits, uint64_t n, uint32_t W, uint32_t win_stride, uint32_t row_stride, uint32_t slot_shift,
                 uint32_t sets, uint32_t bin_shift, uint32_t n_bins, uint32_t tile, uint32_t* block_hist) {
    const MsmPartArgs a = part_args(digits, (size_t)n, W, win_stride, row_stride, slot_shift, sets, bin_shift, n_bins, tile);
    msm_part_hist_kernel<<<dim3(a.n_blocks), dim3(MSM_PART_THREADS)>>>(a, block_hist);
    return finish();
}
int st_part_scatter(const int32_t* digits, uint64_t n, uint32_t W, uint32_t win_stride, uint32_t row_stride, uint32_t slot_shift,
                    uint32_t sets, uint32_t bin_shift, uint32_t n_bins, uint32_t tile, const uint32_t* block_off, uint32_t* part) {
    const MsmPartArgs a = part_args(digits, (size_t)n, W, win_stride, row_stride, slot_shift, sets, bin_shift, n_bins, tile);
    msm_part_scatter_kernel<<<dim3(a.n_blocks), dim3(MSM_PART_THREADS)>>>(a, block_off, reinterpret_cast<uint2*>(part));
    return finish();
}
int st_bin_sort(const uint32_t* part, const uint32_t* block_off, uint32_t n_blocks, uint32_t bin_shift, uint32_t n_bins, uint32_t total,
                uint32_t* counts, uint32_t* starts, uint32_t* sorted) {
    msm_bin_sort_kernel<<<dim3(n_bins), dim3(MSM_BIN_THREADS), (size_t)4 << bin_shift>>>(reinterpret_cast<const uint2*>(part), block_off,
                                                                                        n_blocks, bin_shift, total, counts, starts, sorted);
    return finish();
}

int st_size_hist(const uint32_t* counts, uint64_t total, uint32_t heavy_thr, uint32_t* size_hist, uint32_t* max_count) {
    msm_size_hist_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256)>>>(counts, (size_t)total, heavy_thr, size_hist, max_count);
    return finish();
}
int st_size_scatter(const uint32_t* counts, uint64_t total, uint32_t heavy_thr, uint32_t* size_cursor, uint32_t* order) {
    msm_size_scatter_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256)>>>(counts, (size_t)total, heavy_thr, size_cursor, order);
    return finish();
}
int st_heavy_plan(const uint32_t* size_hist, const uint32_t* counts, const uint32_t* order, const uint32_t* starts, uint32_t total,
                  uint32_t chunk, uint32_t* chunk_start, uint32_t* plan) {
    msm_heavy_plan_kernel<<<dim3(1), dim3(1)>>>(size_hist, counts, order, starts, total, chunk, chunk_start, plan);
    return finish();
}

// buckets / partials are addresses only: the kernel forms dst from them and never dereferences either
int st_acc_tasks(int curve, const uint32_t* starts, const uint32_t* counts, const uint32_t* order, uint32_t total, uint64_t buckets,
                 const uint32_t* chunk_start, uint32_t n_heavy, uint32_t n_chunks, uint32_t chunk, uint64_t partials, void* out,
                 uint32_t* tile_counter) {
    const uint32_t tasks = n_chunks + (total - n_heavy);
    const dim3 grid((tasks + 255) / 256), block(256);
    if (curve == 0)
        msm_acc_tasks_kernel<Mnt4G1><<<grid, block>>>(starts, counts, order, total, (Proj<Mnt4G1>*)(uintptr_t)buckets, chunk_start, n_heavy,
                                                      n_chunks, chunk, (Proj<Mnt4G1>*)(uintptr_t)partials, (AccTaskRec*)out, tile_counter);
    else
        msm_acc_tasks_kernel<Mnt4G2><<<grid, block>>>(starts, counts, order, total, (Proj<Mnt4G2>*)(uintptr_t)buckets, chunk_start, n_heavy,
                                                      n_chunks, chunk, (Proj<Mnt4G2>*)(uintptr_t)partials, (AccTaskRec*)out, tile_counter);
    return finish();
}

int st_base_hash(int curve, const void* pts, const uint8_t* inf, uint64_t n, uint64_t* out) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (curve == 0) msm_base_hash_kernel<Mnt4G1><<<grid, block>>>((const Aff<Mnt4G1>*)pts, inf, (size_t)n, out);
    else msm_base_hash_kernel<Mnt4G2><<<grid, block>>>((const Aff<Mnt4G2>*)pts, inf, (size_t)n, out);
    return finish();
}
int st_dup_verify(int curve, const void* pts, const uint32_t* starts, uint32_t n_groups, uint32_t* members, uint8_t* flags) {
    if (curve == 0) msm_dup_verify_kernel<Mnt4G1><<<dim3(n_groups), dim3(256)>>>((const Aff<Mnt4G1>*)pts, starts, n_groups, members, flags);
    else msm_dup_verify_kernel<Mnt4G2><<<dim3(n_groups), dim3(256)>>>((const Aff<Mnt4G2>*)pts, starts, n_groups, members, flags);
    return finish();
}
int st_merge_scalars(const uint32_t* in, uint32_t* out, uint64_t n, const uint32_t* starts, const uint32_t* members, const uint32_t* chunks,
                     uint32_t n_chunks, uint32_t* partial, const uint32_t* r) {
    msm_merge_scalars_kernel<<<dim3(n_chunks), dim3(256)>>>(in, out, (size_t)n, starts, members, chunks, n_chunks, partial, modulus(r));
    return finish();
}
int st_merge_groups(uint32_t* out, uint64_t n, const uint32_t* starts, const uint32_t* members, const uint32_t* gchunk, uint32_t n_groups,
                    const uint32_t* partial, const uint32_t* r) {
    msm_merge_groups_kernel<<<dim3((n_groups + 63) / 64), dim3(64)>>>(out, (size_t)n, starts, members, gchunk, n_groups, partial, modulus(r));
    return finish();
}

}  // extern "C"
