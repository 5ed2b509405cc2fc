// runtime.h -- process-wide device context shared by the translation units of libginger_hip.so
// (one TU per curve so that hipcc can build them in parallel; see __graft_entry__.py build()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/ginger_hip.h"
#include "fp29.h"
#include "msm_plan.h"

struct gh_poseidon;
namespace gh { struct Mnt4G1; struct Mnt4G2; struct Mnt6G1; struct Mnt6G2; }   // the curve policies (ec29.h)

namespace gh_rt {

// hipFree of a device pointer held in a struct, which is left null.  hipFree waits for the device first.
template <class T> void dev_free(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

struct Domain {
    int log_n = 0;
    gh::Fp* tw = nullptr;          // w^i
    gh::Fp* coset = nullptr;       // g^i
    gh::Fp* coset_inv = nullptr;   // size_inv * g^-i
    gh::Fp size_inv;               // internal form
    gh::Fp* d_size_inv = nullptr;  // the same on the device (the assembly pass reads its final factor from memory)
    uint32_t* scratch = nullptr;
    uint32_t* scratch2 = nullptr;  // second ping-pong vector: an odd number of passes ends in the caller's buffer without a copy
    bool scratch2_failed = false;
    // A Domain lives inside the static context, so it holds raw pointers and is released by gh_shutdown, never by a destructor
    // (which would run after the HIP runtime is gone).  Builders fill it from local DevMem owners on success only (ntt.hip).
    void release() { dev_free(tw); dev_free(coset); dev_free(coset_inv); dev_free(d_size_inv); dev_free(scratch); dev_free(scratch2); }
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct Ctx {
    bool ready = false;
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;       // transforms, bucket sort
    hipStream_t stream_acc = nullptr;   // MSM accumulation (lowest priority: the filler of the pipeline)
    hipStream_t stream_red = nullptr;   // MSM bucket reduction (highest priority: short latency chains)
    hipStream_t stream_acc2 = nullptr;  // second half of a split affine round (msm_impl.h issue_round): same priority as stream_acc
    hipStream_t stream_acc_alt = nullptr;   // the accumulations of the odd jobs of a G1 batch (msm_impl.h msm_batch); null under GH_ACC_ALT=0
    hipEvent_t tev[2] = {nullptr, nullptr};   // fork / join of a split round
    hipEvent_t pev[4][8];               // MSM stage events, one set per job in flight (job k of a batch uses set k & 3)
    std::map<int, Domain> domains[2];
    std::map<std::string, DevBuf> pool;
    int window_override = 0;
    int affine_mode = 2;        // G1 bucket sums by affine rounds (aff_kernels.h): 0 never, 1 always, 2 when the list fills the chip
    gh_msm_timing_t last_msm{};
    std::vector<gh_msm_timing_t> batch_tm;   // per-MSM timings of the last batch call
    float last_fft_ms = 0;
    int dedup_mode = 1;                 // gh_msm_set_dedup: add up the scalars of equal bases (keys with a shift table)
    size_t scratch_reserved = 0;        // scratch_guard(): stack-frame scratch the runtime already holds for this context's queues
    std::vector<std::function<void()>> at_shutdown;   // releases of function-local device / pinned allocations
};

extern Ctx g;
extern std::string g_err;

int ensure_init();
std::mutex& api_mutex();     // the lock every ABI entry point holds (one device context per process)
int pool_get(const char* name, size_t bytes, void** out);
size_t pool_cap(const char* name);                 // current capacity of a cached buffer (0 if none)
void pool_release(const char* prefix);             // free every cached buffer whose name starts with prefix ("" = all)
// Free every cached buffer whose name starts with prefix and whose capacity is above keep_bytes; the others stay.  Waits for
// g.stream before the first free: the caller may be on an error return with kernels in flight.
void pool_trim(const char* prefix, size_t keep_bytes);
constexpr size_t SLAB_KEEP_BYTES = (size_t)64 << 20;   // what Poseidon, Schnorr and EC-VRF entry points trim their buffers to on return
// the cached buffer `name` of one MSM buffer slot: pool name "name#slot"
inline std::string slot_name(const char* name, int slot) { return std::string(name) + "#" + std::to_string(slot); }
template <class T> int slot_buf(const char* name, int slot, size_t bytes, T** out) {
    return pool_get(slot_name(name, slot).c_str(), bytes, (void**)out);
}
// (env_int / env_double, the readers of an environment knob: msm_plan.h)
// Waits for every stream an MSM runs on, the second stream of a split affine round and the alternate accumulation stream
// included: nothing may still read or write a pooled buffer or a cached key when it is released.  Waits on all of them even
// after an error; returns the first error.
inline hipError_t sync_msm_streams() {
    hipError_t e = hipSuccess;
    for (hipStream_t s : {g.stream, g.stream_acc, g.stream_acc2, g.stream_acc_alt, g.stream_red}) {
        if (!s) continue;
        const hipError_t es = hipStreamSynchronize(s);
        if (e == hipSuccess) e = es;
    }
    return e;
}
int device_scan(const uint32_t* in, uint32_t* out, size_t n, const char* tmpname, hipStream_t stream = nullptr);   // nullptr: g.stream
inline int auto_window(size_t n, int deg) { return auto_window(n, deg, g.window_override); }   // msm_plan.h, under gh_msm_set_window
void dist_teardown_locked();                      // dist.hip: gh_shutdown (API lock held) destroys the communicator with the context

// No C++ exception leaves the library (include/ginger_hip.h: "nothing is thrown"; the reference's multi_scalar_mul is
// infallible, variable_base.rs:85-90, and the Rust shim falls back to the CPU path on a non-zero status): every extern "C"
// entry point is a function-try-block whose handler returns api_exception() -- std::bad_alloc -> GH_E_NOMEM, anything else
// -> GH_E_HIP, the message in gh_last_error().  Called from inside a catch handler only.
int api_exception() noexcept;

// Kernels with KB-scale stack frames (the out-of-line EC functions of the cold paths: 2-17 KB per lane, build/*.log) make the
// runtime reserve frame x 64 lanes x resident waves of scratch at dispatch -- up to 9 GB for the MNT6 G2 instances -- and a
// reservation that fails does so inside the runtime's queue handler, which ends the process (the round-3 abort inside
// gh_msm_cached with 640 MB free: DESIGN.md section 9-4b).  scratch_guard() asks the code object for the kernel's frame and
// refuses the launch with GH_E_NOMEM when the card cannot hold the reservation; GH_LAUNCH is hipLaunchKernelGGL behind it.
int scratch_guard(const void* kernel, size_t threads);
#define GH_LAUNCH(kern, grid, block, shmem, st, ...)                                                              \
    do {                                                                                                          \
        const dim3 g_ = (grid), b_ = (block);                                                                     \
        if (int rc_ = gh_rt::scratch_guard((const void*)(kern), (size_t)g_.x * g_.y * g_.z * b_.x * b_.y * b_.z)) \
            return rc_;                                                                                           \
        hipLaunchKernelGGL(kern, g_, b_, shmem, st, __VA_ARGS__);                                                 \
    } while (0)

#define HIPCHK(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            char b_[512];                                                                    \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            gh_rt::g_err = b_;                                                               \
            return e_ == hipErrorOutOfMemory ? GH_E_NOMEM : GH_E_HIP;                        \
        }                                                                                    \
    } while (0)

// Owner of one hipMalloc allocation: whatever way a function is left -- the early returns inside HIPCHK and GH_LAUNCH included
// -- the destructor frees it.  hipFree waits for the device, so nothing that still runs can read freed memory.  For locals and
// for members of heap handles only: an object with static storage duration would free after the HIP runtime is gone, so statics
// keep raw pointers and a g.at_shutdown hook.  release() hands the pointer to a longer-lived struct once a build has succeeded.
class DevMem {
public:
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept : p_(o.release()) {}
    DevMem& operator=(DevMem&& o) noexcept { if (this != &o) { reset(); p_ = o.release(); } return *this; }
    ~DevMem() { reset(); }
    int alloc(size_t bytes) {       // frees what it held; GH_E_NOMEM / GH_E_HIP with the message in g_err
        reset();
        HIPCHK(hipMalloc(&p_, bytes));
        return GH_OK;
    }
    void* get() const { return p_; }
    template <class T> T* as() const { return static_cast<T*>(p_); }
    void* release() { void* p = p_; p_ = nullptr; return p; }
    void reset() { dev_free(p_); }
private:
    void* p_ = nullptr;
};

// ---- curves: the facts every unit needs about a curve id
inline int curve_deg(gh_curve_t c) { return c == GH_MNT4753_G2 ? 2 : (c == GH_MNT6753_G2 ? 3 : 1); }   // extension degree of the base field
template <class C> struct CurveId;
template <> struct CurveId<gh::Mnt4G1> { static constexpr gh_curve_t id = GH_MNT4753_G1; };
template <> struct CurveId<gh::Mnt4G2> { static constexpr gh_curve_t id = GH_MNT4753_G2; };
template <> struct CurveId<gh::Mnt6G1> { static constexpr gh_curve_t id = GH_MNT6753_G1; };
template <> struct CurveId<gh::Mnt6G2> { static constexpr gh_curve_t id = GH_MNT6753_G2; };
inline int unknown_curve() { g_err = "unknown curve id"; return GH_E_BAD_ARG; }
// fn<C>(args) for the curve policy C of a curve id: the two G1 curves (Schnorr, EC-VRF: the caller has checked is_g1), or all four
#define GH_G1_DISPATCH(curve, fn, ...) ((curve) == GH_MNT6753_G1 ? fn<gh::Mnt6G1>(__VA_ARGS__) : fn<gh::Mnt4G1>(__VA_ARGS__))
// fn<P>(args) for the field policy P of a field id; the caller has checked the id (unit_host.h field_ok)
#define GH_FIELD_DISPATCH(field, fn, ...) ((field) == GH_MNT4753_FR ? fn<gh::P6>(__VA_ARGS__) : fn<gh::P4>(__VA_ARGS__))
#define GH_CURVE_DISPATCH(curve, fn, ...)                          \
    ((curve) == GH_MNT4753_G1   ? fn<gh::Mnt4G1>(__VA_ARGS__)       \
     : (curve) == GH_MNT4753_G2 ? fn<gh::Mnt4G2>(__VA_ARGS__)       \
     : (curve) == GH_MNT6753_G1 ? fn<gh::Mnt6G1>(__VA_ARGS__)       \
     : (curve) == GH_MNT6753_G2 ? fn<gh::Mnt6G2>(__VA_ARGS__)       \
                                : gh_rt::unknown_curve())

// ---- per-curve entry points (msm_<curve>.hip)
// A resident key.  The destructor is the one place that knows which device arrays a key owns: `delete h` frees them all.
struct BasesBase {
    gh_curve_t curve;
    size_t n = 0;
    void* d_points = nullptr;   // n x Aff<C>, internal layout
    uint8_t* d_inf = nullptr;   // n bytes or null
    void* d_table = nullptr;    // precomputed shift table: pre_W rows of n x Aff<C> (row w = 2^(pre_c w) P), or null
    int pre_c = 0, pre_W = 0;   // window bits, rows of the table
    int pre_G = 1;              // bucket sets: row j = 2^(pre_c pre_G j) P, window w = j pre_G + g reads row j and files into set g
                                // (1 = full table, one bucket set; GH_TABLE_ROWS caps the rows: a partial table)
    // equal bases (msm_kernels.h "equal bases"): groups of indices that hold the same point up to sign, found when the shift table is built
    uint32_t* d_dup_starts = nullptr;   // n_dup_groups + 1
    uint32_t* d_dup_members = nullptr;  // base index | negative << 31, the canonical base first
    uint32_t* d_dup_chunks = nullptr;   // 3 per chunk (first member, end, group) followed by n_dup_groups + 1 chunk offsets per group
    uint32_t n_dup_groups = 0, n_dup_members = 0, n_dup_chunks = 0;
    uint8_t aff_asm_off = 0;    // G2: an MSM over this key overflowed the exception list of the assembly rounds (a key with many equal
                                // bases, e.g. a proving key's b_g2_query under an assignment with equal values: every pair of such bases
                                // in a bucket is a doubling) -- later MSMs go straight to the C++ round kernel, which doubles inline
    static constexpr uint32_t MAGIC = 0x6768424au;
    uint32_t magic = MAGIC;
    BasesBase() = default;
    BasesBase(const BasesBase&) = delete;
    BasesBase& operator=(const BasesBase&) = delete;
    ~BasesBase() {
        dev_free(d_points); dev_free(d_inf); dev_free(d_table);
        dev_free(d_dup_starts); dev_free(d_dup_members); dev_free(d_dup_chunks);
        magic = 0;
    }
};
// the checked cast of a handle of the C ABI: null for a null pointer or for memory that is not a live key
inline BasesBase* bases_of(gh_bases_t handle) {
    BasesBase* h = reinterpret_cast<BasesBase*>(handle);
    return h && h->magic == BasesBase::MAGIC ? h : nullptr;
}
struct MsmOps {
    int (*upload)(const uint64_t* bases, const uint8_t* infinity, size_t n, int canonical, BasesBase** out);
    int (*run)(BasesBase* h, const void* d_scalars, size_t n_scalars, uint64_t* out_xyz);
    int (*host)(const uint64_t* bases, const uint8_t* infinity, size_t n_bases, const uint64_t* scalars,
                size_t n_scalars, uint64_t* out_xyz);
    int (*proj_add)(uint64_t* acc_xyz, const uint64_t* p_xyz);
    int (*to_affine)(const uint64_t* xyz, uint64_t* out_xy, uint8_t* is_infinity);
    int (*precompute)(BasesBase* h, int window_bits, int max_rows);
    int (*batch)(BasesBase* const* hs, const void* const* d_scalars, const size_t* n_scalars, int count, uint64_t* out_xyz);
    int (*proj_mul)(const uint64_t* p_xyz, const uint64_t* scalar12, uint64_t* out_xyz);
    int (*proj_neg)(uint64_t* xyz);
    int (*acc_lists)(const void* points, const uint32_t* sorted, const uint32_t* starts, const uint32_t* counts,
                     const uint32_t* order, uint32_t total, void* out_proj, hipStream_t st);
};
const MsmOps* msm_ops_mnt4753_g1();
const MsmOps* msm_ops_mnt4753_g2();
const MsmOps* msm_ops_mnt6753_g1();
const MsmOps* msm_ops_mnt6753_g2();
const MsmOps* ops_of(gh_curve_t curve);            // null, with "unknown curve id" in g_err, for anything else

// ---- transforms (ntt.hip)
int fft_run(gh_field_t field, void* d_data, uint32_t log_n, uint32_t flags);
int vec_op(gh_field_t field, int op, void* d_a, const void* d_b, const uint64_t* scalar12, size_t n);
int witness_map(gh_field_t field, void* d_a, void* d_b, void* d_c, uint32_t log_n, const uint64_t* d1,
                const uint64_t* d2, const uint64_t* d3, void* d_h);
int sap_witness_map(gh_field_t field, void* d_a, void* d_c, uint32_t log_n, const uint64_t* d1, const uint64_t* d2, void* d_h);
int batch_inverse(gh_field_t field, void* d_a, size_t n);
int lagrange_coefficients(gh_field_t field, uint32_t log_n, const uint64_t* tau12, void* d_out);
// *tw = the domain's table of group_gen^i, i < 2^log_n, in the internal form (built on first use); null for log_n = 0, which has none
int domain_table(gh_field_t field, uint32_t log_n, const gh::Fp** tw);

// ---- lock-held helpers for other units (schnorr.hip, ecvrf.hip); the caller holds api_mutex() and has run ensure_init()
struct FixedTable;                                 // fixed_base.hip: a window table of one base
int fixed_table_create(gh_curve_t curve, const uint64_t* g_xyz, size_t scalar_size, int window, FixedTable** out);
int fixed_table_sums(const FixedTable* t, const void* d_scalars, size_t n, void* d_out_proj);   // on g.stream, internal Proj<C>
void fixed_table_destroy(FixedTable* t);          // null is fine
int poseidon_field(const gh_poseidon* h, gh_field_t* out);                              // GH_E_BAD_HANDLE if h is none
int poseidon_hash_dev_locked(gh_poseidon* h, const void* d_in, size_t n, size_t len, void* d_out);   // on g.stream, no sync
void poseidon_trim_slab();                         // the release of a large slab every Poseidon entry point does on return
// points.hip, on g.stream, no sync: d_code[i * stride] = the GH_POINT_* code of point i (membership: 0, 3 or 4; decompression: 0 .. 4,
// d_xy / d_inf the points, failed rows zero).  points_validate_mark(0 / 1) brackets such launches on the points unit's own timer;
// points_validate_finish(), after the caller's stream synchronise, makes their distance the validate phase of gh_points_last_timing.
int points_member_dev(gh_curve_t curve, const void* d_xy, const uint8_t* d_inf, size_t n, uint8_t* d_code, size_t stride);
int points_decompress_dev(gh_curve_t curve, const void* d_x, const uint8_t* d_flags, size_t n, void* d_xy, uint8_t* d_inf, uint8_t* d_code, size_t stride);
int points_validate_mark(int end);
int points_validate_finish();

}  // namespace gh_rt
