// points.hip -- the C ABI of include/ginger_hip_points.h but for its two verifiers (pairing.hip): batched group membership,
// decompression and compression of points, one row per lane, and the device-side entries the verifiers validate their proof
// points through.  The arithmetic is the GH_HD text of sqrt29.h; here are the kernels around it, the constants in device
// memory and the host steps.  DESIGN.md section 15.
//
// Every loop a kernel runs has a compile-time trip count (sqrt29.h): a row's input decides which rounds correct and which
// status comes out, never how long the lane runs.
#include "vb_kernels.h"
#include "sqrt29.h"
#include "../../include/ginger_hip_points.h"

namespace {

PhaseTimer g_tm{3};                                // upload, validate, download

// (t - 1) / 2 of the three fields a root is taken in, and the signed digits of the two group orders
__constant__ uint32_t c_e_p4[SQRT_E_WORDS_P4] = GH_P4_SQRT_E32;
__constant__ uint32_t c_e_p6[SQRT_E_WORDS_P6] = GH_P6_SQRT_E32;
__constant__ uint32_t c_e_p6q3[SQRT_E_WORDS_P6Q3] = GH_P6Q3_SQRT_E32;
__constant__ int8_t c_r_mnt4[GH_MNT4_R_DIGITS] = GH_MNT4_R_NAF;
__constant__ int8_t c_r_mnt6[GH_MNT6_R_DIGITS] = GH_MNT6_R_NAF;
template <class C> __device__ __forceinline__ const uint32_t* sqrt_e();
template <class C> __device__ __forceinline__ const int8_t* r_naf();
template <> __device__ __forceinline__ const uint32_t* sqrt_e<Mnt4G1>() { return c_e_p4; }
template <> __device__ __forceinline__ const uint32_t* sqrt_e<Mnt4G2>() { return c_e_p4; }
template <> __device__ __forceinline__ const uint32_t* sqrt_e<Mnt6G1>() { return c_e_p6; }
template <> __device__ __forceinline__ const uint32_t* sqrt_e<Mnt6G2>() { return c_e_p6q3; }
template <> __device__ __forceinline__ const int8_t* r_naf<Mnt4G1>() { return c_r_mnt4; }
template <> __device__ __forceinline__ const int8_t* r_naf<Mnt4G2>() { return c_r_mnt4; }
template <> __device__ __forceinline__ const int8_t* r_naf<Mnt6G1>() { return c_r_mnt6; }
template <> __device__ __forceinline__ const int8_t* r_naf<Mnt6G2>() { return c_r_mnt6; }

// u32 words of a coordinate in ABI form; a point is two of them, a compressed x one
template <class C> constexpr int coord_words() { return 24 * C::FC::DEG; }

// out[i * stride] = the GH_POINT_* code of point i (0, NotOnCurve or NotPrimeOrder), or with as_ok whether it is 0
template <class C>
__global__ void __launch_bounds__(BLOCK)
member_kernel(const uint32_t* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n, typename C::FC::T b, uint8_t* __restrict__ out,
              size_t stride, int as_ok) {
    typedef typename C::FC F;
    constexpr int W = coord_words<C>();
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint8_t code = PT_OK;
    if (!inf[i]) {
        const Aff<C> p{F::from_abi(xy + i * 2 * W), F::from_abi(xy + i * 2 * W + W)};
        if (!aff_on_curve<C>(p, b)) code = PT_NOT_ON_CURVE;
        else if constexpr (!PointCurve<C>::PRIME_ORDER)
            if (!r_times_is_zero<C>(p, r_naf<C>())) code = PT_NOT_PRIME_ORDER;
    }
    out[i * stride] = as_ok ? code == PT_OK : code;
}

template <class C>
__global__ void __launch_bounds__(BLOCK)
decompress_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ flags, size_t n, typename C::FC::T b, uint32_t* __restrict__ out_xy,
                  uint8_t* __restrict__ out_inf, uint8_t* __restrict__ status, size_t stride) {
    typedef typename C::FC F;
    constexpr int W = coord_words<C>();
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    Aff<C> p;
    bool inf;
    const uint8_t st = decompress_row<C>(x + i * W, flags[i], b, sqrt_e<C>(), r_naf<C>(), p, inf);
    F::to_abi(out_xy + i * 2 * W, p.x);                      // a failed row: zero
    F::to_abi(out_xy + i * 2 * W + W, p.y);
    out_inf[i] = inf;
    status[i * stride] = st;
}

template <class C>
__global__ void __launch_bounds__(BLOCK)
compress_kernel(const uint32_t* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n, uint32_t* __restrict__ out_x,
                uint8_t* __restrict__ out_flags) {
    typedef typename C::FC F;
    constexpr int W = coord_words<C>();
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const Aff<C> p{F::from_abi(xy + i * 2 * W), F::from_abi(xy + i * 2 * W + W)};
    out_flags[i] = compress_row<C>(p, inf[i] != 0, out_x + i * W);
}

// ---------------------------------------------------------------------------------------------------- host side
template <class C> int member_dev(const void* d_xy, const uint8_t* d_inf, size_t n, uint8_t* d_out, size_t stride, int as_ok) {
    GH_LAUNCH((member_kernel<C>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_xy, d_inf, n, PointCurve<C>::b(), d_out,
              stride, as_ok);
    HIPCHK(hipGetLastError());
    return GH_OK;
}
template <class C> int decompress_dev(const void* d_x, const uint8_t* d_flags, size_t n, void* d_xy, uint8_t* d_inf, uint8_t* d_code, size_t stride) {
    GH_LAUNCH((decompress_kernel<C>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_x, d_flags, n, PointCurve<C>::b(),
              (uint32_t*)d_xy, d_inf, d_code, stride);
    HIPCHK(hipGetLastError());
    return GH_OK;
}

// u64 words of a coordinate
template <class C> constexpr size_t coord_u64() { return 12 * C::FC::DEG; }

template <class C> int run_membership(const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_ok) {
    constexpr size_t CW = coord_u64<C>();
    uint64_t* d_xy;
    uint8_t *d_inf, *d_ok;
    int rc = dbuf("vb_pts_xy", n * 2 * CW, &d_xy);
    if (!rc) rc = dbuf("vb_pts_inf", n, &d_inf);
    if (!rc) rc = dbuf("vb_pts_st", n, &d_ok);
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark()) || (rc = up(d_xy, xy, n * 2 * CW)) || (rc = up(d_inf, inf, n)) || (rc = ph.mark())) return rc;
    if ((rc = member_dev<C>(d_xy, d_inf, n, d_ok, 1, 1)) || (rc = ph.mark())) return rc;
    HIPCHK(hipMemcpyAsync(out_ok, d_ok, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

template <class C> int run_decompress(const uint64_t* x, const uint8_t* flags, size_t n, uint64_t* out_xy, uint8_t* out_inf, uint8_t* out_status) {
    constexpr size_t CW = coord_u64<C>();
    uint64_t *d_x, *d_xy;
    uint8_t *d_fl, *d_inf, *d_st;
    int rc = dbuf("vb_pts_x", n * CW, &d_x);
    if (!rc) rc = dbuf("vb_pts_fl", n, &d_fl);
    if (!rc) rc = dbuf("vb_pts_xy", n * 2 * CW, &d_xy);
    if (!rc) rc = dbuf("vb_pts_inf", n, &d_inf);
    if (!rc) rc = dbuf("vb_pts_st", n, &d_st);
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark()) || (rc = up(d_x, x, n * CW)) || (rc = up(d_fl, flags, n)) || (rc = ph.mark())) return rc;
    if ((rc = decompress_dev<C>(d_x, d_fl, n, d_xy, d_inf, d_st, 1)) || (rc = ph.mark())) return rc;
    HIPCHK(hipMemcpyAsync(out_xy, d_xy, n * 2 * CW * 8, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_inf, d_inf, n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

template <class C> int run_compress(const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_x, uint8_t* out_flags) {
    constexpr size_t CW = coord_u64<C>();
    uint64_t *d_x, *d_xy;
    uint8_t *d_fl, *d_inf;
    int rc = dbuf("vb_pts_x", n * CW, &d_x);
    if (!rc) rc = dbuf("vb_pts_fl", n, &d_fl);
    if (!rc) rc = dbuf("vb_pts_xy", n * 2 * CW, &d_xy);
    if (!rc) rc = dbuf("vb_pts_inf", n, &d_inf);
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark()) || (rc = up(d_xy, xy, n * 2 * CW)) || (rc = up(d_inf, inf, n)) || (rc = ph.mark())) return rc;
    GH_LAUNCH((compress_kernel<C>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_xy, (const uint8_t*)d_inf, n, (uint32_t*)d_x,
              d_fl);
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipMemcpyAsync(out_x, d_x, n * CW * 8, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_flags, d_fl, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

// the coefficients of n points (Montgomery form) are below the curve's base modulus
template <class C> bool coords_below(const uint64_t* xy, size_t n) { return all_below<typename C::PF>(xy, 2 * C::FC::DEG * n); }

// what every entry point checks of the curve, the pointers (non_null) and the row count
int check_call(gh_curve_t curve, size_t n, bool non_null) {
    if (curve < GH_MNT4753_G1 || curve > GH_MNT6753_G2) return gh_rt::unknown_curve();
    if (n && !non_null) return null_arg();
    size_t b;
    if (mul_overflows(n, 4096, &b)) return too_large();
    return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- for pairing_impl.h
namespace gh_rt {

int points_member_dev(gh_curve_t curve, const void* d_xy, const uint8_t* d_inf, size_t n, uint8_t* d_code, size_t stride) {
    return GH_CURVE_DISPATCH(curve, member_dev, d_xy, d_inf, n, d_code, stride, 0);
}
int points_decompress_dev(gh_curve_t curve, const void* d_x, const uint8_t* d_flags, size_t n, void* d_xy, uint8_t* d_inf, uint8_t* d_code,
                          size_t stride) {
    return GH_CURVE_DISPATCH(curve, decompress_dev, d_x, d_flags, n, d_xy, d_inf, d_code, stride);
}
int points_validate_mark(int end) {
    return end ? g_tm.mark() : g_tm.begin().mark();
}
int points_validate_finish() { return g_tm.single(1); }

}  // namespace gh_rt

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

extern "C" {

int gh_group_membership(gh_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out_ok) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = check_call(curve, n, xy && inf && out_ok)) return rc;
    if (!GH_CURVE_DISPATCH(curve, coords_below, xy, n)) { g_err = "a coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_CURVE_DISPATCH(curve, run_membership, xy, inf, n, out_ok);
} catch (...) { return gh_rt::api_exception(); }

int gh_points_decompress(gh_curve_t curve, const uint64_t* x, const uint8_t* flags, size_t n, uint64_t* out_xy, uint8_t* out_inf,
                         uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = check_call(curve, n, x && flags && out_xy && out_inf && out_status)) return rc;
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_CURVE_DISPATCH(curve, run_decompress, x, flags, n, out_xy, out_inf, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_points_compress(gh_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_x, uint8_t* out_flags) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = check_call(curve, n, xy && inf && out_x && out_flags)) return rc;
    if (!GH_CURVE_DISPATCH(curve, coords_below, xy, n)) { g_err = "a coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_CURVE_DISPATCH(curve, run_compress, xy, inf, n, out_x, out_flags);
} catch (...) { return gh_rt::api_exception(); }

int gh_points_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return g_tm.copy_out(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
