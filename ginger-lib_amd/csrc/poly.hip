// poly.hip -- the C ABI of include/ginger_hip_poly.h: DensePolynomial, SparsePolynomial and Evaluations arithmetic of
// algebra::fft over vectors that stay on the device.  The level arithmetic is poly_plan.h, the lane bodies are
// poly_kernels.h (both host-tested); here are the kernels that put a thread index in front of them, the launch sequences and
// the entry points.  DESIGN.md section 17.
//
//   poly_fold_kernel         one level of a Horner fold: lane g folds c_g, c_(g + G), ... in w = z^G; KP points share one pass
//                            over the coefficients (level 0 of evaluate), the levels above run one point per grid.y
//   poly_scan_seg_kernel     pass 1 of the suffix scan T_i = x_i + mu T_(i + N): the outgoing value of every segment
//   poly_scan_write_kernel   pass 2: every segment again from its true carry, writing T.  With products and N = 1 this is the
//                            division by x - z, without products and N = 2^log_n the division by the vanishing polynomial
//   poly_axpy_kernel, poly_mul_vanishing_kernel, poly_elements_kernel, poly_sparse_kernel   one lane per row
//   poly_reduce_kernel       per-block maximum (last non-zero row) or sum (zero rows); the host finishes the per-block results
// Mul and the division of evaluations are sequences over fft_run, vec_op and batch_inverse of runtime.h.
#include <algorithm>
#include <vector>
#include "unit_host.h"
#include "poly_kernels.h"
#include "../../include/ginger_hip_poly.h"

namespace {

using gh_rt::DevMem;

constexpr int BLOCK = 128;             // the fold and the scan: lanes that hold a product
constexpr int EBLOCK = 256;            // one row per lane
constexpr int RBLOCK = 256, RITEMS = 8;   // a block of the reduction covers RBLOCK * RITEMS rows
constexpr int FOLD_GROUP = 4;          // points that share a pass over the coefficients

PolyTuning g_tune;
PhaseTimer g_tm{1};                    // one bracket: from before the first launch to the one wait of an entry point

// ---------------------------------------------------------------------------------------------------- kernels
// w: k factors of this level; point p0 + p reads fin + (p0 + p) in_stride (ABI_IN: every point reads abi) and writes
// out + (p0 + p) out_stride, or row p0 + p of out_abi where that is given (the last level: G = 1)
template <class P, int KP, bool ABI_IN>
__global__ void __launch_bounds__(BLOCK)
poly_fold_kernel(uint64_t n, uint64_t G, const uint32_t* __restrict__ abi, const Fp* __restrict__ fin, uint64_t in_stride, const Fp* __restrict__ w,
                 uint32_t k, Fp* __restrict__ out, uint64_t out_stride, uint32_t* __restrict__ out_abi) {
    __shared__ Fp ws[KP];
    const uint32_t p0 = blockIdx.y * KP;
    if (threadIdx.x < KP) ws[threadIdx.x] = w[p0 + threadIdx.x < k ? p0 + threadIdx.x : k - 1];   // a partial group repeats the last point
    __syncthreads();
    const uint64_t gi = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (gi >= G) return;
    Fp acc[KP];
    poly_fold_lane<P, KP, ABI_IN>(n, G, gi, abi, ABI_IN ? nullptr : fin + (uint64_t)p0 * in_stride, ws, acc);
#pragma unroll
    for (int p = 0; p < KP; p++) {
        if (p0 + p >= k) continue;
        if (out_abi) poly_st_row(out_abi + (uint64_t)(p0 + p) * 24, acc[p]);
        else out[(uint64_t)(p0 + p) * out_stride + gi] = acc[p];
    }
}

template <class P, bool ABI_IN, bool MUL>
__global__ void __launch_bounds__(BLOCK)
poly_scan_seg_kernel(PolyScanLevel lv, const uint32_t* __restrict__ abi, const Fp* __restrict__ fin, Fp mu, Fp* __restrict__ next) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= lv.lanes()) return;
    next[t] = poly_scan_seg_lane<P, ABI_IN, MUL>(lv, t, abi, fin, mu);           // t = s N + r: the element of the next level
}

template <class P, bool ABI, bool MUL>
__global__ void __launch_bounds__(BLOCK)
poly_scan_write_kernel(PolyScanLevel lv, const uint32_t* __restrict__ abi, Fp* fio, Fp mu, const Fp* __restrict__ carry, uint64_t split, uint32_t* lo,
                       uint32_t* hi) {
    const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= lv.lanes()) return;
    poly_scan_write_lane<P, ABI, MUL>(lv, t, abi, fio, mu, carry, split, lo, hi);
}

template <class P>
__global__ void __launch_bounds__(EBLOCK)
poly_axpy_kernel(int op, const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb, Fp f, uint32_t* out, uint64_t rows) {
    const uint64_t i = (uint64_t)blockIdx.x * EBLOCK + threadIdx.x;
    if (i < rows) poly_axpy_lane<P>(op, i, a, na, b, nb, f, out);
}

template <class P>
__global__ void __launch_bounds__(EBLOCK) poly_mul_vanishing_kernel(const uint32_t* __restrict__ in, uint64_t n, uint64_t N, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * EBLOCK + threadIdx.x;
    if (i < n + N) poly_mul_vanishing_lane<P>(i, in, n, N, out);
}

template <class P> __global__ void __launch_bounds__(EBLOCK) poly_elements_kernel(const Fp* __restrict__ tw, uint64_t N, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * EBLOCK + threadIdx.x;
    if (i < N) poly_elements_lane<P>(i, tw, out);
}

template <class P>
__global__ void __launch_bounds__(EBLOCK)
poly_sparse_kernel(uint32_t log_n, const Fp* __restrict__ tw, const uint64_t* __restrict__ exps, const Fp* __restrict__ coeffs, uint64_t t,
                   uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * EBLOCK + threadIdx.x;
    if (i < ((uint64_t)1 << log_n)) poly_sparse_lane<P>(i, log_n, tw, exps, coeffs, t, out);
}

// COUNT = false: per_block[b] = the last non-zero row of the block's rows plus one (0: none); true: its number of zero rows
template <bool COUNT> __global__ void __launch_bounds__(RBLOCK) poly_reduce_kernel(const uint32_t* __restrict__ rows, uint64_t n, uint64_t* __restrict__ per_block) {
    __shared__ uint64_t part[RBLOCK];
    const uint64_t first = (uint64_t)blockIdx.x * RBLOCK * RITEMS;
    const uint64_t end = first + RBLOCK * RITEMS < n ? first + RBLOCK * RITEMS : n;
    part[threadIdx.x] = COUNT ? poly_count_zero(rows, end, first + threadIdx.x, RBLOCK) : poly_last_nonzero(rows, end, first + threadIdx.x, RBLOCK);
    __syncthreads();
    for (int h = RBLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const uint64_t o = part[threadIdx.x + h];
            part[threadIdx.x] = COUNT ? part[threadIdx.x] + o : (o > part[threadIdx.x] ? o : part[threadIdx.x]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) per_block[blockIdx.x] = part[0];
}

// ---------------------------------------------------------------------------------------------------- host side
int two_adicity(gh_field_t f) { return f == GH_MNT4753_FR ? GH_P6_TWO_ADICITY : GH_P4_TWO_ADICITY; }
int rows_ok(size_t n) { return n > (SIZE_MAX >> 9) ? too_large() : GH_OK; }
int domain_ok(gh_field_t f, uint32_t log_n) {
    if ((int)log_n >= two_adicity(f)) { g_err = "domain exceeds the field's 2-adicity"; return GH_E_UNSUPPORTED; }
    return GH_OK;
}

// the end of a timed entry point: the second mark, the one wait, the record of gh_poly_last_timing
int wait_timed() {
    HIPCHK(hipGetLastError());
    if (int rc = g_tm.mark()) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return g_tm.single(0);
}

// ---- evaluate.  hw must outlive the caller's wait: its upload is asynchronous.
template <class P> int evaluate_issue(const uint32_t* d_c, size_t n, const uint64_t* points12, size_t k, uint32_t* d_res, std::vector<Fp>& hw) {
    PolyFoldLevel lv[POLY_MAX_LEVELS];
    const int nl = poly_fold_levels(n, g_tune, lv);
    if (!nl) {
        HIPCHK(hipMemsetAsync(d_res, 0, k * 96, g.stream));
        return GH_OK;
    }
    hw.resize((size_t)nl * k);
    for (size_t p = 0; p < k; p++) {
        const Fp z = from_abi12<P>(points12 + 12 * p);
        for (int l = 0; l < nl; l++) hw[(size_t)l * k + p] = poly_pow<P>(z, lv[l].G);
    }
    size_t total = 0;
    for (int l = 0; l + 1 < nl; l++) total += (size_t)lv[l].G * k;
    Fp *d_w, *d_lvl = nullptr;
    if (int rc = dbuf("poly_w", hw.size(), &d_w, 0)) return rc;
    if (total)
        if (int rc = dbuf("poly_lvl", total, &d_lvl, 0)) return rc;
    HIPCHK(hipMemcpyAsync(d_w, hw.data(), hw.size() * sizeof(Fp), hipMemcpyHostToDevice, g.stream));
    const Fp* in = nullptr;
    Fp* out = d_lvl;
    for (int l = 0; l < nl; l++) {
        const bool last = l == nl - 1;
        const Fp* w = d_w + (size_t)l * k;
        if (l == 0 && k >= 2)
            GH_LAUNCH((poly_fold_kernel<P, FOLD_GROUP, true>), dim3(blocks(lv[l].G, BLOCK), blocks(k, FOLD_GROUP)), dim3(BLOCK), 0, g.stream, lv[l].n, lv[l].G, d_c,
                      (const Fp*)nullptr, (uint64_t)0, w, (uint32_t)k, out, lv[l].G, last ? d_res : (uint32_t*)nullptr);
        else if (l == 0)
            GH_LAUNCH((poly_fold_kernel<P, 1, true>), dim3(blocks(lv[l].G, BLOCK), (unsigned)k), dim3(BLOCK), 0, g.stream, lv[l].n, lv[l].G, d_c, (const Fp*)nullptr,
                      (uint64_t)0, w, (uint32_t)k, out, lv[l].G, last ? d_res : (uint32_t*)nullptr);
        else
            GH_LAUNCH((poly_fold_kernel<P, 1, false>), dim3(blocks(lv[l].G, BLOCK), (unsigned)k), dim3(BLOCK), 0, g.stream, lv[l].n, lv[l].G,
                      (const uint32_t*)nullptr, in, lv[l].n, w, (uint32_t)k, out, lv[l].G, last ? d_res : (uint32_t*)nullptr);
        in = out;
        out += (size_t)lv[l].G * k;
    }
    return GH_OK;
}
template <class P> int evaluate_run(const void* d_c, size_t n, const uint64_t* points12, size_t k, uint64_t* out12) {
    uint32_t* d_res;
    if (int rc = dbuf("poly_res", k * 24, &d_res, 0)) return rc;
    std::vector<Fp> hw;
    int rc = g_tm.begin().mark();
    if (!rc) rc = evaluate_issue<P>((const uint32_t*)d_c, n, points12, k, d_res, hw);
    if (rc) { (void)hipStreamSynchronize(g.stream); return rc; }
    HIPCHK(hipMemcpyAsync(out12, d_res, k * 96, hipMemcpyDeviceToHost, g.stream));
    return wait_timed();
}

// ---- scan: T over the m rows of d_in with stride N; T_i goes to row i of lo where i < split, to row i - split of hi otherwise
template <class P, bool MUL>
int scan_issue(const uint32_t* d_in, uint64_t m, uint64_t N, uint32_t L, uint32_t limit, const Fp& mu0, uint64_t split, uint32_t* lo, uint32_t* hi) {
    PolyScanLevel lv[POLY_MAX_LEVELS];
    const int nl = poly_scan_levels(m, N, L, limit, lv);
    if (!nl) return GH_OK;
    size_t total = 0;
    for (int l = 1; l < nl; l++) total += (size_t)lv[l].m;
    Fp* d_lvl = nullptr;
    if (total)
        if (int rc = dbuf("poly_lvl", total, &d_lvl, 0)) return rc;
    std::vector<Fp*> vec((size_t)nl, nullptr);
    std::vector<Fp> mu((size_t)nl, mu0);
    for (int l = 1; l < nl; l++) {
        vec[l] = l == 1 ? d_lvl : vec[l - 1] + lv[l - 1].m;
        if (MUL) mu[l] = poly_pow<P>(mu[l - 1], lv[l - 1].L);
    }
    for (int l = 0; l + 1 < nl; l++) {
        const dim3 grid(blocks(lv[l].lanes(), BLOCK));
        if (l == 0) GH_LAUNCH((poly_scan_seg_kernel<P, true, MUL>), grid, dim3(BLOCK), 0, g.stream, lv[l], d_in, (const Fp*)nullptr, mu[l], vec[l + 1]);
        else GH_LAUNCH((poly_scan_seg_kernel<P, false, MUL>), grid, dim3(BLOCK), 0, g.stream, lv[l], (const uint32_t*)nullptr, (const Fp*)vec[l], mu[l], vec[l + 1]);
    }
    for (int l = nl - 1; l >= 0; l--) {
        const dim3 grid(blocks(lv[l].lanes(), BLOCK));
        const Fp* carry = l == nl - 1 ? nullptr : vec[l + 1];
        if (l == 0) GH_LAUNCH((poly_scan_write_kernel<P, true, MUL>), grid, dim3(BLOCK), 0, g.stream, lv[l], d_in, (Fp*)nullptr, mu[l], carry, split, lo, hi);
        else GH_LAUNCH((poly_scan_write_kernel<P, false, MUL>), grid, dim3(BLOCK), 0, g.stream, lv[l], (const uint32_t*)nullptr, vec[l], mu[l], carry, (uint64_t)0,
                       (uint32_t*)nullptr, (uint32_t*)nullptr);
    }
    return GH_OK;
}

template <class P> int divide_linear_run(const void* d_in, size_t n, const uint64_t* z12, void* d_q, uint64_t* rem12) {
    if (n == 0) {
        for (int i = 0; i < 12; i++) rem12[i] = 0;
        return GH_OK;
    }
    uint32_t* d_rem;
    if (int rc = dbuf("poly_res", (size_t)24, &d_rem, 0)) return rc;
    int rc = g_tm.begin().mark();
    if (!rc) rc = scan_issue<P, true>((const uint32_t*)d_in, n, 1, g_tune.run_len, g_tune.direct_max, from_abi12<P>(z12), 1, d_rem, (uint32_t*)d_q);
    if (rc) { (void)hipStreamSynchronize(g.stream); return rc; }
    HIPCHK(hipMemcpyAsync(rem12, d_rem, 96, hipMemcpyDeviceToHost, g.stream));
    return wait_timed();
}

template <class P> int divide_vanishing_run(const void* d_in, size_t n, uint32_t log_n, void* d_q, void* d_r) {
    const uint64_t N = (uint64_t)1 << log_n;
    int rc = g_tm.begin().mark();
    if (rc) return rc;
    if (n < N) HIPCHK(hipMemsetAsync((uint8_t*)d_r + n * 96, 0, (N - n) * 96, g.stream));      // r = p padded with zeros
    rc = scan_issue<P, false>((const uint32_t*)d_in, n, N, g_tune.seg_max, g_tune.seg_max, fp_zero(), N, (uint32_t*)d_r, (uint32_t*)d_q);
    if (rc) { (void)hipStreamSynchronize(g.stream); return rc; }
    return wait_timed();
}

// ---- reductions, each with its own wait: *result is the host's finish of the per-block results
template <bool COUNT> int reduce_rows(const uint32_t* d, size_t n, size_t* result) {
    *result = 0;
    if (!n) return GH_OK;
    const size_t nb = blocks(n, RBLOCK * RITEMS);
    uint64_t* d_pb;
    if (int rc = dbuf("poly_red", nb, &d_pb, 0)) return rc;
    std::vector<uint64_t> pb(nb);
    GH_LAUNCH((poly_reduce_kernel<COUNT>), dim3((unsigned)nb), dim3(RBLOCK), 0, g.stream, d, (uint64_t)n, d_pb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pb.data(), d_pb, nb * 8, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (uint64_t v : pb) *result = COUNT ? *result + (size_t)v : std::max(*result, (size_t)v);
    return GH_OK;
}
// The trimmed length looks at the last block's worth of rows first: a coefficient vector usually ends in a non-zero row, and
// the whole vector is then never read.
template <bool COUNT> int reduce_run(const void* d, size_t n, size_t* result) {
    constexpr size_t TAIL = (size_t)RBLOCK * RITEMS;
    if (!COUNT && n > TAIL) {
        if (int rc = reduce_rows<false>((const uint32_t*)d + (n - TAIL) * 24, TAIL, result)) return rc;
        if (*result) { *result += n - TAIL; return GH_OK; }
        n -= TAIL;
    }
    return reduce_rows<COUNT>((const uint32_t*)d, n, result);
}

template <class P> int axpy_run(int op, const void* d_a, size_t na, const void* d_b, size_t nb, const uint64_t* f12, void* d_out) {
    const size_t rows = std::max(na, nb);
    if (!rows) return GH_OK;
    const Fp f = f12 ? from_abi12<P>(f12) : fp_zero();
    if (int rc = g_tm.begin().mark()) return rc;
    GH_LAUNCH((poly_axpy_kernel<P>), dim3(blocks(rows, EBLOCK)), dim3(EBLOCK), 0, g.stream, op, (const uint32_t*)d_a, (uint64_t)na, (const uint32_t*)d_b, (uint64_t)nb,
              f, (uint32_t*)d_out, (uint64_t)rows);
    return wait_timed();
}

template <class P> int mul_vanishing_run(const void* d_in, size_t n, uint32_t log_n, void* d_out) {
    const uint64_t N = (uint64_t)1 << log_n;
    if (int rc = g_tm.begin().mark()) return rc;
    GH_LAUNCH((poly_mul_vanishing_kernel<P>), dim3(blocks(n + N, EBLOCK)), dim3(EBLOCK), 0, g.stream, (const uint32_t*)d_in, (uint64_t)n, N, (uint32_t*)d_out);
    return wait_timed();
}

template <class P> int elements_run(gh_field_t field, uint32_t log_n, void* d_out) {
    const Fp* tw;
    if (int rc = gh_rt::domain_table(field, log_n, &tw)) return rc;
    const uint64_t N = (uint64_t)1 << log_n;
    if (int rc = g_tm.begin().mark()) return rc;
    GH_LAUNCH((poly_elements_kernel<P>), dim3(blocks(N, EBLOCK)), dim3(EBLOCK), 0, g.stream, tw, N, (uint32_t*)d_out);
    return wait_timed();
}

template <class P> int sparse_run(gh_field_t field, const uint64_t* exps, const uint64_t* coeffs12, size_t t, uint32_t log_n, void* d_out) {
    const Fp* tw;
    if (int rc = gh_rt::domain_table(field, log_n, &tw)) return rc;
    const uint64_t N = (uint64_t)1 << log_n;
    std::vector<uint64_t> he(t);
    std::vector<Fp> hc(t);
    for (size_t j = 0; j < t; j++) {
        he[j] = exps[j] & (N - 1);
        hc[j] = fp_unpack(reinterpret_cast<const uint32_t*>(coeffs12 + 12 * j));
    }
    uint64_t* d_e = nullptr;
    Fp* d_c = nullptr;
    if (t) {
        int rc;
        if ((rc = dbuf("poly_sp_e", t, &d_e, 0)) || (rc = dbuf("poly_sp_c", t, &d_c, 0))) return rc;
    }
    if (int rc = g_tm.begin().mark()) return rc;
    if (t) {
        HIPCHK(hipMemcpyAsync(d_e, he.data(), t * 8, hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipMemcpyAsync(d_c, hc.data(), t * sizeof(Fp), hipMemcpyHostToDevice, g.stream));
    }
    GH_LAUNCH((poly_sparse_kernel<P>), dim3(blocks(N, EBLOCK)), dim3(EBLOCK), 0, g.stream, log_n, tw, (const uint64_t*)d_e, (const Fp*)d_c, (uint64_t)t, (uint32_t*)d_out);
    return wait_timed();                                          // he, hc live until here
}

// Mul (dense.rs:342-357).  The checks that need the trimmed lengths come first, as the reference returns zero before it asks
// for a domain.
int mul_run(gh_field_t field, const void* d_a, size_t na, const void* d_b, size_t nb, void* d_out, size_t out_cap, size_t* n_out) {
    *n_out = 0;
    size_t ta = 0, tb = 0;
    int rc;
    if ((rc = reduce_run<false>(d_a, na, &ta)) || (rc = reduce_run<false>(d_b, nb, &tb))) return rc;
    if (!ta || !tb) return GH_OK;
    uint32_t log_n = 0;
    while (((size_t)1 << log_n) < na + nb) log_n++;
    if ((rc = domain_ok(field, log_n))) return rc;
    const size_t N = (size_t)1 << log_n;
    if (out_cap < N) { g_err = "out_cap: the output holds fewer rows than the domain of n_a + n_b coefficients"; return GH_E_BAD_ARG; }
    uint8_t* d_pb;
    if ((rc = dbuf("poly_mul_b", N * 96, &d_pb, 0))) return rc;
    if ((rc = g_tm.begin().mark())) return rc;
    uint8_t* d_pa = (uint8_t*)d_out;
    HIPCHK(hipMemcpyAsync(d_pa, d_a, ta * 96, hipMemcpyDeviceToDevice, g.stream));             // rows from the trimmed length on are zero
    HIPCHK(hipMemsetAsync(d_pa + ta * 96, 0, (N - ta) * 96, g.stream));
    HIPCHK(hipMemcpyAsync(d_pb, d_b, tb * 96, hipMemcpyDeviceToDevice, g.stream));
    HIPCHK(hipMemsetAsync(d_pb + tb * 96, 0, (N - tb) * 96, g.stream));
    if ((rc = gh_rt::fft_run(field, d_pa, log_n, 0)) || (rc = gh_rt::fft_run(field, d_pb, log_n, 0)) || (rc = gh_rt::vec_op(field, 0, d_pa, d_pb, nullptr, N)) ||
        (rc = gh_rt::fft_run(field, d_pa, log_n, GH_FFT_INVERSE)))
        return rc;
    if ((rc = wait_timed())) return rc;
    return reduce_run<false>(d_pa, ta + tb - 1, n_out);      // the degrees add up: nothing above is non-zero
}

int evals_div_run(gh_field_t field, void* d_a, const void* d_b, size_t n, size_t* zero_divisors) {
    *zero_divisors = 0;
    if (!n) return GH_OK;
    if (int rc = reduce_run<true>(d_b, n, zero_divisors)) return rc;
    if (*zero_divisors) return GH_OK;
    uint8_t* d_inv;
    int rc;
    if ((rc = dbuf("poly_div_b", n * 96, &d_inv, 0)) || (rc = g_tm.begin().mark())) return rc;
    HIPCHK(hipMemcpyAsync(d_inv, d_b, n * 96, hipMemcpyDeviceToDevice, g.stream));
    if ((rc = gh_rt::batch_inverse(field, d_inv, n)) || (rc = gh_rt::vec_op(field, 0, d_a, d_inv, nullptr, n))) return rc;
    return wait_timed();
}

// host-buffer forms: a device copy of an input vector / the download of an output vector
int up(DevMem& m, const uint64_t* src, size_t rows) {
    if (int rc = m.alloc(std::max(rows, (size_t)1) * 96)) return rc;
    if (rows) HIPCHK(hipMemcpy(m.get(), src, rows * 96, hipMemcpyHostToDevice));
    return GH_OK;
}
int down(uint64_t* dst, const DevMem& m, size_t rows) {
    if (rows) HIPCHK(hipMemcpy(dst, m.get(), rows * 96, hipMemcpyDeviceToHost));
    return GH_OK;
}

// the checks every entry point starts with; `given`: a pointer that must not be null
int prologue(gh_field_t field, bool given, size_t n) {
    if (int rc = field_ok(field)) return rc;
    if (!given) return null_arg();
    return rows_ok(n);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using gh_rt::api_mutex;
using gh_rt::ensure_init;

extern "C" {

int gh_poly_evaluate_dev(gh_field_t field, const void* d_coeffs, size_t n, const uint64_t* points12, size_t k, uint64_t* out12) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (d_coeffs || !n) && (!k || (points12 && out12)), n)) return rc;
    if (k == 0) { g_err = "k: at least one point"; return GH_E_BAD_ARG; }
    if (k > 65535) { g_err = "k: at most 65535 points in one call"; return GH_E_BAD_ARG; }      // a point (or a group of them) per grid.y
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(field, evaluate_run, d_coeffs, n, points12, k, out12);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_evaluate(gh_field_t field, const uint64_t* coeffs, size_t n, const uint64_t* points12, size_t k, uint64_t* out12) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (coeffs || !n) && (!k || (points12 && out12)), n)) return rc;
    if (k == 0) { g_err = "k: at least one point"; return GH_E_BAD_ARG; }
    if (k > 65535) { g_err = "k: at most 65535 points in one call"; return GH_E_BAD_ARG; }      // a point (or a group of them) per grid.y
    if (int rc = ensure_init()) return rc;
    DevMem d;
    if (int rc = up(d, coeffs, n)) return rc;
    return GH_FIELD_DISPATCH(field, evaluate_run, d.get(), n, points12, k, out12);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_resize_dev(gh_field_t field, const void* d_in, size_t n, void* d_out, size_t n_out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (d_in || !n) && (d_out || !n_out), n | n_out)) return rc;
    if (!n_out) return GH_OK;
    if (int rc = ensure_init()) return rc;
    const size_t keep = std::min(n, n_out);
    if (int rc = g_tm.begin().mark()) return rc;
    if (keep) HIPCHK(hipMemcpyAsync(d_out, d_in, keep * 96, hipMemcpyDeviceToDevice, g.stream));
    if (n_out > keep) HIPCHK(hipMemsetAsync((uint8_t*)d_out + keep * 96, 0, (n_out - keep) * 96, g.stream));
    return wait_timed();
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_trimmed_len_dev(gh_field_t field, const void* d, size_t n, size_t* len) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (d || !n) && len, n)) return rc;
    if (int rc = ensure_init()) return rc;
    return reduce_run<false>(d, n, len);
} catch (...) { return gh_rt::api_exception(); }

static int axpy_api(gh_field_t field, int op, const void* d_a, size_t n_a, const void* d_b, size_t n_b, const uint64_t* f12, void* d_out) {
    std::lock_guard<std::mutex> lk(api_mutex());
    const bool given = (d_a || !n_a) && (d_b || !n_b) && (d_out || !(n_a | n_b)) && (op != POLY_ADD_SCALED || f12);
    if (int rc = prologue(field, given, n_a | n_b)) return rc;
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(field, axpy_run, op, d_a, n_a, d_b, n_b, f12, d_out);
}
int gh_poly_add_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, void* d_out) try {
    return axpy_api(field, POLY_ADD, d_a, n_a, d_b, n_b, nullptr, d_out);
} catch (...) { return gh_rt::api_exception(); }
int gh_poly_sub_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, void* d_out) try {
    return axpy_api(field, POLY_SUB, d_a, n_a, d_b, n_b, nullptr, d_out);
} catch (...) { return gh_rt::api_exception(); }
int gh_poly_add_scaled_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, const uint64_t* f12, void* d_out) try {
    return axpy_api(field, POLY_ADD_SCALED, d_a, n_a, d_b, n_b, f12, d_out);
} catch (...) { return gh_rt::api_exception(); }
int gh_poly_neg_dev(gh_field_t field, const void* d_a, size_t n, void* d_out) try {
    return axpy_api(field, POLY_NEG, d_a, n, nullptr, 0, nullptr, d_out);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_mul_by_vanishing_dev(gh_field_t field, const void* d_in, size_t n, uint32_t log_n, void* d_out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (d_in || !n) && d_out, n)) return rc;
    if (int rc = domain_ok(field, log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(field, mul_vanishing_run, d_in, n, log_n, d_out);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_divide_by_vanishing_dev(gh_field_t field, const void* d_in, size_t n, uint32_t log_n, void* d_q, void* d_r) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const bool has_q = log_n < 64 && n > ((size_t)1 << log_n);
    if (int rc = prologue(field, (d_in || !n) && d_r && (d_q || !has_q), n)) return rc;
    if (int rc = domain_ok(field, log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(field, divide_vanishing_run, d_in, n, log_n, d_q, d_r);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_divide_by_vanishing(gh_field_t field, const uint64_t* in, size_t n, uint32_t log_n, uint64_t* q, uint64_t* r) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    const bool has_q = log_n < 64 && n > ((size_t)1 << log_n);
    if (int rc = prologue(field, (in || !n) && r && (q || !has_q), n)) return rc;
    if (int rc = domain_ok(field, log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t N = (size_t)1 << log_n, nq = std::max(n, N) - N;
    DevMem d_in, d_q, d_r;
    int rc;
    if ((rc = up(d_in, in, n)) || (rc = d_q.alloc(std::max(nq, (size_t)1) * 96)) || (rc = d_r.alloc(N * 96))) return rc;
    if ((rc = GH_FIELD_DISPATCH(field, divide_vanishing_run, d_in.get(), n, log_n, d_q.get(), d_r.get()))) return rc;
    if ((rc = down(q, d_q, nq))) return rc;
    return down(r, d_r, N);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_divide_by_linear_dev(gh_field_t field, const void* d_in, size_t n, const uint64_t* z12, void* d_q, uint64_t* rem12) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (d_in || !n) && z12 && rem12 && (d_q || n < 2), n)) return rc;
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(field, divide_linear_run, d_in, n, z12, d_q, rem12);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_divide_by_linear(gh_field_t field, const uint64_t* in, size_t n, const uint64_t* z12, uint64_t* q, uint64_t* rem12) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (in || !n) && z12 && rem12 && (q || n < 2), n)) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t nq = std::max(n, (size_t)1) - 1;
    DevMem d_in, d_q;
    int rc;
    if ((rc = up(d_in, in, n)) || (rc = d_q.alloc(std::max(nq, (size_t)1) * 96))) return rc;
    if ((rc = GH_FIELD_DISPATCH(field, divide_linear_run, d_in.get(), n, z12, d_q.get(), rem12))) return rc;
    return down(q, d_q, nq);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_mul_dev(gh_field_t field, const void* d_a, size_t n_a, const void* d_b, size_t n_b, void* d_out, size_t out_cap, size_t* n_out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (d_a || !n_a) && (d_b || !n_b) && (d_out || !out_cap) && n_out, n_a | n_b)) return rc;
    if (int rc = ensure_init()) return rc;
    return mul_run(field, d_a, n_a, d_b, n_b, d_out, out_cap, n_out);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_mul(gh_field_t field, const uint64_t* a, size_t n_a, const uint64_t* b, size_t n_b, uint64_t* out, size_t out_cap, size_t* n_out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, (a || !n_a) && (b || !n_b) && (out || !out_cap) && n_out, n_a | n_b | out_cap)) return rc;
    if (int rc = ensure_init()) return rc;
    DevMem d_a, d_b, d_out;
    int rc;
    if ((rc = up(d_a, a, n_a)) || (rc = up(d_b, b, n_b)) || (rc = d_out.alloc(std::max(out_cap, (size_t)1) * 96))) return rc;
    if ((rc = mul_run(field, d_a.get(), n_a, d_b.get(), n_b, d_out.get(), out_cap, n_out))) return rc;
    return down(out, d_out, *n_out);
} catch (...) { return gh_rt::api_exception(); }

int gh_evals_div_dev(gh_field_t field, void* d_a, const void* d_b, size_t n, size_t* zero_divisors) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, ((d_a && d_b) || !n) && zero_divisors, n)) return rc;
    if (int rc = ensure_init()) return rc;
    return evals_div_run(field, d_a, d_b, n, zero_divisors);
} catch (...) { return gh_rt::api_exception(); }

int gh_domain_elements_dev(gh_field_t field, uint32_t log_n, void* d_out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, d_out != nullptr, 0)) return rc;
    if (int rc = domain_ok(field, log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(field, elements_run, field, log_n, d_out);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_sparse_evaluate_over_domain_dev(gh_field_t field, const uint64_t* exps, const uint64_t* coeffs12, size_t t, uint32_t log_n, void* d_out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (int rc = prologue(field, ((exps && coeffs12) || !t) && d_out, t)) return rc;
    if (int rc = domain_ok(field, log_n)) return rc;
    if (int rc = ensure_init()) return rc;
    return GH_FIELD_DISPATCH(field, sparse_run, field, exps, coeffs12, t, log_n, d_out);
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_set_tuning(uint32_t run_len, uint32_t direct_max, uint32_t seg_max) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!poly_tuning_ok(run_len, seg_max)) { g_err = "run_len and seg_max: 0 (the default) or at least 2"; return GH_E_BAD_ARG; }
    g_tune.run_len = run_len ? run_len : POLY_RUN_LEN;
    g_tune.direct_max = direct_max ? direct_max : POLY_DIRECT_MAX;
    g_tune.seg_max = seg_max ? seg_max : POLY_SEG_MAX;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poly_last_timing(float* ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (ms) *ms = g_tm.ms[0];
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
