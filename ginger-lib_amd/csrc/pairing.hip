// pairing.hip -- the C ABI of include/ginger_hip_pairing.h: batched MNT4-753 reduced ate pairings, one row per lane, and the
// Groth16 verifier built on them (proof-systems/src/groth16/verifier.rs).  DESIGN.md section 14.
//
// The arithmetic is pairing29.h.  A row's Miller value f (4 Fq, 104 words) lives in registers; the running G2 points of its
// variable pairs (Jacobian X, Y, Z, T: 8 Fq each) and what a pair brings to every step (x_Q, y_Q, x_P, 13 y_P) live in a per-row
// global slab, limb-major with the row index fastest like the slabs of vb_kernels.h, so a wave reads 256 consecutive bytes per
// limb.  A prepared Q (the verifying key's -gamma and -delta) is a table of 499 line coefficients in global memory that every
// lane reads at the same step.
//   pair_setup_kernel    ABI points -> the row's slab, the pair's skip flag (a point at infinity, or a row of status 2)
//   miller_kernel        KV variable + KP prepared pairs with one shared f: f is squared once per digit and multiplied by every
//                        pair's line.  The loop over the 376 signed digits is wave-uniform; only skipped pairs diverge.
//   final_exp_kernel     the reference's split final exponentiation, out in ABI form
//   g2_prepare_kernel    the two tables of a verifying key, one thread each, once per handle
#include <memory>
#include "vb_kernels.h"
#include "pairing29.h"
#include "../../include/ginger_hip_pairing.h"

struct gh_groth16_vk {
    static constexpr uint32_t MAGIC = 0x67684756u;
    uint32_t magic = MAGIC;
    size_t n_abc = 0;
    std::vector<uint64_t> gt;                      // alpha_g1_beta_g2: 48 words
    std::vector<uint64_t> g2_neg;                  // -gamma_g2, -delta_g2: 2 x 48 words
    std::vector<uint64_t> abc;                     // gamma_abc_g1: n_abc x 24 words
    gh_rt::DevMem d_tab;                           // 2 x TABLE_STEPS line coefficients, built on first use
    gh_rt::DevMem d_gt;                            // alpha_g1_beta_g2 on the device
    gh_rt::DevMem d_abc;                           // gamma_abc_g1 on the device (the variable-base rows)
    std::vector<gh_rt::FixedTable*> tables;        // the fixed-base table of gamma_abc_g1[j + 1], for the first n_tables inputs
    bool built = false;
    ~gh_groth16_vk() {
        for (auto* t : tables) gh_rt::fixed_table_destroy(t);
        magic = 0;
    }
};

namespace {

typedef Mnt4Pairing E4;
Timing g_tm{6};                                    // upload, g_ic, Miller loop, final exponentiation, compare, download

__constant__ int8_t c_ate_naf[GH_MNT4_ATE_DIGITS] = GH_MNT4_ATE_NAF;
__constant__ int8_t c_w0_naf[GH_MNT4_W0_DIGITS] = GH_MNT4_W0_NAF;

// slab slots of a row (one Fq each): variable pair j at VAR_SLOTS j, prepared pair j at VAR_SLOTS KV + PRE_SLOTS j
constexpr int VAR_SLOTS = 14;                      // X, Y, Z, T, x_Q, y_Q (2 each), x_P, 13 y_P
constexpr int PRE_SLOTS = 2;                       // x_P, 13 y_P
constexpr int MAX_PAIRS = 3;
constexpr size_t PAIR_SLAB_BYTES = (size_t)1 << 30;
// fixed-base tables of gamma_abc_g1: window 8 (95 rows of 256 affine points, 5 MB per input) for as many inputs as fit this
// bound; the inputs beyond it go through the variable-base kernels of vb_kernels.h
constexpr int ABC_WINDOW = 8;
constexpr size_t ABC_TABLE_BYTES = (size_t)1 << 30;
constexpr size_t ABC_TABLE_EACH = (size_t)((753 + ABC_WINDOW - 1) / ABC_WINDOW) * ((size_t)1 << ABC_WINDOW) * sizeof(Aff<Mnt4G1>);

// where the pairs of a launch come from: ABI words, row i of pair j at base[j] + i * stride[j]
struct PairIn {
    const uint32_t* g1[MAX_PAIRS];
    const uint8_t* g1_inf[MAX_PAIRS];
    size_t g1_stride[MAX_PAIRS], g1_inf_stride[MAX_PAIRS];
    const uint32_t* g2[MAX_PAIRS];                 // the variable pairs only
    const uint8_t* g2_inf[MAX_PAIRS];
    size_t g2_stride[MAX_PAIRS], g2_inf_stride[MAX_PAIRS];
};

__device__ __forceinline__ Fp2T ld2(const RowSlab& s, int slot) { return Fp2T{s.ld(slot), s.ld(slot + 1)}; }
__device__ __forceinline__ void st2(const RowSlab& s, int slot, const Fp2T& v) {
    s.st(slot, v.c0);
    s.st(slot + 1, v.c1);
}

template <class E, int KV, int KP>
__global__ void __launch_bounds__(BLOCK)
pair_setup_kernel(PairIn in, const uint8_t* __restrict__ status, size_t row0, size_t cnt, uint32_t* __restrict__ slab,
                  uint8_t* __restrict__ skip) {
    typedef typename E::PF PF;
    typedef typename E::B B;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const size_t i = row0 + t;
    const RowSlab s{slab + t, cnt};
    const bool dead = status && status[i] == 2;
#pragma unroll
    for (int j = 0; j < KV + KP; j++) {
        bool sk = dead || in.g1_inf[j][i * in.g1_inf_stride[j]] != 0;
        if (j < KV) sk = sk || in.g2_inf[j][i * in.g2_inf_stride[j]] != 0;
        skip[i * (KV + KP) + j] = sk;
        if (sk) continue;
        const uint32_t* p = in.g1[j] + i * in.g1_stride[j];
        const int base = j < KV ? VAR_SLOTS * j + 12 : VAR_SLOTS * KV + PRE_SLOTS * (j - KV);
        s.st(base, fp_from_abi<PF>(p));
        s.st(base + 1, E::mul13(fp_from_abi<PF>(p + 24)));
        if (j < KV) {
            const uint32_t* q = in.g2[j] + i * in.g2_stride[j];
            const Fp2T qx = B::from_abi(q), qy = B::from_abi(q + 48);
            st2(s, VAR_SLOTS * j, qx);
            st2(s, VAR_SLOTS * j + 2, qy);
            st2(s, VAR_SLOTS * j + 4, B::one());
            st2(s, VAR_SLOTS * j + 6, B::one());
            st2(s, VAR_SLOTS * j + 8, qx);
            st2(s, VAR_SLOTS * j + 10, qy);
        }
    }
}

template <class E, int KV, int KP>
__global__ void __launch_bounds__(BLOCK)
miller_kernel(uint32_t* __restrict__ slab, const uint8_t* __restrict__ skip, const typename E::Coeff* __restrict__ tab, size_t row0,
              size_t cnt, typename E::GT* __restrict__ out) {
    typedef typename E::B B;
    typedef typename E::GT GT;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const size_t i = row0 + t;
    const RowSlab s{slab + t, cnt};
    bool sk[KV + KP];
#pragma unroll
    for (int j = 0; j < KV + KP; j++) sk[j] = skip[i * (KV + KP) + j] != 0;
    GT f = E::one();
    // one step of every pair: add == 0 a doubling, +-1 an addition of +-Q; idx the step's entry of the prepared tables
    auto step = [&](int add, int idx) {
#pragma unroll
        for (int j = 0; j < KV; j++) {
            if (sk[j]) continue;
            const int b = VAR_SLOTS * j;
            typename E::G2Run R{ld2(s, b), ld2(s, b + 2), ld2(s, b + 4), ld2(s, b + 6)};
            const typename E::G1Pre P{s.ld(b + 12), s.ld(b + 13)};
            GT l;
            if (add == 0) {
                l = dbl_step_call<E>(R, P);
            } else {
                Fp2T qy = ld2(s, b + 10);
                if (add < 0) qy = B::neg(qy);
                l = add_step_call<E>(R, ld2(s, b + 8), qy, P);
            }
            st2(s, b, R.x);
            st2(s, b + 2, R.y);
            st2(s, b + 4, R.z);
            st2(s, b + 6, R.t);
            f = gt_mul_call<E>(f, l);
        }
#pragma unroll
        for (int j = 0; j < KP; j++) {
            if (sk[KV + j]) continue;
            const int b = VAR_SLOTS * KV + PRE_SLOTS * j;
            const typename E::G1Pre P{s.ld(b), s.ld(b + 1)};
            const typename E::Coeff c = ld_words(tab + (size_t)j * E::TABLE_STEPS + idx);
            f = gt_mul_by_023_call<E>(f, P.py13, E::prepared_line(c, P));
        }
    };
    int idx = 0;
#pragma unroll 1
    for (int d = 0; d < E::ATE_DIGITS; d++) {
        f = gt_sqr_call<E>(f);
        const int n = c_ate_naf[d];
#pragma unroll 1
        for (int h = 0; h < (n != 0 ? 2 : 1); h++) step(h ? n : 0, idx++);      // one inlined body for both kinds of step
    }
    st_words(out + i, E::unitary_inverse(f));      // the trace is negative (mod.rs:219-221)
}

template <class E>
__global__ void __launch_bounds__(BLOCK) final_exp_kernel(const typename E::GT* __restrict__ f, size_t n, uint32_t* __restrict__ out) {
    typedef typename E::PF PF;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const typename E::GT r = E::final_exponentiation(ld_words(f + i), c_w0_naf);
    uint32_t* o = out + i * 96;
    fp_to_abi<PF>(o, r.c0.c0);
    fp_to_abi<PF>(o + 24, r.c0.c1);
    fp_to_abi<PF>(o + 48, r.c1.c0);
    fp_to_abi<PF>(o + 72, r.c1.c1);
}

// the two tables of a verifying key: thread t prepares the point at g2 + 96 t (ABI words)
template <class E>
__global__ void __launch_bounds__(BLOCK) g2_prepare_kernel(const uint32_t* __restrict__ g2, int count, typename E::Coeff* __restrict__ tab) {
    typedef typename E::B B;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count) return;
    E::prepare_g2(B::from_abi(g2 + 96 * t), B::from_abi(g2 + 96 * t + 48), c_ate_naf, tab + (size_t)t * E::TABLE_STEPS);
}

// status 2 for a row with a proof point off its curve (the point at infinity is on it), else 0
template <class E>
__global__ void __launch_bounds__(BLOCK)
proof_check_kernel(const uint32_t* __restrict__ a, const uint8_t* __restrict__ a_inf, const uint32_t* __restrict__ b,
                   const uint8_t* __restrict__ b_inf, const uint32_t* __restrict__ c, const uint8_t* __restrict__ c_inf, size_t n, Fp b1,
                   Fp2T b2, uint8_t* __restrict__ status) {
    typedef typename E::PF PF;
    typedef typename E::B B;
    typedef typename E::G1::FC F;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    auto g1_ok = [&](const uint32_t* xy) {
        const Fp x = fp_from_abi<PF>(xy), y = fp_from_abi<PF>(xy + 24);
        return F::eq(F::sqr(y), F::add(F::add(F::mul(F::sqr(x), x), E::G1::mul_by_a(x)), b1));
    };
    bool ok = a_inf[i] || g1_ok(a + i * 48);
    ok = ok && (c_inf[i] || g1_ok(c + i * 48));
    if (ok && !b_inf[i]) {
        const Fp2T x = B::from_abi(b + i * 96), y = B::from_abi(b + i * 96 + 48);
        ok = B::eq(B::sqr(y), B::add(B::add(B::mul(B::sqr(x), x), E::G2::mul_by_a(x)), b2));
    }
    status[i] = ok ? 0 : 2;
}

// 1 if the row's value is the key's alpha_g1_beta_g2, 0 if not; rows of status 2 keep it
__global__ void __launch_bounds__(256) gt_compare_kernel(const uint64_t* __restrict__ val, const uint64_t* __restrict__ gt, size_t n,
                                                         uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status[i] == 2) return;
    bool eq = true;
    for (int w = 0; w < 48; w++) eq &= val[i * 48 + w] == gt[w];
    status[i] = eq;
}

// ---- g_ic
// public inputs (scalar-field Montgomery, row-major) -> canonical integers, input-major: out[j][i]
template <class PS>
__global__ void __launch_bounds__(256) inputs_to_int_kernel(const uint32_t* __restrict__ in, size_t n, size_t n_inputs, uint32_t* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_inputs) return;
    const size_t i = t / n_inputs, j = t % n_inputs;
    fp_to_int<PS>(out + (j * n + i) * 24, fp_from_abi<PS>(in + t * 24));
}
template <class C> __global__ void __launch_bounds__(256) fill_proj_kernel(Proj<C>* __restrict__ acc, size_t n, const uint32_t* __restrict__ xy) {
    typedef typename C::PF PF;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st_words(acc + i, Proj<C>{fp_from_abi<PF>(xy), fp_from_abi<PF>(xy + 24), C::FC::one()});
}
template <class C> __global__ void __launch_bounds__(BLOCK) proj_acc_kernel(Proj<C>* __restrict__ acc, const Proj<C>* __restrict__ b, size_t n) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    st_words(acc + i, proj_add_call<C>(ld_words(acc + i), ld_words(b + i)));
}
__global__ void __launch_bounds__(256) bcast_xy_kernel(const uint32_t* __restrict__ xy, size_t n, uint32_t* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 48) return;
    out[t] = xy[t % 48];
}

// ---------------------------------------------------------------------------------------------------- host side
// setup, Miller loop and final exponentiation of n rows on g.stream: d_val[i] = the row's value in ABI form (48 u64).  tab: the
// KP prepared tables.  The slab is cut into chunks below PAIR_SLAB_BYTES.
template <class E, int KV, int KP>
int launch_pairs(const PairIn& in, const uint8_t* d_status, const typename E::Coeff* tab, size_t n, uint64_t* d_val, Phases* ph) {
    constexpr size_t row_bytes = (size_t)(VAR_SLOTS * KV + PRE_SLOTS * KP) * NL * 4;
    const size_t chunk = slab_chunk_rows("launch_pairs", PAIR_SLAB_BYTES, row_bytes, n);
    uint32_t* slab;
    uint8_t* d_skip;
    typename E::GT* d_f;
    int rc = gh_rt::pool_get("vb_pair_slab", chunk * row_bytes, (void**)&slab);
    if (!rc) rc = dbuf("vb_pair_skip", n * (KV + KP), &d_skip);
    if (!rc) rc = dbuf("vb_pair_f", n, &d_f);
    if (rc) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t cnt = std::min(chunk, n - r0);
        GH_LAUNCH((pair_setup_kernel<E, KV, KP>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, in, d_status, r0, cnt, slab, d_skip);
        GH_LAUNCH((miller_kernel<E, KV, KP>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, slab, (const uint8_t*)d_skip, tab, r0, cnt, d_f);
    }
    HIPCHK(hipGetLastError());
    if (ph && (rc = ph->mark())) return rc;
    GH_LAUNCH((final_exp_kernel<E>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const typename E::GT*)d_f, n, (uint32_t*)d_val);
    HIPCHK(hipGetLastError());
    if (ph && (rc = ph->mark())) return rc;
    return GH_OK;
}

int run_product(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, size_t k, uint64_t* out_gt) {
    const size_t m = n * k;
    uint64_t *d_g1, *d_g2, *d_val;
    uint8_t *d_i1, *d_i2;
    int rc = dbuf("vb_pair_g1", m * 24, &d_g1);
    if (!rc) rc = dbuf("vb_pair_g2", m * 48, &d_g2);
    if (!rc) rc = dbuf("vb_pair_i1", m, &d_i1);
    if (!rc) rc = dbuf("vb_pair_i2", m, &d_i2);
    if (!rc) rc = dbuf("vb_pair_val", n * 48, &d_val);
    if (rc) return rc;
    Phases ph{g_tm};
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_g1, g1_xy, m * 24)) || (rc = up(d_g2, g2_xy, m * 48)) || (rc = up(d_i1, g1_inf, m)) || (rc = up(d_i2, g2_inf, m)) ||
        (rc = ph.mark()) || (rc = ph.mark()))                                                                    // no g_ic phase
        return rc;
    PairIn in{};
    for (size_t j = 0; j < k; j++) {
        in.g1[j] = (const uint32_t*)d_g1 + 48 * j;
        in.g1_inf[j] = d_i1 + j;
        in.g1_stride[j] = 48 * k;
        in.g1_inf_stride[j] = k;
        in.g2[j] = (const uint32_t*)d_g2 + 96 * j;
        in.g2_inf[j] = d_i2 + j;
        in.g2_stride[j] = 96 * k;
        in.g2_inf_stride[j] = k;
    }
    switch (k) {
        case 1: rc = launch_pairs<E4, 1, 0>(in, nullptr, nullptr, n, d_val, &ph); break;
        case 2: rc = launch_pairs<E4, 2, 0>(in, nullptr, nullptr, n, d_val, &ph); break;
        default: rc = launch_pairs<E4, 3, 0>(in, nullptr, nullptr, n, d_val, &ph); break;
    }
    if (rc || (rc = ph.mark())) return rc;                                                                        // no compare phase
    HIPCHK(hipMemcpyAsync(out_gt, d_val, n * 384, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    if ((rc = ph.finish())) return rc;
    g_tm.ms[1] = g_tm.ms[4] = 0;                                                                                  // phases this call does not have
    return GH_OK;
}

// how many of a key's inputs get a fixed-base table (GH_GROTH16_TABLES: a measurement and test knob, read when a key is first used)
size_t abc_table_count(size_t n_inputs) {
    const int knob = gh_rt::env_int("GH_GROTH16_TABLES", -1);
    const size_t fit = ABC_TABLE_BYTES / ABC_TABLE_EACH;
    return std::min(n_inputs, knob >= 0 ? (size_t)knob : fit);
}

// the device side of a key: the two prepared tables, alpha_g1_beta_g2, gamma_abc_g1 and its fixed-base tables
int vk_ensure(gh_groth16_vk* h) {
    if (h->built) return GH_OK;
    gh_rt::DevMem d_g2, d_tab, d_gt, d_abc;
    int rc;
    if ((rc = d_g2.alloc(2 * 384)) || (rc = d_tab.alloc(2 * E4::TABLE_STEPS * sizeof(E4::Coeff))) || (rc = d_gt.alloc(384)) ||
        (rc = d_abc.alloc(h->n_abc * 192)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_g2.get(), h->g2_neg.data(), 2 * 384, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_gt.get(), h->gt.data(), 384, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_abc.get(), h->abc.data(), h->n_abc * 192, hipMemcpyHostToDevice, g.stream));
    GH_LAUNCH((g2_prepare_kernel<E4>), dim3(1), dim3(BLOCK), 0, g.stream, d_g2.as<const uint32_t>(), 2, d_tab.as<E4::Coeff>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.stream));
    const size_t nt = abc_table_count(h->n_abc - 1);
    static const uint64_t one4[12] = GH_P4_R_64;
    while (h->tables.size() < nt) {
        uint64_t xyz[36];
        memcpy(xyz, h->abc.data() + 24 * (h->tables.size() + 1), 192);
        memcpy(xyz + 24, one4, 96);
        gh_rt::FixedTable* t = nullptr;
        if ((rc = gh_rt::fixed_table_create(GH_MNT4753_G1, xyz, VB_BITS, ABC_WINDOW, &t))) return rc;   // a later call resumes here
        h->tables.push_back(t);
    }
    h->d_tab = std::move(d_tab);
    h->d_gt = std::move(d_gt);
    h->d_abc = std::move(d_abc);
    h->built = true;
    return GH_OK;
}

// d_acc[i] = gamma_abc_g1[0] + sum_j inputs[i][j] gamma_abc_g1[j + 1], then affine in ABI form at d_xy / d_inf
int launch_g_ic(gh_groth16_vk* h, const uint64_t* d_inputs, size_t n, size_t n_inputs, uint64_t* d_xy, uint8_t* d_inf) {
    typedef Mnt4G1 C;
    Proj<C>*d_acc, *d_tmp;
    Fp* d_zp;
    uint32_t* d_k = nullptr;
    uint64_t* d_base = nullptr;
    int rc = dbuf("vb_p", n, &d_acc);
    if (!rc) rc = dbuf("vb_p2", n, &d_tmp);
    if (!rc) rc = dbuf("vb_zp", n, &d_zp);
    if (!rc && n_inputs) rc = dbuf("vb_pair_k", n * n_inputs * 24, &d_k);
    if (!rc && h->tables.size() < n_inputs) rc = dbuf("vb_pk", n * 24, &d_base);
    if (rc) return rc;
    const uint32_t* abc = h->d_abc.as<const uint32_t>();
    GH_LAUNCH((fill_proj_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, d_acc, n, abc);
    if (n_inputs)
        GH_LAUNCH((inputs_to_int_kernel<P6>), dim3(blocks(n * n_inputs, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_inputs, n, n_inputs, d_k);
    for (size_t j = 0; j < n_inputs; j++) {
        const uint32_t* kj = d_k + j * n * 24;
        if (j < h->tables.size()) {
            if ((rc = gh_rt::fixed_table_sums(h->tables[j], kj, n, d_tmp))) return rc;
        } else {
            GH_LAUNCH(bcast_xy_kernel, dim3(blocks(n * 48, 256)), dim3(256), 0, g.stream, abc + 48 * (j + 1), n, (uint32_t*)d_base);
            if ((rc = vb_single<C, 4>(d_base, nullptr, 0, &kj, &d_tmp, 1, n))) return rc;
        }
        GH_LAUNCH((proj_acc_kernel<C>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, d_acc, (const Proj<C>*)d_tmp, n);
    }
    if ((rc = launch_normalize<C>(d_acc, nullptr, n, d_zp, d_xy, 48, 0, d_inf))) return rc;
    HIPCHK(hipGetLastError());
    return GH_OK;
}

int run_verify(gh_groth16_vk* h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
               const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) {
    if (int rc = vk_ensure(h)) return rc;
    uint64_t *d_a, *d_b, *d_c, *d_in = nullptr, *d_gic, *d_val;
    uint8_t *d_ai, *d_bi, *d_ci, *d_gi, *d_st;
    int rc = dbuf("vb_pair_g1", n * 24, &d_a);
    if (!rc) rc = dbuf("vb_pair_g2", n * 48, &d_b);
    if (!rc) rc = dbuf("vb_pair_c", n * 24, &d_c);
    if (!rc) rc = dbuf("vb_pair_i1", n, &d_ai);
    if (!rc) rc = dbuf("vb_pair_i2", n, &d_bi);
    if (!rc) rc = dbuf("vb_pair_i3", n, &d_ci);
    if (!rc && n_inputs) rc = dbuf("vb_pair_in", n * n_inputs * 12, &d_in);
    if (!rc) rc = dbuf("vb_xy", n * 24, &d_gic);
    if (!rc) rc = dbuf("vb_inf", n, &d_gi);
    if (!rc) rc = dbuf("vb_pair_val", n * 48, &d_val);
    if (!rc) rc = dbuf("vb_st", n, &d_st);
    if (rc) return rc;
    Phases ph{g_tm};
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_a, a_xy, n * 24)) || (rc = up(d_b, b_xy, n * 48)) || (rc = up(d_c, c_xy, n * 24)) || (rc = up(d_ai, a_inf, n)) ||
        (rc = up(d_bi, b_inf, n)) || (rc = up(d_ci, c_inf, n)) || (n_inputs && (rc = up(d_in, inputs, n * n_inputs * 12))) || (rc = ph.mark()))
        return rc;
    static const uint64_t b2w[12] = GH_MNT4753_G2_B1_M_64;
    const Fp2T b2{fp_zero(), fp_from_abi<P4>((const uint32_t*)b2w)};
    GH_LAUNCH((proof_check_kernel<E4>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_a, (const uint8_t*)d_ai,
              (const uint32_t*)d_b, (const uint8_t*)d_bi, (const uint32_t*)d_c, (const uint8_t*)d_ci, n, curve_b<Mnt4G1>(), b2, d_st);
    if ((rc = launch_g_ic(h, d_in, n, n_inputs, d_gic, d_gi)) || (rc = ph.mark())) return rc;
    PairIn in{};
    const uint64_t* g1s[3] = {d_a, d_gic, d_c};
    const uint8_t* infs[3] = {d_ai, d_gi, d_ci};
    for (int j = 0; j < 3; j++) {
        in.g1[j] = (const uint32_t*)g1s[j];
        in.g1_inf[j] = infs[j];
        in.g1_stride[j] = 48;
        in.g1_inf_stride[j] = 1;
    }
    in.g2[0] = (const uint32_t*)d_b;
    in.g2_inf[0] = d_bi;
    in.g2_stride[0] = 96;
    in.g2_inf_stride[0] = 1;
    if ((rc = launch_pairs<E4, 1, 2>(in, d_st, h->d_tab.as<const E4::Coeff>(), n, d_val, &ph))) return rc;
    GH_LAUNCH(gt_compare_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_val, h->d_gt.as<const uint64_t>(), n, d_st);
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

// ---- host checks of a key's points (the same GH_HD arithmetic, on the host)
bool g1_on_curve(const uint64_t* xy) {
    typedef Mnt4G1::FC F;
    const Fp x = fp_from_abi<P4>((const uint32_t*)xy), y = fp_from_abi<P4>((const uint32_t*)(xy + 12));
    return F::eq(F::sqr(y), F::add(F::add(F::mul(F::sqr(x), x), Mnt4G1::mul_by_a(x)), curve_b<Mnt4G1>()));
}
bool g2_on_curve(const uint64_t* xy) {
    typedef E4::B B;
    static const uint64_t b2w[12] = GH_MNT4753_G2_B1_M_64;
    const Fp2T b2{fp_zero(), fp_from_abi<P4>((const uint32_t*)b2w)};
    const Fp2T x = B::from_abi((const uint32_t*)xy), y = B::from_abi((const uint32_t*)(xy + 24));
    return B::eq(B::sqr(y), B::add(B::add(B::mul(B::sqr(x), x), Mnt4G2::mul_by_a(x)), b2));
}
void g2_negate(uint64_t* out, const uint64_t* xy) {
    typedef E4::B B;
    memcpy(out, xy, 192);
    B::to_abi((uint32_t*)(out + 24), B::neg(B::from_abi((const uint32_t*)(xy + 24))));
}

int checked_handle(gh_groth16_vk* h) {
    if (!h || h->magic != gh_groth16_vk::MAGIC) { g_err = "not a Groth16 verifying key"; return GH_E_BAD_HANDLE; }
    return GH_OK;
}
int check_engine(int engine) {
    if (engine != GH_PAIRING_MNT4753) { g_err = "unknown pairing engine"; return GH_E_BAD_ARG; }
    return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

extern "C" {

int gh_pairing_product(int engine, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
                       size_t k, uint64_t* out_gt) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = check_engine(engine)) return rc;
    if (k < 1 || k > MAX_PAIRS) { g_err = "the number of pairs per row must be 1, 2 or 3"; return GH_E_BAD_ARG; }
    if (n && (!g1_xy || !g1_inf || !g2_xy || !g2_inf || !out_gt)) { g_err = "null argument"; return GH_E_BAD_ARG; }
    size_t b;
    if (mul_overflows(n, 4096, &b)) { g_err = "input too large"; return GH_E_BAD_ARG; }
    if (!all_below<P4>(g1_xy, 2 * n * k) || !all_below<P4>(g2_xy, 4 * n * k)) { g_err = "a coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return run_product(g1_xy, g1_inf, g2_xy, g2_inf, n, k, out_gt);
} catch (...) { return gh_rt::api_exception(); }

int gh_groth16_vk_create(int engine, const uint64_t* alpha_g1_beta_g2, const uint64_t* gamma_g2_xy, const uint64_t* delta_g2_xy,
                         const uint64_t* gamma_abc_g1_xy, size_t n_abc, gh_groth16_vk_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!out) { g_err = "null argument"; return GH_E_BAD_ARG; }
    *out = nullptr;
    if (int rc = check_engine(engine)) return rc;
    if (!alpha_g1_beta_g2 || !gamma_g2_xy || !delta_g2_xy || !gamma_abc_g1_xy) { g_err = "null argument"; return GH_E_BAD_ARG; }
    size_t b;
    if (n_abc == 0 || mul_overflows(n_abc, 4096, &b)) { g_err = "gamma_abc_g1 must hold at least one point"; return GH_E_BAD_ARG; }
    if (!all_below<P4>(alpha_g1_beta_g2, 4) || !all_below<P4>(gamma_g2_xy, 4) || !all_below<P4>(delta_g2_xy, 4) ||
        !all_below<P4>(gamma_abc_g1_xy, 2 * n_abc)) {
        g_err = "a coefficient of the verifying key is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (!g2_on_curve(gamma_g2_xy) || !g2_on_curve(delta_g2_xy)) { g_err = "gamma_g2 or delta_g2 is not on the curve"; return GH_E_BAD_ARG; }
    for (size_t j = 0; j < n_abc; j++)
        if (!g1_on_curve(gamma_abc_g1_xy + 24 * j)) { g_err = "a point of gamma_abc_g1 is not on the curve"; return GH_E_BAD_ARG; }
    std::unique_ptr<gh_groth16_vk> h(new gh_groth16_vk());
    h->n_abc = n_abc;
    h->gt.assign(alpha_g1_beta_g2, alpha_g1_beta_g2 + 48);
    h->g2_neg.resize(96);
    g2_negate(h->g2_neg.data(), gamma_g2_xy);
    g2_negate(h->g2_neg.data() + 48, delta_g2_xy);
    h->abc.assign(gamma_abc_g1_xy, gamma_abc_g1_xy + 24 * n_abc);
    *out = h.release();
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_groth16_vk_free(gh_groth16_vk_t h) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!h) return GH_OK;
    if (int rc = checked_handle(h)) return rc;
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_groth16_verify(gh_groth16_vk_t h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                      const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    if (n_inputs + 1 != h->n_abc) { g_err = "the number of public inputs does not match gamma_abc_g1 (MalformedVerifyingKey)"; return GH_E_BAD_ARG; }
    if (n && (!a_xy || !a_inf || !b_xy || !b_inf || !c_xy || !c_inf || (n_inputs && !inputs) || !out_status)) {
        g_err = "null argument";
        return GH_E_BAD_ARG;
    }
    size_t ni = 0, b = 0;
    if (mul_overflows(n, n_inputs, &ni) || mul_overflows(ni, 96 * 4, &b) || mul_overflows(n, 4096, &b)) { g_err = "input too large"; return GH_E_BAD_ARG; }
    if (!all_below<P4>(a_xy, 2 * n) || !all_below<P4>(b_xy, 4 * n) || !all_below<P4>(c_xy, 2 * n)) {
        g_err = "a proof coordinate is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (n_inputs && !all_below<P6>(inputs, ni)) { g_err = "a public input is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return run_verify(h, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_pairing_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return g_tm.copy_out(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
