// pairing_impl.h -- batched reduced ate pairings, one row per lane, and the Groth16 verifier built on them
// (proof-systems/src/groth16/verifier.rs), as templates over the engine policy E: Mnt4Pairing (pairing29.h, instantiated by
// pairing.hip) or Mnt6Pairing (pairing29_mnt6.h, pairing_mnt6753.hip).  Each unit ends with GH_DEFINE_PAIRING_OPS, and the C ABI
// of pairing.hip reaches an engine through its PairingOps, as the MSM reaches a curve through msm_impl.h.  DESIGN.md section 14.
//
// Everything that counts Fq words comes from the engine: D = E::BDEG is the degree of the tower's base over Fq (2 or 3), a G2
// coordinate and half a GT element are D Fq, a G2 point and a GT element 24 D ABI words.  A row's Miller value f (2 D Fq)
// lives in registers; the running G2 points of its variable pairs (Jacobian X, Y, Z, T: 4 D Fq each) and what a pair brings to
// every step (x_Q, y_Q, x_P and the line's Fq factor: 13 y_P on MNT4, y_P on MNT6) live in a per-row global slab, limb-major
// with the row index fastest like the slabs of vb_kernels.h, so a wave reads 256 consecutive bytes per limb.  A prepared Q
// (the verifying key's -gamma and -delta) is a table of 499 line coefficients in global memory that every lane reads at the
// same step.
//   pair_setup_kernel    ABI points -> the row's slab, the pair's skip flag (a point at infinity, or a row of status 2 or 3)
//   miller_kernel        KV variable + KP prepared pairs with one shared f: f is squared once per digit and multiplied by every
//                        pair's line.  The loop over the 376 signed digits is wave-uniform; only skipped pairs diverge.
//   final_exp_kernel     the reference's split final exponentiation, out in ABI form
//   g2_prepare_kernel    the two tables of a verifying key, one thread each, once per handle
#pragma once
#include <memory>
#include "vb_kernels.h"
#include "pairing29_mnt6.h"
#include "../../include/ginger_hip_pairing.h"
#include "../../include/ginger_hip_points.h"

struct gh_groth16_vk {
    static constexpr uint32_t MAGIC = 0x67684756u;
    uint32_t magic = MAGIC;
    int engine = GH_PAIRING_MNT4753;               // GH_PAIRING_*: which PairingOps verify with this key
    size_t n_abc = 0;
    std::vector<uint64_t> gt;                      // alpha_g1_beta_g2: 24 D words
    std::vector<uint64_t> g2_neg;                  // -gamma_g2, -delta_g2: 2 x 24 D words
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

struct gh_gm17_vk;                                 // gm17_verify_impl.h

// what the C ABI calls for a key's or a call's engine: the bodies of the entry points after the lock and the engine check
namespace gh_rt {
struct PairingOps {
    int (*product)(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, size_t k, uint64_t* out_gt);
    int (*vk_create)(int engine, const uint64_t* alpha_g1_beta_g2, const uint64_t* gamma_g2_xy, const uint64_t* delta_g2_xy,
                     const uint64_t* gamma_abc_g1_xy, size_t n_abc, gh_groth16_vk** out);
    int (*verify)(gh_groth16_vk* h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                  const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status);
    int (*last_timing)(float* phase_ms, int max_phases, float* total_ms);
    // include/ginger_hip_points.h: verify after the membership test of A, B, C (compressed == 0: the points as for verify) or
    // after their decompression (compressed != 0: a, b, c hold canonical x, the *_inf arguments the flags bytes)
    int (*verify_validated)(gh_groth16_vk* h, int compressed, const uint64_t* a, const uint8_t* a_inf, const uint64_t* b, const uint8_t* b_inf,
                            const uint64_t* c, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status,
                            uint8_t* out_point_status);
    // the GM17 verifier of gm17_verify_impl.h (include/ginger_hip_gm17.h)
    int (*gm17_vk_create)(int engine, const uint64_t* g_alpha_g1_xy, const uint64_t* h_beta_g2_xy, const uint64_t* g_gamma_g1_xy,
                          const uint64_t* h_gamma_g2_xy, const uint64_t* h_g2_xy, const uint64_t* query_g1_xy, size_t n_query, gh_gm17_vk** out);
    int (*gm17_verify)(gh_gm17_vk* h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                       const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status);
    int (*gm17_last_timing)(float* phase_ms, int max_phases, float* total_ms);
};
const PairingOps* pairing_ops_mnt4753();
const PairingOps* pairing_ops_mnt6753();
}  // namespace gh_rt

namespace {

PhaseTimer g_tm{6};                                // upload, g_ic, Miller loop, final exponentiation, compare, download

// the signed digits of an engine's loop count and of its w0, most significant first
__constant__ int8_t c_ate_naf4[GH_MNT4_ATE_DIGITS] = GH_MNT4_ATE_NAF;
__constant__ int8_t c_w0_naf4[GH_MNT4_W0_DIGITS] = GH_MNT4_W0_NAF;
__constant__ int8_t c_ate_naf6[GH_MNT6_ATE_DIGITS] = GH_MNT6_ATE_NAF;
__constant__ int8_t c_w0_naf6[GH_MNT6_W0_DIGITS] = GH_MNT6_W0_NAF;
template <class E> __device__ __forceinline__ const int8_t* ate_naf();
template <class E> __device__ __forceinline__ const int8_t* w0_naf();
template <> __device__ __forceinline__ const int8_t* ate_naf<Mnt4Pairing>() { return c_ate_naf4; }
template <> __device__ __forceinline__ const int8_t* w0_naf<Mnt4Pairing>() { return c_w0_naf4; }
template <> __device__ __forceinline__ const int8_t* ate_naf<Mnt6Pairing>() { return c_ate_naf6; }
template <> __device__ __forceinline__ const int8_t* w0_naf<Mnt6Pairing>() { return c_w0_naf6; }

// the host's side of an engine: PS the scalar field of the public inputs, the G1 curve of the g_ic tables, the name under which
// launch_pairs reports its chunks (GH_TEST_SLAB_ROWS), one in Montgomery form, and the twist's b
template <class E> struct EngineHost;
template <> struct EngineHost<Mnt4Pairing> {
    typedef P6 PS;
    static constexpr gh_curve_t g1_curve = GH_MNT4753_G1;
    static constexpr const char* pairs_loop = "launch_pairs";
    static const uint64_t* one() { static const uint64_t v[12] = GH_P4_R_64; return v; }
    static Fp2T g2_b() {
        static const uint64_t b2w[12] = GH_MNT4753_G2_B1_M_64;
        return Fp2T{fp_zero(), fp_from_abi<P4>((const uint32_t*)b2w)};
    }
};
template <> struct EngineHost<Mnt6Pairing> {
    typedef P4 PS;
    static constexpr gh_curve_t g1_curve = GH_MNT6753_G1;
    static constexpr const char* pairs_loop = "launch_pairs_mnt6";
    static const uint64_t* one() { static const uint64_t v[12] = GH_P6_R_64; return v; }
    static Fp3T g2_b() {
        static const uint64_t b0[12] = GH_MNT6753_G2_B0_M_64, b1[12] = GH_MNT6753_G2_B1_M_64, b2[12] = GH_MNT6753_G2_B2_M_64;
        return Fp3T{fp_from_abi<P6>((const uint32_t*)b0), fp_from_abi<P6>((const uint32_t*)b1), fp_from_abi<P6>((const uint32_t*)b2)};
    }
};

// slab slots of a row (one Fq each): variable pair j at var_slots j, prepared pair j at var_slots KV + PRE_SLOTS j.  A variable
// pair: X, Y, Z, T, x_Q, y_Q (D each) at 0, D .. 5 D, then x_P and the line's Fq factor: 14 slots on MNT4, 20 on MNT6
template <class E> constexpr int var_slots() { return 6 * E::BDEG + 2; }
constexpr int PRE_SLOTS = 2;                       // x_P, the line's Fq factor
// ABI words (u32) of a G2 point and of a GT element; a G2 coordinate and half a GT element are half of it
template <class E> constexpr int tower_words() { return 48 * E::BDEG; }
constexpr int MAX_PAIRS = 3;
constexpr size_t PAIR_SLAB_BYTES = (size_t)1 << 30;
// fixed-base tables of gamma_abc_g1: window 8 (95 rows of 256 affine points, 5 MB per input) for as many inputs as fit this
// bound; the inputs beyond it go through the variable-base kernels of vb_kernels.h
constexpr int ABC_WINDOW = 8;
constexpr size_t ABC_TABLE_BYTES = (size_t)1 << 30;
constexpr size_t ABC_TABLE_EACH = (size_t)((753 + ABC_WINDOW - 1) / ABC_WINDOW) * ((size_t)1 << ABC_WINDOW) * sizeof(Aff<Mnt4G1>);
static_assert(sizeof(Aff<Mnt6G1>) == sizeof(Aff<Mnt4G1>), "one table size for both G1");

// where the pairs of a launch come from: ABI words, row i of pair j at base[j] + i * stride[j]
struct PairIn {
    const uint32_t* g1[MAX_PAIRS];
    const uint8_t* g1_inf[MAX_PAIRS];
    size_t g1_stride[MAX_PAIRS], g1_inf_stride[MAX_PAIRS];
    const uint32_t* g2[MAX_PAIRS];                 // the variable pairs only
    const uint8_t* g2_inf[MAX_PAIRS];
    size_t g2_stride[MAX_PAIRS], g2_inf_stride[MAX_PAIRS];
    // pair j takes its G1 / G2 point of row i from xy + i * stride (u32 words; 0: one point for every row) and the point's
    // infinity byte from inf[i * inf_stride]
    void g1_rows(int j, const void* xy, const uint8_t* inf, size_t stride = 48, size_t inf_stride = 1) {
        g1[j] = (const uint32_t*)xy;
        g1_inf[j] = inf;
        g1_stride[j] = stride;
        g1_inf_stride[j] = inf_stride;
    }
    void g2_rows(int j, const void* xy, const uint8_t* inf, size_t stride, size_t inf_stride = 1) {
        g2[j] = (const uint32_t*)xy;
        g2_inf[j] = inf;
        g2_stride[j] = stride;
        g2_inf_stride[j] = inf_stride;
    }
};

// a tower coordinate in B::DEG consecutive slots
template <class B> __device__ __forceinline__ typename B::T ld_t(const RowSlab& s, int slot) {
    if constexpr (B::DEG == 2) return typename B::T{s.ld(slot), s.ld(slot + 1)};
    else return typename B::T{s.ld(slot), s.ld(slot + 1), s.ld(slot + 2)};
}
template <class B> __device__ __forceinline__ void st_t(const RowSlab& s, int slot, const typename B::T& v) {
#pragma unroll
    for (int i = 0; i < B::DEG; i++) s.st(slot + i, B::comp(v, i));
}

template <class E, int KV, int KP>
__global__ void __launch_bounds__(BLOCK)
pair_setup_kernel(PairIn in, const uint8_t* __restrict__ status, size_t row0, size_t cnt, uint32_t* __restrict__ slab,
                  uint8_t* __restrict__ skip) {
    typedef typename E::PF PF;
    typedef typename E::B B;
    constexpr int D = E::BDEG, VS = var_slots<E>();
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const size_t i = row0 + t;
    const RowSlab s{slab + t, cnt};
    const bool dead = status && status[i] >= 2;               // 2: a point off its curve, 3: a point failed validation
#pragma unroll
    for (int j = 0; j < KV + KP; j++) {
        bool sk = dead || in.g1_inf[j][i * in.g1_inf_stride[j]] != 0;
        if (j < KV) sk = sk || in.g2_inf[j][i * in.g2_inf_stride[j]] != 0;
        skip[i * (KV + KP) + j] = sk;
        if (sk) continue;
        const uint32_t* p = in.g1[j] + i * in.g1_stride[j];
        const int base = j < KV ? VS * j + 6 * D : VS * KV + PRE_SLOTS * (j - KV);
        const typename E::G1Pre pre = E::g1_pre(fp_from_abi<PF>(p), fp_from_abi<PF>(p + 24));
        s.st(base, pre.px);
        s.st(base + 1, E::line_c0(pre));
        if (j < KV) {
            const uint32_t* q = in.g2[j] + i * in.g2_stride[j];
            const typename B::T qx = B::from_abi(q), qy = B::from_abi(q + tower_words<E>() / 2);
            st_t<B>(s, VS * j, qx);
            st_t<B>(s, VS * j + D, qy);
            st_t<B>(s, VS * j + 2 * D, B::one());
            st_t<B>(s, VS * j + 3 * D, B::one());
            st_t<B>(s, VS * j + 4 * D, qx);
            st_t<B>(s, VS * j + 5 * D, qy);
        }
    }
}

template <class E, int KV, int KP>
__global__ void __launch_bounds__(BLOCK)
miller_kernel(uint32_t* __restrict__ slab, const uint8_t* __restrict__ skip, const typename E::Coeff* __restrict__ tab, size_t row0,
              size_t cnt, typename E::GT* __restrict__ out) {
    typedef typename E::B B;
    typedef typename B::T BT;
    typedef typename E::GT GT;
    constexpr int D = E::BDEG, VS = var_slots<E>();
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
            const int b = VS * j;
            typename E::G2Run R{ld_t<B>(s, b), ld_t<B>(s, b + D), ld_t<B>(s, b + 2 * D), ld_t<B>(s, b + 3 * D)};
            const typename E::G1Pre P{s.ld(b + 6 * D), s.ld(b + 6 * D + 1)};
            GT l;
            if (add == 0) {
                l = dbl_step_call<E>(R, P);
            } else {
                BT qy = ld_t<B>(s, b + 5 * D);
                if (add < 0) qy = B::neg(qy);
                l = add_step_call<E>(R, ld_t<B>(s, b + 4 * D), qy, P);
            }
            st_t<B>(s, b, R.x);
            st_t<B>(s, b + D, R.y);
            st_t<B>(s, b + 2 * D, R.z);
            st_t<B>(s, b + 3 * D, R.t);
            f = gt_mul_call<E>(f, l);
        }
#pragma unroll
        for (int j = 0; j < KP; j++) {
            if (sk[KV + j]) continue;
            const int b = VS * KV + PRE_SLOTS * j;
            const typename E::G1Pre P{s.ld(b), s.ld(b + 1)};
            const typename E::Coeff c = ld_words(tab + (size_t)j * E::TABLE_STEPS + idx);
            f = gt_mul_by_line_call<E>(f, E::line_c0(P), E::prepared_line(c, P));
        }
    };
    int idx = 0;
#pragma unroll 1
    for (int d = 0; d < E::ATE_DIGITS; d++) {
        f = gt_sqr_call<E>(f);
        const int n = ate_naf<E>()[d];
#pragma unroll 1
        for (int h = 0; h < (n != 0 ? 2 : 1); h++) step(h ? n : 0, idx++);      // one inlined body for both kinds of step
    }
    st_words(out + i, E::miller_end(f));           // MNT4: the trace is negative (mnt4/mod.rs:219-221)
}

template <class E>
__global__ void __launch_bounds__(BLOCK) final_exp_kernel(const typename E::GT* __restrict__ f, size_t n, uint32_t* __restrict__ out) {
    typedef typename E::B B;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const typename E::GT r = E::final_exponentiation(ld_words(f + i), w0_naf<E>());
    uint32_t* o = out + i * tower_words<E>();
    B::to_abi(o, r.c0);
    B::to_abi(o + tower_words<E>() / 2, r.c1);
}

// the two tables of a verifying key: thread t prepares the point at g2 + 48 D t (ABI words)
template <class E>
__global__ void __launch_bounds__(BLOCK) g2_prepare_kernel(const uint32_t* __restrict__ g2, int count, typename E::Coeff* __restrict__ tab) {
    typedef typename E::B B;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count) return;
    constexpr int W = tower_words<E>();
    E::prepare_g2(B::from_abi(g2 + W * t), B::from_abi(g2 + W * t + W / 2), ate_naf<E>(), tab + (size_t)t * E::TABLE_STEPS);
}

// status 2 for a row with a proof point off its curve (the point at infinity is on it), else 0
template <class E>
__global__ void __launch_bounds__(BLOCK)
proof_check_kernel(const uint32_t* __restrict__ a, const uint8_t* __restrict__ a_inf, const uint32_t* __restrict__ b,
                   const uint8_t* __restrict__ b_inf, const uint32_t* __restrict__ c, const uint8_t* __restrict__ c_inf, size_t n, Fp b1,
                   typename E::B::T b2, uint8_t* __restrict__ status) {
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
        constexpr int W = tower_words<E>();
        const typename B::T x = B::from_abi(b + i * W), y = B::from_abi(b + i * W + W / 2);
        ok = B::eq(B::sqr(y), B::add(B::add(B::mul(B::sqr(x), x), E::G2::mul_by_a(x)), b2));
    }
    status[i] = ok ? 0 : 2;
}

// status 3 (GH_VERIFY_INVALID_POINT) for a row with a non-zero point code (pst: 3 per row, A, B, C), over what proof_check_kernel wrote
__global__ void __launch_bounds__(256) point_status_kernel(const uint8_t* __restrict__ pst, size_t n, uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (pst[3 * i] | pst[3 * i + 1] | pst[3 * i + 2]) status[i] = GH_VERIFY_INVALID_POINT;
}

// 1 if the row's value (W u64 words) is the key's alpha_g1_beta_g2, 0 if not; rows of status 2 and 3 keep it
template <int W>
__global__ void __launch_bounds__(256) gt_compare_kernel(const uint64_t* __restrict__ val, const uint64_t* __restrict__ gt, size_t n,
                                                         uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status[i] >= 2) return;
    bool eq = true;
    for (int w = 0; w < W; w++) eq &= val[i * W + w] == gt[w];
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
// setup, Miller loop and final exponentiation of n rows on g.stream: d_val[i] = the row's value in ABI form (24 D u64).  tab: the
// KP prepared tables.  The slab is cut into chunks below PAIR_SLAB_BYTES.
template <class E, int KV, int KP>
int launch_pairs(const PairIn& in, const uint8_t* d_status, const typename E::Coeff* tab, size_t n, uint64_t* d_val, PhaseTimer* ph) {
    constexpr size_t row_bytes = (size_t)(var_slots<E>() * KV + PRE_SLOTS * KP) * NL * 4;
    const size_t chunk = slab_chunk_rows(EngineHost<E>::pairs_loop, PAIR_SLAB_BYTES, row_bytes, n);
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

template <class E>
int run_product(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, size_t k, uint64_t* out_gt) {
    constexpr size_t TW = tower_words<E>() / 2;    // u64 words of a G2 point and of a GT element
    const size_t m = n * k;
    uint64_t *d_g1, *d_g2, *d_val;
    uint8_t *d_i1, *d_i2;
    int rc = dbuf("vb_pair_g1", m * 24, &d_g1);
    if (!rc) rc = dbuf("vb_pair_g2", m * TW, &d_g2);
    if (!rc) rc = dbuf("vb_pair_i1", m, &d_i1);
    if (!rc) rc = dbuf("vb_pair_i2", m, &d_i2);
    if (!rc) rc = dbuf("vb_pair_val", n * TW, &d_val);
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_g1, g1_xy, m * 24)) || (rc = up(d_g2, g2_xy, m * TW)) || (rc = up(d_i1, g1_inf, m)) || (rc = up(d_i2, g2_inf, m)) ||
        (rc = ph.mark()) || (rc = ph.mark()))                                                                    // no g_ic phase
        return rc;
    PairIn in{};
    for (size_t j = 0; j < k; j++) {
        in.g1_rows(j, d_g1 + 24 * j, d_i1 + j, 48 * k, k);
        in.g2_rows(j, d_g2 + TW * j, d_i2 + j, 2 * TW * k, k);
    }
    switch (k) {
        case 1: rc = launch_pairs<E, 1, 0>(in, nullptr, nullptr, n, d_val, &ph); break;
        case 2: rc = launch_pairs<E, 2, 0>(in, nullptr, nullptr, n, d_val, &ph); break;
        default: rc = launch_pairs<E, 3, 0>(in, nullptr, nullptr, n, d_val, &ph); break;
    }
    if (rc || (rc = ph.mark())) return rc;                                                                        // no compare phase
    HIPCHK(hipMemcpyAsync(out_gt, d_val, n * TW * 8, hipMemcpyDeviceToHost, g.stream));
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

// the fixed-base tables of the points after the first of `pts` (n_pts x 24 words, ABI), for as many as abc_table_count allows; a
// later call resumes where an earlier one failed
template <class E> int ensure_abc_tables(const uint64_t* pts, size_t n_pts, std::vector<gh_rt::FixedTable*>& tables) {
    const size_t nt = abc_table_count(n_pts - 1);
    while (tables.size() < nt) {
        uint64_t xyz[36];
        memcpy(xyz, pts + 24 * (tables.size() + 1), 192);
        memcpy(xyz + 24, EngineHost<E>::one(), 96);
        gh_rt::FixedTable* t = nullptr;
        if (int rc = gh_rt::fixed_table_create(EngineHost<E>::g1_curve, xyz, VB_BITS, ABC_WINDOW, &t)) return rc;
        tables.push_back(t);
    }
    return GH_OK;
}

// the device side of a key: the two prepared tables, alpha_g1_beta_g2, gamma_abc_g1 and its fixed-base tables
template <class E> int vk_ensure(gh_groth16_vk* h) {
    if (h->built) return GH_OK;
    constexpr size_t TB = tower_words<E>() * 4;    // bytes of a G2 point and of a GT element
    gh_rt::DevMem d_g2, d_tab, d_gt, d_abc;
    int rc;
    if ((rc = d_g2.alloc(2 * TB)) || (rc = d_tab.alloc(2 * E::TABLE_STEPS * sizeof(typename E::Coeff))) || (rc = d_gt.alloc(TB)) ||
        (rc = d_abc.alloc(h->n_abc * 192)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_g2.get(), h->g2_neg.data(), 2 * TB, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_gt.get(), h->gt.data(), TB, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_abc.get(), h->abc.data(), h->n_abc * 192, hipMemcpyHostToDevice, g.stream));
    GH_LAUNCH((g2_prepare_kernel<E>), dim3(1), dim3(BLOCK), 0, g.stream, d_g2.as<const uint32_t>(), 2, d_tab.as<typename E::Coeff>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.stream));
    if ((rc = ensure_abc_tables<E>(h->abc.data(), h->n_abc, h->tables))) return rc;
    h->d_tab = std::move(d_tab);
    h->d_gt = std::move(d_gt);
    h->d_abc = std::move(d_abc);
    h->built = true;
    return GH_OK;
}

// d_acc[i] = abc[0] + sum_j inputs[i][j] abc[j + 1], then affine in ABI form at d_xy / d_inf.  abc: the n_inputs + 1 base points
// on the device (Groth16's gamma_abc_g1, GM17's query); tables: the fixed-base tables of abc[1 ..], the inputs beyond them go
// through the variable-base kernels
template <class E>
int launch_g_ic(const uint32_t* abc, const std::vector<gh_rt::FixedTable*>& tables, const uint64_t* d_inputs, size_t n, size_t n_inputs,
                uint64_t* d_xy, uint8_t* d_inf) {
    typedef typename E::G1 C;
    Proj<C>*d_acc, *d_tmp;
    Fp* d_zp;
    uint32_t* d_k = nullptr;
    uint64_t* d_base = nullptr;
    int rc = dbuf("vb_p", n, &d_acc);
    if (!rc) rc = dbuf("vb_p2", n, &d_tmp);
    if (!rc) rc = dbuf("vb_zp", n, &d_zp);
    if (!rc && n_inputs) rc = dbuf("vb_pair_k", n * n_inputs * 24, &d_k);
    if (!rc && tables.size() < n_inputs) rc = dbuf("vb_pk", n * 24, &d_base);
    if (rc) return rc;
    GH_LAUNCH((fill_proj_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, d_acc, n, abc);
    if (n_inputs)
        GH_LAUNCH((inputs_to_int_kernel<typename EngineHost<E>::PS>), dim3(blocks(n * n_inputs, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_inputs, n, n_inputs, d_k);
    for (size_t j = 0; j < n_inputs; j++) {
        const uint32_t* kj = d_k + j * n * 24;
        if (j < tables.size()) {
            if ((rc = gh_rt::fixed_table_sums(tables[j], kj, n, d_tmp))) return rc;
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

// the pooled buffers of a verification of n rows: A, B, C with their infinity bytes, the inputs, g_ic, the rows' values and status
struct VerifyBufs {
    uint64_t *d_a, *d_b, *d_c, *d_in = nullptr, *d_gic, *d_val;
    uint8_t *d_ai, *d_bi, *d_ci, *d_gi, *d_st;
};
template <class E> int verify_bufs(size_t n, size_t n_inputs, VerifyBufs& v) {
    constexpr size_t TW = tower_words<E>() / 2;    // u64 words of a G2 point and of a GT element
    int rc = dbuf("vb_pair_g1", n * 24, &v.d_a);
    if (!rc) rc = dbuf("vb_pair_g2", n * TW, &v.d_b);
    if (!rc) rc = dbuf("vb_pair_c", n * 24, &v.d_c);
    if (!rc) rc = dbuf("vb_pair_i1", n, &v.d_ai);
    if (!rc) rc = dbuf("vb_pair_i2", n, &v.d_bi);
    if (!rc) rc = dbuf("vb_pair_i3", n, &v.d_ci);
    if (!rc && n_inputs) rc = dbuf("vb_pair_in", n * n_inputs * 12, &v.d_in);
    if (!rc) rc = dbuf("vb_xy", n * 24, &v.d_gic);
    if (!rc) rc = dbuf("vb_inf", n, &v.d_gi);
    if (!rc) rc = dbuf("vb_pair_val", n * TW, &v.d_val);
    if (!rc) rc = dbuf("vb_st", n, &v.d_st);
    return rc;
}

// A, B, C and their infinity bytes from the host into v
template <class E>
int upload_proofs(const VerifyBufs& v, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                  const uint8_t* c_inf, size_t n) {
    constexpr size_t TW = tower_words<E>() / 2;
    int rc;
    if ((rc = up(v.d_a, a_xy, n * 24)) || (rc = up(v.d_b, b_xy, n * TW)) || (rc = up(v.d_c, c_xy, n * 24)) || (rc = up(v.d_ai, a_inf, n)) ||
        (rc = up(v.d_bi, b_inf, n)))
        return rc;
    return up(v.d_ci, c_inf, n);
}

// the device part of a verification, over proof points and inputs that are on the device: the curve check, g_ic, the Miller
// loops, the final exponentiation and the compare, with the marks of those phases; v.d_st holds the rows' status.  d_pst
// (nullable): 3 point codes per row, a row with a non-zero one gets status 3 and is not evaluated.
template <class E> int verify_device(gh_groth16_vk* h, const VerifyBufs& v, const uint8_t* d_pst, size_t n, size_t n_inputs, PhaseTimer& ph) {
    constexpr size_t TW = tower_words<E>() / 2;
    int rc;
    GH_LAUNCH((proof_check_kernel<E>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)v.d_a, (const uint8_t*)v.d_ai,
              (const uint32_t*)v.d_b, (const uint8_t*)v.d_bi, (const uint32_t*)v.d_c, (const uint8_t*)v.d_ci, n, curve_b<typename E::G1>(),
              EngineHost<E>::g2_b(), v.d_st);
    if (d_pst) GH_LAUNCH(point_status_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, d_pst, n, v.d_st);
    if ((rc = launch_g_ic<E>(h->d_abc.as<const uint32_t>(), h->tables, v.d_in, n, n_inputs, v.d_gic, v.d_gi)) || (rc = ph.mark())) return rc;
    PairIn in{};
    in.g1_rows(0, v.d_a, v.d_ai);
    in.g2_rows(0, v.d_b, v.d_bi, 2 * TW);
    in.g1_rows(1, v.d_gic, v.d_gi);
    in.g1_rows(2, v.d_c, v.d_ci);
    if ((rc = launch_pairs<E, 1, 2>(in, v.d_st, h->d_tab.as<const typename E::Coeff>(), n, v.d_val, &ph))) return rc;
    GH_LAUNCH((gt_compare_kernel<(int)TW>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)v.d_val, h->d_gt.as<const uint64_t>(), n, v.d_st);
    HIPCHK(hipGetLastError());
    return ph.mark();
}

template <class E>
int run_verify(gh_groth16_vk* h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
               const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) {
    if (int rc = vk_ensure<E>(h)) return rc;
    VerifyBufs v;
    int rc = verify_bufs<E>(n, n_inputs, v);
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if ((rc = upload_proofs<E>(v, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, n)) || (n_inputs && (rc = up(v.d_in, inputs, n * n_inputs * 12))) ||
        (rc = ph.mark()))
        return rc;
    if ((rc = verify_device<E>(h, v, nullptr, n, n_inputs, ph))) return rc;
    HIPCHK(hipMemcpyAsync(out_status, v.d_st, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

// gh_groth16_verify_checked / _compressed: the proof points are validated on the device (points.hip) before the verification
// body runs over them; the validation belongs to the upload phase of this unit's timing record and is the validate phase of
// gh_points_last_timing.  compressed: a, b, c hold canonical x (12 D u64 per row for B), the *_fl arguments the flags bytes.
template <class E>
int run_verify_validated(gh_groth16_vk* h, int compressed, const uint64_t* a, const uint8_t* a_fl, const uint64_t* b, const uint8_t* b_fl,
                         const uint64_t* c, const uint8_t* c_fl, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status,
                         uint8_t* out_point_status) {
    constexpr size_t TW = tower_words<E>() / 2;
    constexpr gh_curve_t G1 = EngineHost<E>::g1_curve, G2 = (gh_curve_t)(EngineHost<E>::g1_curve + 1);
    if (int rc = vk_ensure<E>(h)) return rc;
    VerifyBufs v;
    uint8_t* d_pst;
    uint64_t *d_ax = nullptr, *d_bx = nullptr, *d_cx = nullptr;
    uint8_t *d_af = nullptr, *d_bf = nullptr, *d_cf = nullptr;
    int rc = verify_bufs<E>(n, n_inputs, v);
    if (!rc) rc = dbuf("vb_pts_pst", n * 3, &d_pst);
    if (!rc && compressed) {
        rc = dbuf("vb_pts_ax", n * 12, &d_ax);
        if (!rc) rc = dbuf("vb_pts_bx", n * TW / 2, &d_bx);
        if (!rc) rc = dbuf("vb_pts_cx", n * 12, &d_cx);
        if (!rc) rc = dbuf("vb_pts_af", n, &d_af);
        if (!rc) rc = dbuf("vb_pts_bf", n, &d_bf);
        if (!rc) rc = dbuf("vb_pts_cf", n, &d_cf);
    }
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if (n_inputs && (rc = up(v.d_in, inputs, n * n_inputs * 12))) return rc;
    if (compressed) {
        if ((rc = up(d_ax, a, n * 12)) || (rc = up(d_bx, b, n * TW / 2)) || (rc = up(d_cx, c, n * 12)) || (rc = up(d_af, a_fl, n)) ||
            (rc = up(d_bf, b_fl, n)) || (rc = up(d_cf, c_fl, n)) || (rc = gh_rt::points_validate_mark(0)) ||
            (rc = gh_rt::points_decompress_dev(G1, d_ax, d_af, n, v.d_a, v.d_ai, d_pst, 3)) ||
            (rc = gh_rt::points_decompress_dev(G2, d_bx, d_bf, n, v.d_b, v.d_bi, d_pst + 1, 3)) ||
            (rc = gh_rt::points_decompress_dev(G1, d_cx, d_cf, n, v.d_c, v.d_ci, d_pst + 2, 3)))
            return rc;
    } else {
        if ((rc = upload_proofs<E>(v, a, a_fl, b, b_fl, c, c_fl, n)) || (rc = gh_rt::points_validate_mark(0)) ||
            (rc = gh_rt::points_member_dev(G1, v.d_a, v.d_ai, n, d_pst, 3)) || (rc = gh_rt::points_member_dev(G2, v.d_b, v.d_bi, n, d_pst + 1, 3)) ||
            (rc = gh_rt::points_member_dev(G1, v.d_c, v.d_ci, n, d_pst + 2, 3)))
            return rc;
    }
    if ((rc = gh_rt::points_validate_mark(1)) || (rc = ph.mark())) return rc;
    if ((rc = verify_device<E>(h, v, d_pst, n, n_inputs, ph))) return rc;
    HIPCHK(hipMemcpyAsync(out_status, v.d_st, n, hipMemcpyDeviceToHost, g.stream));
    if (out_point_status) HIPCHK(hipMemcpyAsync(out_point_status, d_pst, n * 3, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    if ((rc = gh_rt::points_validate_finish())) return rc;
    return ph.finish();
}

// ---- host checks of a key's points (the same GH_HD arithmetic, on the host)
template <class E> bool g1_on_curve(const uint64_t* xy) {
    typedef typename E::G1 C;
    typedef typename C::FC F;
    const Fp x = fp_from_abi<typename E::PF>((const uint32_t*)xy), y = fp_from_abi<typename E::PF>((const uint32_t*)(xy + 12));
    return F::eq(F::sqr(y), F::add(F::add(F::mul(F::sqr(x), x), C::mul_by_a(x)), curve_b<C>()));
}
template <class E> bool g2_on_curve(const uint64_t* xy) {
    typedef typename E::B B;
    constexpr int H = tower_words<E>() / 4;        // u64 words of a coordinate
    const typename B::T x = B::from_abi((const uint32_t*)xy), y = B::from_abi((const uint32_t*)(xy + H));
    return B::eq(B::sqr(y), B::add(B::add(B::mul(B::sqr(x), x), E::G2::mul_by_a(x)), EngineHost<E>::g2_b()));
}
template <class E> void g2_negate(uint64_t* out, const uint64_t* xy) {
    typedef typename E::B B;
    constexpr int H = tower_words<E>() / 4;
    memcpy(out, xy, H * 8);
    B::to_abi((uint32_t*)(out + H), B::neg(B::from_abi((const uint32_t*)(xy + H))));
}

// ---- the bodies of the entry points for one engine, under the caller's lock
template <class E>
int api_product(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, size_t k, uint64_t* out_gt) {
    typedef typename E::PF PF;
    if (k < 1 || k > MAX_PAIRS) { g_err = "the number of pairs per row must be 1, 2 or 3"; return GH_E_BAD_ARG; }
    if (n && (!g1_xy || !g1_inf || !g2_xy || !g2_inf || !out_gt)) return null_arg();
    size_t b;
    if (mul_overflows(n, 4096, &b)) return too_large();
    if (!all_below<PF>(g1_xy, 2 * n * k) || !all_below<PF>(g2_xy, 2 * E::BDEG * n * k)) { g_err = "a coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = gh_rt::ensure_init()) return rc;
    return run_product<E>(g1_xy, g1_inf, g2_xy, g2_inf, n, k, out_gt);
}

template <class E>
int api_vk_create(int engine, const uint64_t* alpha_g1_beta_g2, const uint64_t* gamma_g2_xy, const uint64_t* delta_g2_xy,
                  const uint64_t* gamma_abc_g1_xy, size_t n_abc, gh_groth16_vk** out) {
    typedef typename E::PF PF;
    constexpr size_t TW = tower_words<E>() / 2, TC = 2 * E::BDEG;       // u64 words / Fq coefficients of a G2 point and of a GT element
    if (!alpha_g1_beta_g2 || !gamma_g2_xy || !delta_g2_xy || !gamma_abc_g1_xy) return null_arg();
    size_t b;
    if (n_abc == 0 || mul_overflows(n_abc, 4096, &b)) { g_err = "gamma_abc_g1 must hold at least one point"; return GH_E_BAD_ARG; }
    if (!all_below<PF>(alpha_g1_beta_g2, TC) || !all_below<PF>(gamma_g2_xy, TC) || !all_below<PF>(delta_g2_xy, TC) ||
        !all_below<PF>(gamma_abc_g1_xy, 2 * n_abc)) {
        g_err = "a coefficient of the verifying key is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (!g2_on_curve<E>(gamma_g2_xy) || !g2_on_curve<E>(delta_g2_xy)) { g_err = "gamma_g2 or delta_g2 is not on the curve"; return GH_E_BAD_ARG; }
    for (size_t j = 0; j < n_abc; j++)
        if (!g1_on_curve<E>(gamma_abc_g1_xy + 24 * j)) { g_err = "a point of gamma_abc_g1 is not on the curve"; return GH_E_BAD_ARG; }
    std::unique_ptr<gh_groth16_vk> h(new gh_groth16_vk());
    h->engine = engine;
    h->n_abc = n_abc;
    h->gt.assign(alpha_g1_beta_g2, alpha_g1_beta_g2 + TW);
    h->g2_neg.resize(2 * TW);
    g2_negate<E>(h->g2_neg.data(), gamma_g2_xy);
    g2_negate<E>(h->g2_neg.data() + TW, delta_g2_xy);
    h->abc.assign(gamma_abc_g1_xy, gamma_abc_g1_xy + 24 * n_abc);
    *out = h.release();
    return GH_OK;
}

// the argument checks the verify entry points share.  n_points: the points of the key that take the public inputs (one more
// than the inputs), what: that array's name.  compressed: a, b, c hold untrusted x coordinates, and what is wrong with them
// is a row's status, not an argument error.
template <class E>
int check_proof_args(size_t n_points, const char* what, bool compressed, const uint64_t* a, const uint8_t* a_inf, const uint64_t* b,
                     const uint8_t* b_inf, const uint64_t* c, const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs,
                     const uint8_t* out_status) {
    typedef typename E::PF PF;
    if (n_inputs + 1 != n_points) {
        g_err = std::string("the number of public inputs does not match ") + what + " (MalformedVerifyingKey)";
        return GH_E_BAD_ARG;
    }
    if (n && (!a || !a_inf || !b || !b_inf || !c || !c_inf || (n_inputs && !inputs) || !out_status)) return null_arg();
    size_t ni = 0, by = 0;
    if (mul_overflows(n, n_inputs, &ni) || mul_overflows(ni, 96 * 4, &by) || mul_overflows(n, 4096, &by)) return too_large();
    if (!compressed && (!all_below<PF>(a, 2 * n) || !all_below<PF>(b, 2 * E::BDEG * n) || !all_below<PF>(c, 2 * n))) {
        g_err = "a proof coordinate is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (n_inputs && !all_below<typename EngineHost<E>::PS>(inputs, ni)) { g_err = "a public input is not below the modulus"; return GH_E_BAD_ARG; }
    return GH_OK;
}

template <class E>
int api_verify(gh_groth16_vk* h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
               const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) {
    if (int rc = check_proof_args<E>(h->n_abc, "gamma_abc_g1", false, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status)) return rc;
    if (n == 0) return GH_OK;
    if (int rc = gh_rt::ensure_init()) return rc;
    return run_verify<E>(h, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status);
}

template <class E>
int api_verify_validated(gh_groth16_vk* h, int compressed, const uint64_t* a, const uint8_t* a_fl, const uint64_t* b, const uint8_t* b_fl,
                         const uint64_t* c, const uint8_t* c_fl, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status,
                         uint8_t* out_point_status) {
    if (int rc = check_proof_args<E>(h->n_abc, "gamma_abc_g1", compressed != 0, a, a_fl, b, b_fl, c, c_fl, inputs, n, n_inputs, out_status)) return rc;
    if (n == 0) return GH_OK;
    if (int rc = gh_rt::ensure_init()) return rc;
    return run_verify_validated<E>(h, compressed, a, a_fl, b, b_fl, c, c_fl, inputs, n, n_inputs, out_status, out_point_status);
}

int api_last_timing(float* phase_ms, int max_phases, float* total_ms) { return g_tm.copy_out(phase_ms, max_phases, total_ms); }

}  // namespace

// the unit's engine behind gh_rt::NAME()
#define GH_DEFINE_PAIRING_OPS(ENGINE, NAME)                                                                                 \
    namespace gh_rt {                                                                                                        \
    const PairingOps* NAME() {                                                                                               \
        static const PairingOps ops = {&api_product<ENGINE>,        &api_vk_create<ENGINE>, &api_verify<ENGINE>,  &api_last_timing, &api_verify_validated<ENGINE>, \
                                       &api_gm17_vk_create<ENGINE>, &api_gm17_verify<ENGINE>, &api_gm17_last_timing};           \
        return &ops;                                                                                                         \
    }                                                                                                                        \
    }

