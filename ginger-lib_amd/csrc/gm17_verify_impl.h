// gm17_verify_impl.h -- the batched GM17 verifier (proof-systems/src/gm17/verifier.rs:9-76, include/ginger_hip_gm17.h) on the
// pairing kernels of pairing_impl.h, as templates over the same engine policy E.  Included by pairing.hip and
// pairing_mnt6753.hip after pairing_impl.h; the engine's PairingOps end with the three entry points below.  DESIGN.md 14b.
//
//   gm17_sums_kernel   one row per lane: -S1 = -(A + g_alpha), S2 = B + h_beta and -B in ABI form with infinity bytes, by
//                      the complete affine addition of gm17_sum.h (one inversion per sum, no data-dependent loop)
//   test1              launch_pairs<E, 1, 2>: the variable pair (-S1, S2), the prepared pairs (g_psi, h_gamma) and (C, h)
//   test2              launch_pairs<E, 1, 1>: the variable pair (g_gamma, -B), g_gamma read with stride 0 from the key, the
//                      prepared pair (A, h_gamma) through the same table pointer
//   verdict            gt_compare_kernel on test1's values against the key's e(-g_alpha, h_beta), on test2's against one,
//                      then the AND; rows of status 2 keep it
// g_psi is launch_g_ic over the key's query, with Groth16's fixed-base tables and variable-base fallback.
#pragma once
#include "pairing_impl.h"
#include "gm17_sum.h"
#include "../../include/ginger_hip_gm17.h"

struct gh_gm17_vk {
    static constexpr uint32_t MAGIC = 0x6768374du;
    uint32_t magic = MAGIC;
    int engine = GH_PAIRING_MNT4753;               // GH_PAIRING_*: which PairingOps verify with this key
    size_t n_query = 0;
    std::vector<uint64_t> g1;                      // g_alpha, g_gamma, -g_alpha: 3 x 24 words
    std::vector<uint64_t> g2;                      // h_gamma, h (the order of the tables), h_beta: 3 x 24 D words
    std::vector<uint64_t> query;                   // n_query x 24 words
    gh_rt::DevMem d_g1, d_g2;                      // the two arrays above, then one zero byte row behind d_g1 (no key point is at infinity)
    gh_rt::DevMem d_tab;                           // 2 x TABLE_STEPS line coefficients of h_gamma and h
    gh_rt::DevMem d_gt;                            // e(-g_alpha, h_beta), then one: 2 x 24 D words
    gh_rt::DevMem d_query;
    std::vector<gh_rt::FixedTable*> tables;        // the fixed-base table of query[j + 1], for the first inputs
    bool built = false;
    ~gh_gm17_vk() {
        for (auto* t : tables) gh_rt::fixed_table_destroy(t);
        magic = 0;
    }
};

namespace {

PhaseTimer g_gm17_tm{9};                           // upload, g_psi, sums, test1 Miller / final exp, test2 Miller / final exp, compare, download

// rows of status 2 are left alone (their pairs are skipped by pair_setup_kernel); every other row gets
//   ns1 = -(A + g_alpha),  s2 = B + h_beta,  nb = -B     with their infinity bytes (nb's is B's own)
// key_g1: g_alpha at word 0; key_hbeta: h_beta (ABI words)
template <class E>
__global__ void __launch_bounds__(BLOCK)
gm17_sums_kernel(const uint32_t* __restrict__ a, const uint8_t* __restrict__ a_inf, const uint32_t* __restrict__ b,
                 const uint8_t* __restrict__ b_inf, const uint8_t* __restrict__ status, const uint32_t* __restrict__ key_g1,
                 const uint32_t* __restrict__ key_hbeta, size_t n, uint32_t* __restrict__ ns1, uint8_t* __restrict__ ns1_inf,
                 uint32_t* __restrict__ s2, uint8_t* __restrict__ s2_inf, uint32_t* __restrict__ nb) {
    typedef typename E::PF PF;
    typedef typename E::B B;
    typedef typename B::T BT;
    constexpr int W = tower_words<E>();
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (status[i] == 2) {
        ns1_inf[i] = s2_inf[i] = 1;
        return;
    }
    {
        const bool inf = a_inf[i] != 0;
        const Gm17Point<Fp> p{inf ? fp_zero() : fp_from_abi<PF>(a + i * 48), inf ? fp_zero() : fp_from_abi<PF>(a + i * 48 + 24), inf};
        const Gm17Point<Fp> q{fp_from_abi<PF>(key_g1), fp_from_abi<PF>(key_g1 + 24), false};
        const Gm17Point<Fp> s = gm17_neg<Gm17G1<E>>(gm17_add<Gm17G1<E>>(p, q));
        fp_to_abi<PF>(ns1 + i * 48, s.x);
        fp_to_abi<PF>(ns1 + i * 48 + 24, s.y);
        ns1_inf[i] = s.inf;
    }
    {
        const bool inf = b_inf[i] != 0;
        const Gm17Point<BT> p{inf ? B::zero() : B::from_abi(b + i * W), inf ? B::zero() : B::from_abi(b + i * W + W / 2), inf};
        const Gm17Point<BT> q{B::from_abi(key_hbeta), B::from_abi(key_hbeta + W / 2), false};
        const Gm17Point<BT> s = gm17_add<Gm17G2<E>>(p, q);
        B::to_abi(s2 + i * W, s.x);
        B::to_abi(s2 + i * W + W / 2, s.y);
        s2_inf[i] = s.inf;
        B::to_abi(nb + i * W, p.x);
        B::to_abi(nb + i * W + W / 2, B::neg(p.y));
    }
}

// status[i] = status[i] AND other[i]; rows of status 2 keep it
__global__ void __launch_bounds__(256) gm17_and_kernel(uint8_t* __restrict__ status, const uint8_t* __restrict__ other, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status[i] == 2) return;
    status[i] = status[i] == 1 && other[i] == 1;
}

// the device side of a key: the key's points, the tables [h_gamma, h], e(-g_alpha, h_beta) by the product path, query and
// its fixed-base tables
template <class E> int gm17_vk_ensure(gh_gm17_vk* h) {
    if (h->built) return GH_OK;
    constexpr size_t TW = tower_words<E>() / 2, TB = TW * 8;       // u64 words / bytes of a G2 point and of a GT element
    gh_rt::DevMem d_g1, d_g2, d_tab, d_gt, d_query;
    int rc;
    if ((rc = d_g1.alloc(3 * 192 + 64)) || (rc = d_g2.alloc(3 * TB)) || (rc = d_tab.alloc(2 * E::TABLE_STEPS * sizeof(typename E::Coeff))) ||
        (rc = d_gt.alloc(2 * TB)) || (rc = d_query.alloc(h->n_query * 192)))
        return rc;
    HIPCHK(hipMemsetAsync(d_g1.get(), 0, 3 * 192 + 64, g.stream));
    HIPCHK(hipMemcpyAsync(d_g1.get(), h->g1.data(), 3 * 192, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_g2.get(), h->g2.data(), 3 * TB, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_query.get(), h->query.data(), h->n_query * 192, hipMemcpyHostToDevice, g.stream));
    {
        std::vector<uint64_t> one(TW, 0);                          // the one of the target field: c0.c0 = 1
        memcpy(one.data(), EngineHost<E>::one(), 96);
        HIPCHK(hipMemcpyAsync(d_gt.as<uint64_t>() + TW, one.data(), TB, hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));                    // `one` leaves scope
    }
    GH_LAUNCH((g2_prepare_kernel<E>), dim3(1), dim3(BLOCK), 0, g.stream, d_g2.as<const uint32_t>(), 2, d_tab.as<typename E::Coeff>());
    HIPCHK(hipGetLastError());
    // e(-g_alpha, h_beta): one row of one variable pair
    PairIn in{};
    const uint8_t* zero = d_g1.as<const uint8_t>() + 3 * 192;
    in.g1_rows(0, d_g1.as<const uint32_t>() + 2 * 48, zero, 0, 0);
    in.g2_rows(0, d_g2.as<const uint32_t>() + 2 * 2 * TW, zero, 0, 0);
    if ((rc = launch_pairs<E, 1, 0>(in, nullptr, nullptr, 1, d_gt.as<uint64_t>(), nullptr))) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    if ((rc = ensure_abc_tables<E>(h->query.data(), h->n_query, h->tables))) return rc;
    h->d_g1 = std::move(d_g1);
    h->d_g2 = std::move(d_g2);
    h->d_tab = std::move(d_tab);
    h->d_gt = std::move(d_gt);
    h->d_query = std::move(d_query);
    h->built = true;
    return GH_OK;
}

template <class E>
int run_gm17_verify(gh_gm17_vk* h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                    const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) {
    constexpr size_t TW = tower_words<E>() / 2;    // u64 words of a G2 point and of a GT element
    if (int rc = gm17_vk_ensure<E>(h)) return rc;
    VerifyBufs v;                                  // v.d_gic / v.d_gi hold g_psi, v.d_val test1's values until the compare
    uint64_t *d_ns1, *d_s2, *d_nb, *d_val2;
    uint8_t *d_s1i, *d_s2i, *d_st2;
    int rc = verify_bufs<E>(n, n_inputs, v);
    if (!rc) rc = dbuf("vb_gm17_ns1", n * 24, &d_ns1);
    if (!rc) rc = dbuf("vb_gm17_s2", n * TW, &d_s2);
    if (!rc) rc = dbuf("vb_gm17_nb", n * TW, &d_nb);
    if (!rc) rc = dbuf("vb_gm17_i1", n, &d_s1i);
    if (!rc) rc = dbuf("vb_gm17_i2", n, &d_s2i);
    if (!rc) rc = dbuf("vb_gm17_val2", n * TW, &d_val2);
    if (!rc) rc = dbuf("vb_gm17_st2", n, &d_st2);
    if (rc) return rc;
    PhaseTimer& ph = g_gm17_tm.begin();
    if ((rc = ph.mark())) return rc;
    if ((rc = upload_proofs<E>(v, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, n)) || (n_inputs && (rc = up(v.d_in, inputs, n * n_inputs * 12))) ||
        (rc = ph.mark()))
        return rc;
    GH_LAUNCH((proof_check_kernel<E>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)v.d_a, (const uint8_t*)v.d_ai,
              (const uint32_t*)v.d_b, (const uint8_t*)v.d_bi, (const uint32_t*)v.d_c, (const uint8_t*)v.d_ci, n, curve_b<typename E::G1>(),
              EngineHost<E>::g2_b(), v.d_st);
    if ((rc = launch_g_ic<E>(h->d_query.as<const uint32_t>(), h->tables, v.d_in, n, n_inputs, v.d_gic, v.d_gi)) || (rc = ph.mark())) return rc;
    const uint32_t* key_g1 = h->d_g1.as<const uint32_t>();
    const uint32_t* key_g2 = h->d_g2.as<const uint32_t>();
    const uint8_t* zero = h->d_g1.as<const uint8_t>() + 3 * 192;
    GH_LAUNCH((gm17_sums_kernel<E>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)v.d_a, (const uint8_t*)v.d_ai,
              (const uint32_t*)v.d_b, (const uint8_t*)v.d_bi, (const uint8_t*)v.d_st, key_g1, key_g2 + 2 * 2 * TW, n, (uint32_t*)d_ns1, d_s1i,
              (uint32_t*)d_s2, d_s2i, (uint32_t*)d_nb);
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    const typename E::Coeff* tab = h->d_tab.as<const typename E::Coeff>();
    {   // test1: (-S1, S2) variable, (g_psi, h_gamma) and (C, h) prepared
        PairIn in{};
        in.g1_rows(0, d_ns1, d_s1i);
        in.g2_rows(0, d_s2, d_s2i, 2 * TW);
        in.g1_rows(1, v.d_gic, v.d_gi);
        in.g1_rows(2, v.d_c, v.d_ci);
        if ((rc = launch_pairs<E, 1, 2>(in, v.d_st, tab, n, v.d_val, &ph))) return rc;
    }
    {   // test2: (g_gamma, -B) variable, g_gamma the key's for every row; (A, h_gamma) prepared: the first table
        PairIn in{};
        in.g1_rows(0, key_g1 + 48, zero, 0, 0);
        in.g2_rows(0, d_nb, v.d_bi, 2 * TW);
        in.g1_rows(1, v.d_a, v.d_ai);
        if ((rc = launch_pairs<E, 1, 1>(in, v.d_st, tab, n, d_val2, &ph))) return rc;
    }
    HIPCHK(hipMemcpyAsync(d_st2, v.d_st, n, hipMemcpyDeviceToDevice, g.stream));
    GH_LAUNCH((gt_compare_kernel<(int)TW>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)v.d_val, h->d_gt.as<const uint64_t>(), n, v.d_st);
    GH_LAUNCH((gt_compare_kernel<(int)TW>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_val2, h->d_gt.as<const uint64_t>() + TW, n, d_st2);
    GH_LAUNCH(gm17_and_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, v.d_st, (const uint8_t*)d_st2, n);
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipMemcpyAsync(out_status, v.d_st, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

// ---- the bodies of the entry points for one engine, under the caller's lock
template <class E>
int api_gm17_vk_create(int engine, const uint64_t* g_alpha_g1_xy, const uint64_t* h_beta_g2_xy, const uint64_t* g_gamma_g1_xy,
                       const uint64_t* h_gamma_g2_xy, const uint64_t* h_g2_xy, const uint64_t* query_g1_xy, size_t n_query, gh_gm17_vk** out) {
    typedef typename E::PF PF;
    typedef typename E::G1::FC F;
    constexpr size_t TW = tower_words<E>() / 2, TC = 2 * E::BDEG;       // u64 words / Fq coefficients of a G2 point
    if (!g_alpha_g1_xy || !h_beta_g2_xy || !g_gamma_g1_xy || !h_gamma_g2_xy || !h_g2_xy || !query_g1_xy) return null_arg();
    size_t b;
    if (n_query == 0 || mul_overflows(n_query, 4096, &b)) { g_err = "query must hold at least one point"; return GH_E_BAD_ARG; }
    if (!all_below<PF>(g_alpha_g1_xy, 2) || !all_below<PF>(h_beta_g2_xy, TC) || !all_below<PF>(g_gamma_g1_xy, 2) || !all_below<PF>(h_gamma_g2_xy, TC) ||
        !all_below<PF>(h_g2_xy, TC) || !all_below<PF>(query_g1_xy, 2 * n_query)) {
        g_err = "a coefficient of the verifying key is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (!g1_on_curve<E>(g_alpha_g1_xy) || !g1_on_curve<E>(g_gamma_g1_xy)) { g_err = "g_alpha_g1 or g_gamma_g1 is not on the curve"; return GH_E_BAD_ARG; }
    if (!g2_on_curve<E>(h_beta_g2_xy) || !g2_on_curve<E>(h_gamma_g2_xy) || !g2_on_curve<E>(h_g2_xy)) {
        g_err = "h_beta_g2, h_gamma_g2 or h_g2 is not on the curve";
        return GH_E_BAD_ARG;
    }
    for (size_t j = 0; j < n_query; j++)
        if (!g1_on_curve<E>(query_g1_xy + 24 * j)) { g_err = "a point of query is not on the curve"; return GH_E_BAD_ARG; }
    std::unique_ptr<gh_gm17_vk> h(new gh_gm17_vk());
    h->engine = engine;
    h->n_query = n_query;
    h->g1.resize(3 * 24);
    memcpy(h->g1.data(), g_alpha_g1_xy, 192);
    memcpy(h->g1.data() + 24, g_gamma_g1_xy, 192);
    memcpy(h->g1.data() + 48, g_alpha_g1_xy, 96);                       // -g_alpha
    fp_to_abi<PF>((uint32_t*)(h->g1.data() + 60), F::neg(fp_from_abi<PF>((const uint32_t*)(g_alpha_g1_xy + 12))));
    h->g2.resize(3 * TW);
    memcpy(h->g2.data(), h_gamma_g2_xy, TW * 8);
    memcpy(h->g2.data() + TW, h_g2_xy, TW * 8);
    memcpy(h->g2.data() + 2 * TW, h_beta_g2_xy, TW * 8);
    h->query.assign(query_g1_xy, query_g1_xy + 24 * n_query);
    *out = h.release();
    return GH_OK;
}

template <class E>
int api_gm17_verify(gh_gm17_vk* h, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                    const uint8_t* c_inf, const uint64_t* inputs, size_t n, size_t n_inputs, uint8_t* out_status) {
    if (int rc = check_proof_args<E>(h->n_query, "query", false, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status)) return rc;
    if (n == 0) return GH_OK;
    if (int rc = gh_rt::ensure_init()) return rc;
    return run_gm17_verify<E>(h, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, inputs, n, n_inputs, out_status);
}

int api_gm17_last_timing(float* phase_ms, int max_phases, float* total_ms) { return g_gm17_tm.copy_out(phase_ms, max_phases, total_ms); }

}  // namespace
