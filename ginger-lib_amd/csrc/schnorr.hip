// schnorr.hip -- the C ABI of include/ginger_hip_schnorr.h: the batched variable-base scalar multiplication gh_batch_mul and
// the field-based Schnorr signature (primitives/src/signature/schnorr/field_based_schnorr.rs) built on it, the fixed-base
// path of fixed_base.hip and the Poseidon kernels of poseidon.hip.  DESIGN.md section 12.
//
// The kernels and the host steps shared with ecvrf.hip are those of vb_kernels.h.
#include "vb_kernels.h"
#include "../../include/ginger_hip_schnorr.h"

struct gh_schnorr {
    uint32_t magic = 0x6768536eu;
    gh_curve_t curve;
    gh_poseidon_t hash = nullptr;
    GeneratorTable gen;
};

namespace {

constexpr int VB_W_DEFAULT = 4;                       // the fastest of the sweep w = 4, 5, 6
PhaseTimer g_tm{6};                                   // upload, fixed base, variable base, normalise, hash, finish

// hash rows m_0 .. m_(len-1) | R.x | R.y | pk.x: the message and pk.x (0 for the point at infinity); R comes from normalize_kernel
__global__ void __launch_bounds__(256) rows_kernel(const uint64_t* __restrict__ msg, const uint64_t* __restrict__ pk_xy,
                                                   const uint8_t* __restrict__ pk_inf, size_t n, size_t len, uint64_t* __restrict__ rows) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t* r = rows + i * (len + 3) * 12;
    for (size_t w = 0; w < len * 12; w++) r[w] = msg[i * len * 12 + w];
    const bool zero = pk_inf[i] != 0;
    for (int w = 0; w < 12; w++) r[(len + 2) * 12 + w] = zero ? 0ull : pk_xy[i * 24 + w];
}

// verify step 7: 1 if e' == e, 0 if not, Err rows keep 2
__global__ void __launch_bounds__(256) compare_kernel(const uint64_t* __restrict__ e2, const uint64_t* __restrict__ sig, size_t n,
                                                      uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status[i] == 2) return;
    bool eq = true;
    for (int w = 0; w < 12; w++) eq &= e2[i * 12 + w] == sig[i * 24 + w];
    status[i] = eq;
}

// ---------------------------------------------------------------------------------------------------- host side
int vb_window() {
    static const int w = gh_rt::env_int("GH_SCHNORR_WINDOW", VB_W_DEFAULT);   // measurement knob: 4, 5 or 6; anything else: the default
    return (w == 4 || w == 5 || w == 6) ? w : VB_W_DEFAULT;
}

// d_out[i] = (+-) k_i P_i as internal Proj<C>, on g.stream
template <class C> int vb_launch(const void* d_xy, const uint8_t* d_inf, const uint32_t* d_k, size_t n, int negate, Proj<C>* d_out) {
    switch (vb_window()) {
        case 5: return vb_single<C, 5>(d_xy, d_inf, negate, &d_k, &d_out, 1, n);
        case 6: return vb_single<C, 6>(d_xy, d_inf, negate, &d_k, &d_out, 1, n);
    }
    return vb_single<C, 4>(d_xy, d_inf, negate, &d_k, &d_out, 1, n);
}

template <class C> int run_sign(gh_schnorr* h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n,
                                size_t len, const uint64_t* nonce, uint64_t* out_sig, uint8_t* out_status) {
    typedef typename Scheme<C>::PF PF;
    typedef typename Scheme<C>::PS PS;
    if (int rc = h->gen.ensure(h->curve, n)) return rc;
    const size_t rw = (len + 3) * 12;
    uint64_t *d_sk, *d_nonce, *d_pk, *d_msg, *d_rows, *d_e, *d_sig;
    uint8_t *d_pkinf, *d_st;
    uint32_t* d_k;
    Proj<C>* d_p;
    Fp* d_zp;
    int rc = dbuf("vb_in", n * 12, &d_sk);
    if (!rc) rc = dbuf("vb_in2", n * 12, &d_nonce);
    if (!rc) rc = dbuf("vb_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("vb_pkinf", n, &d_pkinf);
    if (!rc) rc = dbuf("vb_msg", n * len * 12, &d_msg);
    if (!rc) rc = dbuf("vb_k", n * 24, &d_k);
    if (!rc) rc = dbuf("vb_p", n, &d_p);
    if (!rc) rc = dbuf("vb_zp", n, &d_zp);
    if (!rc) rc = dbuf("vb_rows", n * rw, &d_rows);
    if (!rc) rc = dbuf("vb_h", n * 12, &d_e);
    if (!rc) rc = dbuf("vb_xy", n * 24, &d_sig);
    if (!rc) rc = dbuf("vb_st", n, &d_st);
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_sk, sk, n * 12)) || (rc = up(d_nonce, nonce, n * 12)) || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_pkinf, pk_inf, n)) ||
        (rc = up(d_msg, msg, n * len * 12)) || (rc = ph.mark()))
        return rc;
    GH_LAUNCH((mont_to_int_kernel<PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_nonce, n, d_k, d_st);
    if ((rc = gh_rt::fixed_table_sums(h->gen.table, d_k, n, d_p)) || (rc = ph.mark()) || (rc = ph.mark())) return rc;   // no variable-base phase
    GH_LAUNCH(rows_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_msg, (const uint64_t*)d_pk, (const uint8_t*)d_pkinf,
              n, len, d_rows);
    if ((rc = launch_normalize<C>(d_p, nullptr, n, d_zp, d_rows, rw * 2, len * 24, nullptr))) return rc;
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    if ((rc = gh_rt::poseidon_hash_dev_locked(h->hash, d_rows, n, len + 3, d_e)) || (rc = ph.mark())) return rc;
    GH_LAUNCH((sign_finish_kernel<PF, PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_e, (const uint32_t*)d_sk,
              (const uint32_t*)d_nonce, n, (uint32_t*)d_sig, d_st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_sig, d_sig, n * 192, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

template <class C> int run_verify(gh_schnorr* h, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                                  const uint64_t* sig, uint8_t* out_status) {
    typedef typename Scheme<C>::PF PF;
    if (int rc = h->gen.ensure(h->curve, n)) return rc;
    const size_t rw = (len + 3) * 12;
    uint64_t *d_sig, *d_pk, *d_msg, *d_rows, *d_e;
    uint8_t *d_pkinf, *d_st;
    uint32_t *d_ei, *d_si;
    Proj<C>*d_pa, *d_pb;
    Fp* d_zp;
    int rc = dbuf("vb_xy", n * 24, &d_sig);
    if (!rc) rc = dbuf("vb_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("vb_pkinf", n, &d_pkinf);
    if (!rc) rc = dbuf("vb_msg", n * len * 12, &d_msg);
    if (!rc) rc = dbuf("vb_k", n * 24, &d_ei);
    if (!rc) rc = dbuf("vb_k2", n * 24, &d_si);
    if (!rc) rc = dbuf("vb_p", n, &d_pa);
    if (!rc) rc = dbuf("vb_p2", n, &d_pb);
    if (!rc) rc = dbuf("vb_zp", n, &d_zp);
    if (!rc) rc = dbuf("vb_rows", n * rw, &d_rows);
    if (!rc) rc = dbuf("vb_h", n * 12, &d_e);
    if (!rc) rc = dbuf("vb_st", n, &d_st);
    if (rc) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_sig, sig, n * 24)) || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_pkinf, pk_inf, n)) || (rc = up(d_msg, msg, n * len * 12)) ||
        (rc = ph.mark()))
        return rc;
    GH_LAUNCH((sig_prep_kernel<PF>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_sig, n, d_ei, d_si, d_st);
    if ((rc = gh_rt::fixed_table_sums(h->gen.table, d_si, n, d_pa)) || (rc = ph.mark())) return rc;                 // s G
    if ((rc = vb_launch<C>(d_pk, d_pkinf, d_ei, n, 1, d_pb)) || (rc = ph.mark())) return rc;                   // e (-PK)
    GH_LAUNCH(rows_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_msg, (const uint64_t*)d_pk, (const uint8_t*)d_pkinf,
              n, len, d_rows);
    if ((rc = launch_normalize<C>(d_pa, d_pb, n, d_zp, d_rows, rw * 2, len * 24, nullptr))) return rc;
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    if ((rc = gh_rt::poseidon_hash_dev_locked(h->hash, d_rows, n, len + 3, d_e)) || (rc = ph.mark())) return rc;
    GH_LAUNCH(compare_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_e, (const uint64_t*)d_sig, n, d_st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

template <class C> int run_batch_mul(const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_xyz) {
    uint64_t *d_xy, *d_out;
    uint32_t* d_k;
    uint8_t* d_inf = nullptr;
    Proj<C>* d_p;
    int rc = dbuf("vb_pk", n * 24, &d_xy);
    if (!rc) rc = dbuf("vb_k", n * 24, &d_k);
    if (!rc) rc = dbuf("vb_p", n, &d_p);
    if (!rc) rc = dbuf("vb_rows", n * 36, &d_out);
    if (!rc && inf) rc = dbuf("vb_pkinf", n, &d_inf);
    if (rc || (rc = up(d_xy, xy, n * 24)) || (rc = up((uint64_t*)d_k, scalars, n * 12)) || (inf && (rc = up(d_inf, inf, n)))) return rc;
    if ((rc = g_tm.begin().mark()) || (rc = vb_launch<C>(d_xy, d_inf, d_k, n, 0, d_p)) || (rc = g_tm.mark())) return rc;
    GH_LAUNCH((proj_to_abi_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const Proj<C>*)d_p, n, (uint32_t*)d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_xyz, d_out, n * 288, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return g_tm.single(2);                                             // the variable-base phase: the two kernels
}

int checked_handle(gh_schnorr* h) {
    if (!h || h->magic != 0x6768536eu) { g_err = "not a Schnorr handle"; return GH_E_BAD_HANDLE; }
    return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

extern "C" {

int gh_schnorr_create(gh_curve_t curve, gh_poseidon_t hash, int window, gh_schnorr_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!hash || !out) return null_arg();
    *out = nullptr;
    if (int rc = check_create("Schnorr", curve, hash, window)) return rc;
    auto* h = new gh_schnorr();
    h->curve = curve;
    h->hash = hash;
    h->gen.window = window;
    *out = h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_free(gh_schnorr_t h) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!h) return GH_OK;
    if (int rc = checked_handle(h)) return rc;
    h->gen.destroy();
    h->magic = 0;
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_public_keys(gh_schnorr_t h, const uint64_t* sk, size_t n, uint64_t* out_pk_xy, uint8_t* out_pk_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    return public_keys_api(h->gen, h->curve, sk, n, out_pk_xy, out_pk_inf);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_sign(gh_schnorr_t h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg,
                    size_t n, size_t len, const uint64_t* nonce, uint64_t* out_sig, uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    if (n && (!sk || !pk_xy || !pk_inf || (len && !msg) || !nonce || !out_sig || !out_status)) return null_arg();
    if (int rc = GH_G1_DISPATCH(h->curve, check_rows, pk_xy, len ? msg : nullptr, n, len)) return rc;
    if (!GH_G1_DISPATCH(h->curve, scalar_below, sk, n) || !GH_G1_DISPATCH(h->curve, scalar_below, nonce, n)) {
        g_err = "a secret key or nonce is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_G1_DISPATCH(h->curve, run_sign, h, sk, pk_xy, pk_inf, msg, n, len, nonce, out_sig, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_verify(gh_schnorr_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                      const uint64_t* sig, uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    if (n && (!pk_xy || !pk_inf || (len && !msg) || !sig || !out_status)) return null_arg();
    if (int rc = GH_G1_DISPATCH(h->curve, check_rows, pk_xy, len ? msg : nullptr, n, len)) return rc;
    if (!GH_G1_DISPATCH(h->curve, data_below, sig, 2 * n)) { g_err = "a signature element is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_G1_DISPATCH(h->curve, run_verify, h, pk_xy, pk_inf, msg, n, len, sig, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_keyverify(gh_schnorr_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    return keyverify_api(h->curve, pk_xy, pk_inf, n, out_ok);
} catch (...) { return gh_rt::api_exception(); }

int gh_batch_mul(gh_curve_t curve, const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_xyz) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = check_batch("gh_batch_mul", curve, n, xy && scalars && out_xyz)) return rc;
    if (!GH_G1_DISPATCH(curve, data_below, xy, 2 * n)) { g_err = "a base coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (!below_2_753(scalars, n)) { g_err = "a scalar is not below 2^753"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_G1_DISPATCH(curve, run_batch_mul, xy, inf, scalars, n, out_xyz);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return g_tm.copy_out(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
