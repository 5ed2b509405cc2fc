// schnorr.hip -- the C ABI of include/ginger_hip_schnorr.h: the batched variable-base scalar multiplication gh_batch_mul and
// the field-based Schnorr signature (primitives/src/signature/schnorr/field_based_schnorr.rs) built on it, the fixed-base
// path of fixed_base.hip and the Poseidon kernels of poseidon.hip.  DESIGN.md section 12.
//
// The kernels are those of vb_kernels.h.  Large batches are cut into chunks whose slab stays below VB_SLAB_BYTES.
#include <chrono>
#include <vector>
#include "vb_kernels.h"
#include "../../include/ginger_hip_schnorr.h"

using namespace gh;
using gh_rt::g;
using gh_rt::g_err;

struct gh_schnorr {
    uint32_t magic = 0x6768536eu;
    gh_curve_t curve;
    gh_poseidon_t hash = nullptr;
    int window = 0;                       // the caller's fixed-base window, 0 = automatic
    gh_rt::FixedTable* table = nullptr;   // the generator's window table (scalar_size 753), built on first use
    int table_window = 0;                 // the window it was built with
};

namespace {

constexpr size_t VB_SLAB_BYTES = (size_t)1 << 30;     // bound of the variable-base slab; larger batches run in chunks
constexpr size_t SLAB_KEEP_BYTES = (size_t)64 << 20;  // pooled buffers above this are released when an entry point returns
constexpr int VB_W_DEFAULT = 4;                       // the fastest of the sweep w = 4, 5, 6
constexpr int NPHASES = 6;
float g_phase_ms[NPHASES];
float g_total_ms = 0;

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

template <class C, int W> int vb_launch_w(const void* d_xy, const uint8_t* d_inf, const void* d_k, size_t n, int negate, void* d_out) {
    const size_t per_row = (size_t)VbWindow<W>::E * SLOTS_PER_ENTRY * NL * 4;
    size_t chunk = std::max<size_t>(BLOCK, (VB_SLAB_BYTES / per_row) / BLOCK * BLOCK);
    chunk = std::min(chunk, n);
    uint32_t* slab = nullptr;
    if (int rc = gh_rt::pool_get("schnorr_slab", chunk * per_row, (void**)&slab)) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t cnt = std::min(chunk, n - r0);
        GH_LAUNCH((vb_table_kernel<C, W>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_xy, d_inf, r0, cnt,
                  negate, slab);
        GH_LAUNCH((vb_mul_kernel<C, W>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)slab, (const uint32_t*)d_k,
                  d_inf, r0, cnt, (Proj<C>*)d_out);
    }
    HIPCHK(hipGetLastError());
    return GH_OK;
}
// d_out[i] = (+-) k_i P_i as internal Proj<C>, on g.stream
template <class C> int vb_launch(const void* d_xy, const uint8_t* d_inf, const void* d_k, size_t n, int negate, void* d_out) {
    if (n == 0) return GH_OK;
    switch (vb_window()) {
        case 5: return vb_launch_w<C, 5>(d_xy, d_inf, d_k, n, negate, d_out);
        case 6: return vb_launch_w<C, 6>(d_xy, d_inf, d_k, n, negate, d_out);
    }
    return vb_launch_w<C, 4>(d_xy, d_inf, d_k, n, negate, d_out);
}

struct Trim {
    ~Trim() {
        // every pooled buffer of this unit (pool names are matched as prefixes: "schnorr_k" covers "schnorr_k2")
        bool synced = false;
        for (const char* b : {"schnorr_slab", "schnorr_rows", "schnorr_pa", "schnorr_pb", "schnorr_xy", "schnorr_msg", "schnorr_k2",
                              "schnorr_k", "schnorr_zp", "schnorr_e", "schnorr_in2", "schnorr_in", "schnorr_pkinf", "schnorr_pk",
                              "schnorr_st"})
            if (gh_rt::pool_cap(b) > SLAB_KEEP_BYTES) {
                if (!synced) (void)hipStreamSynchronize(g.stream);   // an error return may leave kernels in flight
                synced = true;
                gh_rt::pool_release(b);
            }
        gh_rt::poseidon_trim_slab();
    }
};

bool valid(const gh_schnorr* h) { return h && h->magic == 0x6768536eu; }

int ensure_table(gh_schnorr* h, size_t n) { return generator_table(h->curve, h->window, n, &h->table, &h->table_window); }

template <class C> int run_public_keys(gh_schnorr* h, const uint64_t* sk, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    typedef typename Scheme<C>::PS PS;
    if (int rc = ensure_table(h, n)) return rc;
    uint64_t *d_sk, *d_xy;
    uint32_t* d_k;
    Proj<C>* d_p;
    Fp* d_zp;
    uint8_t* d_inf;
    int rc = dbuf("schnorr_in", n * 12, &d_sk);
    if (!rc) rc = dbuf("schnorr_k", n * 24, &d_k);
    if (!rc) rc = dbuf("schnorr_pa", n, &d_p);
    if (!rc) rc = dbuf("schnorr_zp", n, &d_zp);
    if (!rc) rc = dbuf("schnorr_xy", n * 24, &d_xy);
    if (!rc) rc = dbuf("schnorr_inf", n, &d_inf);
    if (rc) return rc;
    if ((rc = up(d_sk, sk, n * 12))) return rc;
    GH_LAUNCH((mont_to_int_kernel<PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_sk, n, d_k, (uint8_t*)nullptr);
    if ((rc = gh_rt::fixed_table_sums(h->table, d_k, n, d_p))) return rc;
    GH_LAUNCH((normalize_kernel<C>), dim3(blocks(blocks(n, NORM_RUN), BLOCK)), dim3(BLOCK), 0, g.stream, d_p, (const Proj<C>*)nullptr, n,
              d_zp, (uint32_t*)d_xy, (size_t)48, (size_t)0, d_inf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_xy, d_xy, n * 192, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_inf, d_inf, n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return GH_OK;
}

template <class C> int run_sign(gh_schnorr* h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n,
                                size_t len, const uint64_t* nonce, uint64_t* out_sig, uint8_t* out_status) {
    typedef typename Scheme<C>::PF PF;
    typedef typename Scheme<C>::PS PS;
    if (int rc = ensure_table(h, n)) return rc;
    const size_t rw = (len + 3) * 12;
    uint64_t *d_sk, *d_nonce, *d_pk, *d_msg, *d_rows, *d_e, *d_sig;
    uint8_t *d_pkinf, *d_st;
    uint32_t* d_k;
    Proj<C>* d_p;
    Fp* d_zp;
    int rc = dbuf("schnorr_in", n * 12, &d_sk);
    if (!rc) rc = dbuf("schnorr_in2", n * 12, &d_nonce);
    if (!rc) rc = dbuf("schnorr_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("schnorr_pkinf", n, &d_pkinf);
    if (!rc) rc = dbuf("schnorr_msg", n * len * 12, &d_msg);
    if (!rc) rc = dbuf("schnorr_k", n * 24, &d_k);
    if (!rc) rc = dbuf("schnorr_pa", n, &d_p);
    if (!rc) rc = dbuf("schnorr_zp", n, &d_zp);
    if (!rc) rc = dbuf("schnorr_rows", n * rw, &d_rows);
    if (!rc) rc = dbuf("schnorr_e", n * 12, &d_e);
    if (!rc) rc = dbuf("schnorr_xy", n * 24, &d_sig);
    if (!rc) rc = dbuf("schnorr_st", n, &d_st);
    if (rc) return rc;
    Phases ph{g_phase_ms, NPHASES, &g_total_ms};
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_sk, sk, n * 12)) || (rc = up(d_nonce, nonce, n * 12)) || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_pkinf, pk_inf, n)) ||
        (rc = up(d_msg, msg, n * len * 12)) || (rc = ph.mark()))
        return rc;
    GH_LAUNCH((mont_to_int_kernel<PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_nonce, n, d_k, d_st);
    if ((rc = gh_rt::fixed_table_sums(h->table, d_k, n, d_p)) || (rc = ph.mark()) || (rc = ph.mark())) return rc;   // no variable-base phase
    GH_LAUNCH(rows_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_msg, (const uint64_t*)d_pk, (const uint8_t*)d_pkinf,
              n, len, d_rows);
    GH_LAUNCH((normalize_kernel<C>), dim3(blocks(blocks(n, NORM_RUN), BLOCK)), dim3(BLOCK), 0, g.stream, d_p, (const Proj<C>*)nullptr, n,
              d_zp, (uint32_t*)d_rows, rw * 2, len * 24, (uint8_t*)nullptr);
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
    if (int rc = ensure_table(h, n)) return rc;
    const size_t rw = (len + 3) * 12;
    uint64_t *d_sig, *d_pk, *d_msg, *d_rows, *d_e;
    uint8_t *d_pkinf, *d_st;
    uint32_t *d_ei, *d_si;
    Proj<C>*d_pa, *d_pb;
    Fp* d_zp;
    int rc = dbuf("schnorr_xy", n * 24, &d_sig);
    if (!rc) rc = dbuf("schnorr_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("schnorr_pkinf", n, &d_pkinf);
    if (!rc) rc = dbuf("schnorr_msg", n * len * 12, &d_msg);
    if (!rc) rc = dbuf("schnorr_k", n * 24, &d_ei);
    if (!rc) rc = dbuf("schnorr_k2", n * 24, &d_si);
    if (!rc) rc = dbuf("schnorr_pa", n, &d_pa);
    if (!rc) rc = dbuf("schnorr_pb", n, &d_pb);
    if (!rc) rc = dbuf("schnorr_zp", n, &d_zp);
    if (!rc) rc = dbuf("schnorr_rows", n * rw, &d_rows);
    if (!rc) rc = dbuf("schnorr_e", n * 12, &d_e);
    if (!rc) rc = dbuf("schnorr_st", n, &d_st);
    if (rc) return rc;
    Phases ph{g_phase_ms, NPHASES, &g_total_ms};
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_sig, sig, n * 24)) || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_pkinf, pk_inf, n)) || (rc = up(d_msg, msg, n * len * 12)) ||
        (rc = ph.mark()))
        return rc;
    GH_LAUNCH((sig_prep_kernel<PF>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_sig, n, d_ei, d_si, d_st);
    if ((rc = gh_rt::fixed_table_sums(h->table, d_si, n, d_pa)) || (rc = ph.mark())) return rc;                 // s G
    if ((rc = vb_launch<C>(d_pk, d_pkinf, d_ei, n, 1, d_pb)) || (rc = ph.mark())) return rc;                   // e (-PK)
    GH_LAUNCH(rows_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_msg, (const uint64_t*)d_pk, (const uint8_t*)d_pkinf,
              n, len, d_rows);
    GH_LAUNCH((normalize_kernel<C>), dim3(blocks(blocks(n, NORM_RUN), BLOCK)), dim3(BLOCK), 0, g.stream, d_pa, (const Proj<C>*)d_pb, n, d_zp,
              (uint32_t*)d_rows, rw * 2, len * 24, (uint8_t*)nullptr);
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

template <class C> int run_keyverify(const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok) {
    typedef typename Scheme<C>::PF PF;
    static const uint64_t b4[12] = GH_MNT4753_G1_B0_M_64, b6[12] = GH_MNT6753_G1_B0_M_64;
    const Fp b = fp_from_abi<PF>((const uint32_t*)(std::is_same<C, Mnt6G1>::value ? b6 : b4));
    uint64_t* d_pk;
    uint8_t *d_inf, *d_ok;
    int rc = dbuf("schnorr_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("schnorr_pkinf", n, &d_inf);
    if (!rc) rc = dbuf("schnorr_st", n, &d_ok);
    if (rc || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_inf, pk_inf, n))) return rc;
    GH_LAUNCH((on_curve_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_pk, (const uint8_t*)d_inf, n, b, d_ok);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_ok, d_ok, n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return GH_OK;
}

template <class C> int run_batch_mul(const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_xyz) {
    uint64_t *d_xy, *d_k, *d_out;
    uint8_t* d_inf = nullptr;
    Proj<C>* d_p;
    int rc = dbuf("schnorr_pk", n * 24, &d_xy);
    if (!rc) rc = dbuf("schnorr_k", n * 12, &d_k);
    if (!rc) rc = dbuf("schnorr_pa", n, &d_p);
    if (!rc) rc = dbuf("schnorr_rows", n * 36, &d_out);
    if (!rc && inf) rc = dbuf("schnorr_pkinf", n, &d_inf);
    if (rc || (rc = up(d_xy, xy, n * 24)) || (rc = up(d_k, scalars, n * 12)) || (inf && (rc = up(d_inf, inf, n)))) return rc;
    HIPCHK(hipEventRecord(g.ev[0], g.stream));
    if ((rc = vb_launch<C>(d_xy, d_inf, d_k, n, 0, d_p))) return rc;
    HIPCHK(hipEventRecord(g.ev[1], g.stream));
    GH_LAUNCH((proj_to_abi_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const Proj<C>*)d_p, n, (uint32_t*)d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_xyz, d_out, n * 288, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (int i = 0; i < NPHASES; i++) g_phase_ms[i] = 0;
    HIPCHK(hipEventElapsedTime(&g_phase_ms[2], g.ev[0], g.ev[1]));   // the variable-base phase: the two kernels
    g_total_ms = g_phase_ms[2];
    return GH_OK;
}

// the checks every sign / verify / keyverify shares: handle, nulls, sizes, moduli
template <class C> int check_common(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len) {
    typedef typename Scheme<C>::PF PF;
    size_t nm = 0, b = 0;
    if (mul_overflows(n, len, &nm) || mul_overflows(nm, 96 * 4, &b) || mul_overflows(n, 1024, &b)) { g_err = "input too large"; return GH_E_BAD_ARG; }
    if (!all_below<PF>(pk_xy, 2 * n)) { g_err = "a public-key coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (msg && !all_below<PF>(msg, nm)) { g_err = "a message element is not below the modulus"; return GH_E_BAD_ARG; }
    (void)pk_inf;
    return GH_OK;
}

int checked_handle(gh_schnorr* h) {
    if (!valid(h)) { g_err = "not a Schnorr handle"; return GH_E_BAD_HANDLE; }
    return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

#define GH_SCHNORR_DISPATCH(curve, fn, ...) ((curve) == GH_MNT6753_G1 ? fn<Mnt6G1>(__VA_ARGS__) : fn<Mnt4G1>(__VA_ARGS__))

extern "C" {

int gh_schnorr_create(gh_curve_t curve, gh_poseidon_t hash, int window, gh_schnorr_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!hash || !out) { g_err = "null argument"; return GH_E_BAD_ARG; }
    *out = nullptr;
    if (curve != GH_MNT6753_G1 && curve != GH_MNT4753_G1) { g_err = "the Schnorr group must be a G1 curve"; return GH_E_BAD_ARG; }
    if (window < 0 || window > 22) { g_err = "fixed-base window must be 0 or in [1, 22]"; return GH_E_BAD_ARG; }
    gh_field_t f;
    if (poseidon_field(hash, &f)) { g_err = "not a Poseidon handle"; return GH_E_BAD_ARG; }
    const gh_field_t need = curve == GH_MNT6753_G1 ? Scheme<Mnt6G1>::field : Scheme<Mnt4G1>::field;
    if (f != need) { g_err = "the hash's field is not the curve's base field"; return GH_E_BAD_ARG; }
    auto* h = new gh_schnorr();
    h->curve = curve;
    h->hash = hash;
    h->window = window;
    *out = h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_free(gh_schnorr_t h) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!h) return GH_OK;
    if (!valid(h)) { g_err = "not a Schnorr handle"; return GH_E_BAD_HANDLE; }
    fixed_table_destroy(h->table);
    h->magic = 0;
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_public_keys(gh_schnorr_t h, const uint64_t* sk, size_t n, uint64_t* out_pk_xy, uint8_t* out_pk_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    if (n && (!sk || !out_pk_xy || !out_pk_inf)) { g_err = "null argument"; return GH_E_BAD_ARG; }
    size_t b;
    if (mul_overflows(n, 1024, &b)) { g_err = "input too large"; return GH_E_BAD_ARG; }
    const bool m6 = h->curve == GH_MNT6753_G1;
    if (!(m6 ? all_below<P4>(sk, n) : all_below<P6>(sk, n))) { g_err = "a secret key is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_SCHNORR_DISPATCH(h->curve, run_public_keys, h, sk, n, out_pk_xy, out_pk_inf);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_sign(gh_schnorr_t h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg,
                    size_t n, size_t len, const uint64_t* nonce, uint64_t* out_sig, uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    if (n && (!sk || !pk_xy || !pk_inf || (len && !msg) || !nonce || !out_sig || !out_status)) { g_err = "null argument"; return GH_E_BAD_ARG; }
    const bool m6 = h->curve == GH_MNT6753_G1;
    if (int rc = m6 ? check_common<Mnt6G1>(pk_xy, pk_inf, len ? msg : nullptr, n, len) : check_common<Mnt4G1>(pk_xy, pk_inf, len ? msg : nullptr, n, len))
        return rc;
    if (!(m6 ? all_below<P4>(sk, n) && all_below<P4>(nonce, n) : all_below<P6>(sk, n) && all_below<P6>(nonce, n))) {
        g_err = "a secret key or nonce is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_SCHNORR_DISPATCH(h->curve, run_sign, h, sk, pk_xy, pk_inf, msg, n, len, nonce, out_sig, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_verify(gh_schnorr_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                      const uint64_t* sig, uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    if (n && (!pk_xy || !pk_inf || (len && !msg) || !sig || !out_status)) { g_err = "null argument"; return GH_E_BAD_ARG; }
    const bool m6 = h->curve == GH_MNT6753_G1;
    if (int rc = m6 ? check_common<Mnt6G1>(pk_xy, pk_inf, len ? msg : nullptr, n, len) : check_common<Mnt4G1>(pk_xy, pk_inf, len ? msg : nullptr, n, len))
        return rc;
    if (!(m6 ? all_below<P6>(sig, 2 * n) : all_below<P4>(sig, 2 * n))) { g_err = "a signature element is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_SCHNORR_DISPATCH(h->curve, run_verify, h, pk_xy, pk_inf, msg, n, len, sig, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_keyverify(gh_schnorr_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked_handle(h)) return rc;
    if (n && (!pk_xy || !pk_inf || !out_ok)) { g_err = "null argument"; return GH_E_BAD_ARG; }
    const bool m6 = h->curve == GH_MNT6753_G1;
    if (int rc = m6 ? check_common<Mnt6G1>(pk_xy, pk_inf, nullptr, n, 0) : check_common<Mnt4G1>(pk_xy, pk_inf, nullptr, n, 0)) return rc;
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_SCHNORR_DISPATCH(h->curve, run_keyverify, pk_xy, pk_inf, n, out_ok);
} catch (...) { return gh_rt::api_exception(); }

int gh_batch_mul(gh_curve_t curve, const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_xyz) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (curve == GH_MNT4753_G2 || curve == GH_MNT6753_G2) { g_err = "gh_batch_mul: G1 curves only"; return GH_E_UNSUPPORTED; }
    if (curve != GH_MNT4753_G1 && curve != GH_MNT6753_G1) { g_err = "unknown curve id"; return GH_E_BAD_ARG; }
    if (n && (!xy || !scalars || !out_xyz)) { g_err = "null argument"; return GH_E_BAD_ARG; }
    size_t b;
    if (mul_overflows(n, 1024, &b)) { g_err = "input too large"; return GH_E_BAD_ARG; }
    const bool m6 = curve == GH_MNT6753_G1;
    if (!(m6 ? all_below<P6>(xy, 2 * n) : all_below<P4>(xy, 2 * n))) { g_err = "a base coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    for (size_t i = 0; i < n; i++)
        if (scalars[12 * i + 11] >> 49) { g_err = "a scalar is not below 2^753"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_SCHNORR_DISPATCH(curve, run_batch_mul, xy, inf, scalars, n, out_xyz);
} catch (...) { return gh_rt::api_exception(); }

int gh_schnorr_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if ((!phase_ms && max_phases > 0) || max_phases < 0) { g_err = "null argument"; return GH_E_BAD_ARG; }
    const int cnt = std::min(max_phases, NPHASES);
    for (int i = 0; i < cnt; i++) phase_ms[i] = g_phase_ms[i];
    if (total_ms) *total_ms = g_total_ms;
    return cnt;
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
