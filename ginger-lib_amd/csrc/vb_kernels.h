// vb_kernels.h -- the per-row variable-base kernels and their launches, the pipeline kernels and the pipeline steps that
// schnorr.hip and ecvrf.hip share (DESIGN.md sections 12 and 13), on the host layer of unit_host.h.  Everything sits in an
// anonymous namespace: every unit that includes this header gets its own instances of the kernels.
//
// Variable base, one lane per row (out[i] = k_i P_i, a different P_i per row):
//   vb_table_kernel   the odd multiples (2 j + 1) P_i, j < 2^(W-1), by one doubling and 2^(W-1) - 1 projective additions, then
//                     to affine by Montgomery's trick over the row's entries with ONE safegcd inversion (fp_inv, ~40 products);
//                     the entries live in a per-row global slab, limb-major with the row index fastest (the lanes of a wave
//                     read 256 consecutive bytes per limb)
//   vb_mul_kernel     the regular signed-window recoding of schnorr_recode.h: W (M - 1) doublings and M - 1 mixed additions
//                     for every row, digits read straight from the scalar's bits, one final correction for an even scalar.
//                     Only the exceptional cases inside the mixed addition (P = +-Q, an accumulator at infinity) diverge.
#pragma once
#include "unit_host.h"
#include "msm_kernels.h"
#include "schnorr_recode.h"

namespace {

constexpr int BLOCK = 64;

// ---------------------------------------------------------------------------------------------------- device helpers
// slot s of the row's slab: NL words, stride T (rows of the chunk)
struct RowSlab {
    uint32_t* base;
    size_t stride;
    __device__ __forceinline__ Fp ld(int slot) const {
        Fp r;
        const uint32_t* q = base + (size_t)slot * NL * stride;
#pragma unroll
        for (int i = 0; i < NL; i++) r.l[i] = q[(size_t)i * stride];
        return r;
    }
    __device__ __forceinline__ void st(int slot, const Fp& v) const {
        uint32_t* q = base + (size_t)slot * NL * stride;
#pragma unroll
        for (int i = 0; i < NL; i++) q[(size_t)i * stride] = v.l[i];
    }
};
// entry j: slots 4 j (x), 4 j + 1 (y), 4 j + 2 (z), 4 j + 3 (prefix product of the Montgomery trick)
constexpr int SLOTS_PER_ENTRY = 4;

// internal Montgomery -> the integer itself, 24 LE words
template <class P> GH_HD void fp_to_int(uint32_t* w, const Fp& a) {
    Fp one = fp_zero();
    one.l[0] = 1;
    fp_pack(w, fp_mul<P>(a, one));
}
// an integer below p (24 LE words) -> internal Montgomery
template <class P> GH_HD Fp fp_from_int(const uint32_t* w) { return fp_mul<P>(fp_unpack(w), fp_const<P>(P::R2I)); }
GH_HD bool bit752(const uint32_t* w) { return (w[23] >> 16) & 1u; }

// ---------------------------------------------------------------------------------------------------- variable base
template <class C, int W>
__global__ void __launch_bounds__(BLOCK)
vb_table_kernel(const uint32_t* __restrict__ xy /* n x 48 words, ABI */, const uint8_t* __restrict__ inf, size_t row0, size_t cnt,
                int negate, uint32_t* __restrict__ slab) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    constexpr int E = VbWindow<W>::E;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const size_t i = row0 + t;
    const RowSlab s{slab + t, cnt};
    if (inf && inf[i]) return;                               // vb_mul_kernel writes infinity without reading the slab
    Proj<C> p{fp_from_abi<PF>(xy + i * 48), fp_from_abi<PF>(xy + i * 48 + 24), F::one()};
    if (negate) p.y = F::neg(p.y);
    const Proj<C> d = proj_dbl_call<C>(p);
    Fp run = F::one();
#pragma unroll 1
    for (int j = 0; j < E; j++) {
        if (j) p = proj_add_call<C>(p, d);
        s.st(SLOTS_PER_ENTRY * j, p.x);
        s.st(SLOTS_PER_ENTRY * j + 1, p.y);
        s.st(SLOTS_PER_ENTRY * j + 2, p.z);
        s.st(SLOTS_PER_ENTRY * j + 3, run);                  // product of the non-zero Z before entry j
        if (!F::is_zero(p.z)) run = F::mul(run, p.z);
    }
    Fp inv = fp_inv<PF>(run);
#pragma unroll 1
    for (int j = E - 1; j >= 0; j--) {
        const Fp z = s.ld(SLOTS_PER_ENTRY * j + 2);
        if (F::is_zero(z)) continue;                         // only for a base off the curve: its row is garbage, not a fault
        const Fp zi = F::mul(inv, s.ld(SLOTS_PER_ENTRY * j + 3));
        inv = F::mul(inv, z);
        s.st(SLOTS_PER_ENTRY * j, F::mul(s.ld(SLOTS_PER_ENTRY * j), zi));
        s.st(SLOTS_PER_ENTRY * j + 1, F::mul(s.ld(SLOTS_PER_ENTRY * j + 1), zi));
    }
}

template <class C, int W>
__global__ void __launch_bounds__(BLOCK)
vb_mul_kernel(const uint32_t* __restrict__ slab, const uint32_t* __restrict__ scalars /* n x 24 words, canonical */,
              const uint8_t* __restrict__ inf, size_t row0, size_t cnt, Proj<C>* __restrict__ out) {
    typedef typename C::F F;
    constexpr int M = VbWindow<W>::M;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const size_t i = row0 + t;
    if (inf && inf[i]) {
        st_words(out + i, proj_zero<C>());
        return;
    }
    const RowSlab s{const_cast<uint32_t*>(slab) + t, cnt};
    const uint32_t* k = scalars + i * 24;
    auto entry = [&](uint32_t idx, bool neg) {
        Aff<C> a{s.ld(SLOTS_PER_ENTRY * idx), s.ld(SLOTS_PER_ENTRY * idx + 1)};
        const Fp ny = F::neg(a.y);
        if (neg) a.y = ny;
        return a;
    };
    uint32_t idx;
    bool neg;
    vb_digit<W>(k, M - 1, idx, neg);
    const Aff<C> top = entry(idx, false);
    Proj<C> q{top.x, top.y, F::one()};
#pragma unroll 1
    for (int j = M - 2; j >= 0; j--) {
#pragma unroll 1
        for (int b = 0; b < W; b++) q = proj_dbl<C>(q);
        vb_digit<W>(k, j, idx, neg);
        q = proj_madd<C>(q, entry(idx, neg));
    }
    if (!(k[0] & 1u)) q = proj_madd<C>(q, entry(0, true));   // k was run as k | 1
    st_words(out + i, q);
}

// ---------------------------------------------------------------------------------------------------- pipeline kernels
// a[i] (+ b[i] if b) to affine by Montgomery's trick over runs of NORM_RUN points; x, y in ABI form at
// out_xy + i * row_words + off (y 24 words later), infinity as (0, 1); out_inf (nullable) the infinity bytes
constexpr int NORM_RUN = 16;
template <class C>
__global__ void __launch_bounds__(BLOCK)
normalize_kernel(Proj<C>* __restrict__ a, const Proj<C>* __restrict__ b, size_t n, Fp* __restrict__ zp, uint32_t* __restrict__ out_xy,
                 size_t row_words, size_t off, uint8_t* __restrict__ out_inf) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t i0 = t * NORM_RUN;
    if (i0 >= n) return;
    const int cnt = (int)(n - i0 < (size_t)NORM_RUN ? n - i0 : (size_t)NORM_RUN);
    Fp run = F::one();
    for (int j = 0; j < cnt; j++) {
        Proj<C> p = ld_words(a + i0 + j);
        if (b) {
            p = proj_add_call<C>(p, ld_words(b + i0 + j));
            st_words(a + i0 + j, p);
        }
        st_words(zp + i0 + j, run);
        if (!F::is_zero(p.z)) run = F::mul(run, p.z);
    }
    Fp inv = fp_inv<PF>(run);
    for (int j = cnt - 1; j >= 0; j--) {
        const Proj<C> p = ld_words(a + i0 + j);
        uint32_t* w = out_xy + (i0 + j) * row_words + off;
        const bool zero = F::is_zero(p.z);
        if (out_inf) out_inf[i0 + j] = zero;
        if (zero) {
            fp_to_abi<PF>(w, fp_zero());
            fp_to_abi<PF>(w + 24, F::one());
            continue;
        }
        const Fp zi = F::mul(inv, ld_words(zp + i0 + j));
        inv = F::mul(inv, p.z);
        fp_to_abi<PF>(w, F::mul(p.x, zi));
        fp_to_abi<PF>(w + 24, F::mul(p.y, zi));
    }
}

// scalar-field Montgomery (ABI) -> canonical integers; zero (nullable) flags k == 0
template <class PS>
__global__ void __launch_bounds__(256) mont_to_int_kernel(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out,
                                                          uint8_t* __restrict__ zero) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp v = fp_from_abi<PS>(in + i * 24);
    fp_to_int<PS>(out + i * 24, v);
    if (zero) zero[i] = fp_is_zero(v);
}

// internal projective -> ABI (gh_proj_mul's layout), infinity as (0, 1, 0)
template <class C>
__global__ void __launch_bounds__(256) proj_to_abi_kernel(const Proj<C>* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Proj<C> p = ld_words(in + i);
    if (F::is_zero(p.z)) p = proj_zero<C>();
    fp_to_abi<PF>(out + i * 72, p.x);
    fp_to_abi<PF>(out + i * 72 + 24, p.y);
    fp_to_abi<PF>(out + i * 72 + 48, p.z);
}

// Schnorr's e, s / the VRF's c, s (data-field Montgomery) -> canonical integers; status 2 (Err) if either is >= 2^752, its scalars zeroed
template <class PF>
__global__ void __launch_bounds__(256) sig_prep_kernel(const uint32_t* __restrict__ sig /* n x 48 words */, size_t n,
                                                       uint32_t* __restrict__ e_int, uint32_t* __restrict__ s_int,
                                                       uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* e = e_int + i * 24;
    uint32_t* s = s_int + i * 24;
    fp_to_int<PF>(e, fp_from_abi<PF>(sig + i * 48));
    fp_to_int<PF>(s, fp_from_abi<PF>(sig + i * 48 + 24));
    const bool err = bit752(e) || bit752(s);
    if (err)
        for (int w = 0; w < 24; w++) e[w] = s[w] = 0u;
    status[i] = err ? 2 : 0;
}

// Schnorr's sign / the VRF's prove, after the hash: e (the VRF's c) < 2^752, s = k + e sk in the scalar field, s < 2^752, s into the data field; status 1, or 0 and a
// zero row (k == 0 was flagged by mont_to_int_kernel in status)
template <class PF, class PS>
__global__ void __launch_bounds__(256) sign_finish_kernel(const uint32_t* __restrict__ e_abi, const uint32_t* __restrict__ sk,
                                                          const uint32_t* __restrict__ nonce, size_t n, uint32_t* __restrict__ sig,
                                                          uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* o = sig + i * 48;
    uint32_t e[24], s[24];
    const Fp ef = fp_from_abi<PF>(e_abi + i * 24);
    fp_to_int<PF>(e, ef);
    bool ok = status[i] == 0 && !bit752(e);                  // status[i] == 1 here: k == 0
    if (ok) {
        const Fp es = fp_from_int<PS>(e);                    // e < 2^752 < r
        const Fp sv = fp_add<PS>(fp_from_abi<PS>(nonce + i * 24), fp_mul<PS>(es, fp_from_abi<PS>(sk + i * 24)));
        fp_to_int<PS>(s, sv);
        ok = !bit752(s);
    }
    if (ok) {
        fp_to_abi<PF>(o, ef);
        fp_to_abi<PF>(o + 24, fp_from_int<PF>(s));           // s < 2^752 < p
    } else {
        for (int w = 0; w < 48; w++) o[w] = 0u;
    }
    status[i] = ok;
}

// keyverify: y^2 == x^3 + a x + b, or the point at infinity
template <class C>
__global__ void __launch_bounds__(256) on_curve_kernel(const uint32_t* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n, Fp b,
                                                       uint8_t* __restrict__ ok) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (inf[i]) { ok[i] = 1; return; }
    const Fp x = fp_from_abi<PF>(xy + i * 48), y = fp_from_abi<PF>(xy + i * 48 + 24);
    const Fp rhs = F::add(F::add(F::mul(F::sqr(x), x), C::mul_by_a(x)), b);
    ok[i] = F::eq(F::sqr(y), rhs);
}

// ---------------------------------------------------------------------------------------------------- host side
// The generator's fixed-base table of a handle: the caller's window, or (window 0) gh_fixed_base_window(n), rebuilt when a
// later call's n asks for a larger window than the table has -- a handle first used on a few rows does not keep a tiny table
// for large batches.  The window grows with log n, so a handle rebuilds at most a few times.
struct GeneratorTable {
    int window = 0;                       // the caller's fixed-base window, 0 = automatic
    gh_rt::FixedTable* table = nullptr;   // the generator's window table (scalar_size 753), built on first use
    int table_window = 0;                 // the window it was built with
    int ensure(gh_curve_t curve, size_t n) {
        const int w = std::max(1, std::min(window ? window : gh_fixed_base_window(n), 22));
        if (table && w <= table_window) return GH_OK;
        if (table) {
            HIPCHK(hipStreamSynchronize(g.stream));
            destroy();
        }
        uint64_t g_xyz[36];
        if (curve == GH_MNT6753_G1) generator_xyz<Mnt6G1>(g_xyz);
        else generator_xyz<Mnt4G1>(g_xyz);
        if (int rc = gh_rt::fixed_table_create(curve, g_xyz, VB_BITS, w, &table)) return rc;
        table_window = w;
        return GH_OK;
    }
    void destroy() {
        gh_rt::fixed_table_destroy(table);
        table = nullptr;
        table_window = 0;
    }
};

// ---- the variable-base launches; large batches are cut into chunks whose slabs stay below VB_SLAB_BYTES together
constexpr size_t VB_SLAB_BYTES = (size_t)1 << 30;
template <int W> constexpr size_t vb_row_bytes() { return (size_t)VbWindow<W>::E * SLOTS_PER_ENTRY * NL * 4; }   // one row of one slab
// rows per chunk of a launch of n rows whose slabs take row_bytes per row and stay below `budget` together: a multiple of BLOCK,
// at most n.  GH_TEST_SLAB_ROWS=R (test support, read on every call; R <= 0 or unset: nothing changes) caps a chunk at R rows
// rounded up to a multiple of BLOCK, so that a test reaches the chunks after the first at a few hundred rows; while it is set,
// every launch says on stderr how it was cut (`loop` names the caller).
inline size_t slab_chunk_rows(const char* loop, size_t budget, size_t row_bytes, size_t n) {
    size_t rows = std::max<size_t>(BLOCK, (budget / row_bytes) / BLOCK * BLOCK);
    const int knob = gh_rt::env_int("GH_TEST_SLAB_ROWS", 0);
    if (knob > 0) rows = std::min(rows, ((size_t)knob + BLOCK - 1) / BLOCK * BLOCK);
    const size_t chunk = std::min(n, rows);
    if (knob > 0) fprintf(stderr, "[gh] slab chunks: %s n=%zu rows=%zu chunks=%zu\n", loop, n, chunk, chunk ? (n + chunk - 1) / chunk : (size_t)0);
    return chunk;
}
template <int W> size_t vb_chunk(const char* loop, size_t n, int slabs) {
    return slab_chunk_rows(loop, VB_SLAB_BYTES, vb_row_bytes<W>() * slabs, n);
}

// one table of (+-) P per row, then d_out[j][i] = d_k[j]_i (+-) P_i for each of the `count` scalar vectors (n x 24 words,
// canonical) as internal Proj<C>, on g.stream
template <class C, int W>
int vb_single(const void* d_xy, const uint8_t* d_inf, int negate, const uint32_t* const* d_k, Proj<C>* const* d_out, int count, size_t n) {
    const size_t chunk = vb_chunk<W>("vb_single", n, 1);
    uint32_t* slab = nullptr;
    if (int rc = gh_rt::pool_get("vb_slab", chunk * vb_row_bytes<W>(), (void**)&slab)) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t cnt = std::min(chunk, n - r0);
        GH_LAUNCH((vb_table_kernel<C, W>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_xy, d_inf, r0, cnt, negate,
                  slab);
        for (int j = 0; j < count; j++)
            GH_LAUNCH((vb_mul_kernel<C, W>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)slab, d_k[j], d_inf, r0, cnt,
                      d_out[j]);
    }
    HIPCHK(hipGetLastError());
    return GH_OK;
}

// ---- the pipeline steps
template <class C>
int launch_normalize(Proj<C>* a, const Proj<C>* b, size_t n, Fp* zp, void* out_xy, size_t row_words, size_t off, uint8_t* out_inf) {
    GH_LAUNCH((normalize_kernel<C>), dim3(blocks(blocks(n, NORM_RUN), BLOCK)), dim3(BLOCK), 0, g.stream, a, b, n, zp, (uint32_t*)out_xy,
              row_words, off, out_inf);
    return GH_OK;
}

// pk = sk G through the handle's table
template <class C> int run_public_keys(GeneratorTable& gt, gh_curve_t curve, const uint64_t* sk, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    typedef typename Scheme<C>::PS PS;
    if (int rc = gt.ensure(curve, n)) return rc;
    uint64_t *d_sk, *d_xy;
    uint32_t* d_k;
    Proj<C>* d_p;
    Fp* d_zp;
    uint8_t* d_inf;
    int rc = dbuf("vb_in", n * 12, &d_sk);
    if (!rc) rc = dbuf("vb_k", n * 24, &d_k);
    if (!rc) rc = dbuf("vb_p", n, &d_p);
    if (!rc) rc = dbuf("vb_zp", n, &d_zp);
    if (!rc) rc = dbuf("vb_xy", n * 24, &d_xy);
    if (!rc) rc = dbuf("vb_inf", n, &d_inf);
    if (rc || (rc = up(d_sk, sk, n * 12))) return rc;
    GH_LAUNCH((mont_to_int_kernel<PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_sk, n, d_k, (uint8_t*)nullptr);
    if ((rc = gh_rt::fixed_table_sums(gt.table, d_k, n, d_p)) || (rc = launch_normalize<C>(d_p, nullptr, n, d_zp, d_xy, 48, 0, d_inf))) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_xy, d_xy, n * 192, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_inf, d_inf, n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return GH_OK;
}
// the body of gh_*_public_keys after the handle check
inline int public_keys_api(GeneratorTable& gt, gh_curve_t curve, const uint64_t* sk, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    if (n && (!sk || !out_xy || !out_inf)) return null_arg();
    size_t b;
    if (mul_overflows(n, 1024, &b)) return too_large();
    if (!GH_G1_DISPATCH(curve, scalar_below, sk, n)) { g_err = "a secret key is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = gh_rt::ensure_init()) return rc;
    return GH_G1_DISPATCH(curve, run_public_keys, gt, curve, sk, n, out_xy, out_inf);
}

template <class C> int run_keyverify(const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok) {
    uint64_t* d_pk;
    uint8_t *d_inf, *d_ok;
    int rc = dbuf("vb_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("vb_pkinf", n, &d_inf);
    if (!rc) rc = dbuf("vb_ok", n, &d_ok);
    if (rc || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_inf, pk_inf, n))) return rc;
    GH_LAUNCH((on_curve_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_pk, (const uint8_t*)d_inf, n, curve_b<C>(),
              d_ok);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_ok, d_ok, n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return GH_OK;
}

// ---- the argument checks
// sizes and the moduli of pk and the message (msg null: none), shared by sign / verify / prove / proof_to_hash / keyverify
template <class C> int check_rows(const uint64_t* pk_xy, const uint64_t* msg, size_t n, size_t len) {
    size_t nm = 0, b = 0;
    if (mul_overflows(n, len, &nm) || mul_overflows(nm, 96 * 4, &b) || mul_overflows(n, 1024, &b)) return too_large();
    if (!data_below<C>(pk_xy, 2 * n)) { g_err = "a public-key coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (msg && !data_below<C>(msg, nm)) { g_err = "a message element is not below the modulus"; return GH_E_BAD_ARG; }
    return GH_OK;
}
// the body of gh_*_keyverify after the handle check
inline int keyverify_api(gh_curve_t curve, const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok) {
    if (n && (!pk_xy || !pk_inf || !out_ok)) return null_arg();
    if (int rc = GH_G1_DISPATCH(curve, check_rows, pk_xy, nullptr, n, 0)) return rc;
    if (n == 0) return GH_OK;
    if (int rc = gh_rt::ensure_init()) return rc;
    return GH_G1_DISPATCH(curve, run_keyverify, pk_xy, pk_inf, n, out_ok);
}
// what gh_*_create checks of the curve, the window and the hash; `scheme` names the caller in the message
inline int check_create(const char* scheme, gh_curve_t curve, gh_poseidon* hash, int window) {
    if (!is_g1(curve)) { g_err = std::string("the ") + scheme + " group must be a G1 curve"; return GH_E_BAD_ARG; }
    if (window < 0 || window > 22) { g_err = "fixed-base window must be 0 or in [1, 22]"; return GH_E_BAD_ARG; }
    gh_field_t f;
    if (gh_rt::poseidon_field(hash, &f)) { g_err = "not a Poseidon handle"; return GH_E_BAD_ARG; }
    const gh_field_t need = curve == GH_MNT6753_G1 ? Scheme<Mnt6G1>::field : Scheme<Mnt4G1>::field;
    if (f != need) { g_err = "the hash's field is not the curve's base field"; return GH_E_BAD_ARG; }
    return GH_OK;
}
// what gh_batch_mul / gh_batch_double_mul (`fn`) check of the curve, the pointers (non_null) and the row count
inline int check_batch(const char* fn, gh_curve_t curve, size_t n, bool non_null) {
    if (curve == GH_MNT4753_G2 || curve == GH_MNT6753_G2) { g_err = std::string(fn) + ": G1 curves only"; return GH_E_UNSUPPORTED; }
    if (!is_g1(curve)) { g_err = "unknown curve id"; return GH_E_BAD_ARG; }
    if (n && !non_null) return null_arg();
    size_t b;
    if (mul_overflows(n, 1024, &b)) return too_large();
    return GH_OK;
}
inline bool below_2_753(const uint64_t* k, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (k[12 * i + 11] >> 49) return false;
    return true;
}

}  // namespace
