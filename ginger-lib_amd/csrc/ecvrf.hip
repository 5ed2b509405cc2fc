// ecvrf.hip -- the C ABI of include/ginger_hip_ecvrf.h: the Bowe-Hopwood Pedersen hash (primitives/src/crh/bowe_hopwood), the
// batched joint double-scalar multiplication gh_batch_double_mul, and the field-based EC-VRF (primitives/src/vrf/ecvrf) built on
// them, on the variable-base kernels of vb_kernels.h, the fixed-base path of fixed_base.hip and the Poseidon kernels of
// poseidon.hip.  DESIGN.md section 13.
//
// Bowe-Hopwood, one lane per row:
//   bh_table_kernel   {1, 2, 3, 4} g of every generator, affine (one doubling, one addition, one doubling, then Montgomery's trick
//                     over the three Z with ONE fp_inv); segment-major in global memory: 128 x 2 generators take 213 KB, more
//                     than the LDS holds, and every lane reads the same generator's entries at a step, so the table stays in cache
//   bh_hash_kernel    chunk t (bits 3t .. 3t + 2 of the little-endian input, zero-padded) adds (1 - 2 c2)(1 + c0 + 2 c1) g_t:
//                     ONE mixed addition of +-entry per chunk, generators at infinity skipped (proj_madd must not see infinity)
// Joint double-scalar multiplication, one lane per row:
//   vb_mul2_kernel    k1 P1 + k2 P2 from two vb_table_kernel slabs: W doublings per digit position and one mixed addition from
//                     each table, both scalars recoded by vb_digit as k | 1, then the two corrections for an even scalar.  A row
//                     whose base is at infinity skips that base (its slab is not read).
// The VRF runs every step on g.stream; only inputs, statuses and results cross PCIe.
#include <vector>
#include "vb_kernels.h"
#include "../../include/ginger_hip_ecvrf.h"

struct gh_bh {
    uint32_t magic = 0x67684268u;
    gh_curve_t curve;
    size_t num_windows = 0, window_size = 0;
    std::vector<uint64_t> gen_xy;         // host copy, segment-major x || y rows
    std::vector<uint8_t> gen_inf;
    gh_rt::DevMem d_tab;                  // {1, 2, 3, 4} g as Aff<C>, built on first use
    gh_rt::DevMem d_inf;                  // the generators' infinity bytes
};

struct gh_ecvrf {
    uint32_t magic = 0x67685672u;
    gh_curve_t curve;
    gh_poseidon_t hash = nullptr;
    gh_bh_t bh = nullptr;
    GeneratorTable gen;
};

namespace {

constexpr int VB_W = 4;                               // gh_batch_mul's default window
constexpr int BH_ENTRIES = 4;                         // {1, 2, 3, 4} g
enum { PH_UPLOAD, PH_GROUP_HASH, PH_FIXED_BASE, PH_VARIABLE_BASE, PH_NORMALISE, PH_HASH, PH_FINISH, NPHASES };
PhaseTimer g_tm{NPHASES};

// ---------------------------------------------------------------------------------------------------- Bowe-Hopwood
template <class C>
__global__ void __launch_bounds__(BLOCK) bh_table_kernel(const uint32_t* __restrict__ gen /* ng x 48 words, ABI */,
                                                         const uint8_t* __restrict__ inf, size_t ng, Aff<C>* __restrict__ tab) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ng) return;
    if (inf[i]) return;                                      // skipped by bh_hash_kernel: never read
    const Proj<C> p1{fp_from_abi<PF>(gen + i * 48), fp_from_abi<PF>(gen + i * 48 + 24), F::one()};
    const Proj<C> p2 = proj_dbl_call<C>(p1);
    const Proj<C> p3 = proj_add_call<C>(p2, p1);
    const Proj<C> p4 = proj_dbl_call<C>(p2);
    // G1 has prime order > 4: no Z is zero for a generator on the curve (gh_bh_create checks that)
    const Fp z23 = F::mul(p2.z, p3.z);
    Fp inv = fp_inv<PF>(F::mul(z23, p4.z));
    const Fp i4 = F::mul(inv, z23);
    inv = F::mul(inv, p4.z);                                 // 1 / (Z2 Z3)
    const Fp i3 = F::mul(inv, p2.z), i2 = F::mul(inv, p3.z);
    Aff<C>* o = tab + i * BH_ENTRIES;
    st_words(o, Aff<C>{p1.x, p1.y});
    st_words(o + 1, Aff<C>{F::mul(p2.x, i2), F::mul(p2.y, i2)});
    st_words(o + 2, Aff<C>{F::mul(p3.x, i3), F::mul(p3.y, i3)});
    st_words(o + 3, Aff<C>{F::mul(p4.x, i4), F::mul(p4.y, i4)});
}

// row i: nbytes bytes at in + i * stride; chunks [0, nchunks) with nchunks = ceil(8 nbytes / 3) <= the generators
template <class C>
__global__ void __launch_bounds__(BLOCK) bh_hash_kernel(const Aff<C>* __restrict__ tab, const uint8_t* __restrict__ ginf,
                                                        const uint8_t* __restrict__ in, size_t stride, size_t nbytes, size_t nchunks,
                                                        size_t n, Proj<C>* __restrict__ out) {
    typedef typename C::F F;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* row = in + i * stride;
    Proj<C> q = proj_zero<C>();
#pragma unroll 1
    for (size_t t = 0; t < nchunks; t++) {
        if (ginf[t]) continue;                               // the same t in every lane: no divergence
        const size_t bit = 3 * t, byte = bit >> 3;          // 3 t < 8 nbytes: byte < nbytes
        uint32_t two = row[byte];
        if (byte + 1 < nbytes) two |= (uint32_t)row[byte + 1] << 8;
        const uint32_t c = (two >> (bit & 7)) & 7u;
        Aff<C> a = ld_words(tab + t * BH_ENTRIES + (c & 3u));   // magnitude 1 + c0 + 2 c1
        const Fp ny = F::neg(a.y);
        if (c & 4u) a.y = ny;
        q = proj_madd<C>(q, a);
    }
    st_words(out + i, q);
}

// ---------------------------------------------------------------------------------------------------- joint double-scalar
// out[i] = k1_i P1_i + k2_i P2_i from the two slabs of vb_table_kernel (the signs of the bases were applied there)
template <class C, int W>
__global__ void __launch_bounds__(BLOCK)
vb_mul2_kernel(const uint32_t* __restrict__ slab1, const uint32_t* __restrict__ k1 /* n x 24 words, canonical */,
               const uint8_t* __restrict__ inf1, const uint32_t* __restrict__ slab2, const uint32_t* __restrict__ k2,
               const uint8_t* __restrict__ inf2, size_t row0, size_t cnt, Proj<C>* __restrict__ out) {
    typedef typename C::F F;
    constexpr int M = VbWindow<W>::M;
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const size_t i = row0 + t;
    const bool on1 = !(inf1 && inf1[i]), on2 = !(inf2 && inf2[i]);
    const RowSlab s1{const_cast<uint32_t*>(slab1) + t, cnt}, s2{const_cast<uint32_t*>(slab2) + t, cnt};
    const uint32_t *ka = k1 + i * 24, *kb = k2 + i * 24;
    auto entry = [&](int b, uint32_t idx, bool neg) {
        const RowSlab& s = b ? s2 : s1;
        Aff<C> a{s.ld(SLOTS_PER_ENTRY * idx), s.ld(SLOTS_PER_ENTRY * idx + 1)};
        const Fp ny = F::neg(a.y);
        if (neg) a.y = ny;
        return a;
    };
    Proj<C> q = proj_zero<C>();
    uint32_t idx;
    bool neg;
#pragma unroll 1
    for (int j = M - 1; j >= 0; j--) {
#pragma unroll 1
        for (int b = 0; b < W; b++) q = proj_dbl<C>(q);     // returns at once while q is infinity (the top digits)
#pragma unroll 1
        for (int b = 0; b < 2; b++) {
            if (!(b ? on2 : on1)) continue;
            vb_digit<W>(b ? kb : ka, j, idx, neg);
            q = proj_madd<C>(q, entry(b, idx, neg));
        }
    }
#pragma unroll 1
    for (int b = 0; b < 2; b++)
        if ((b ? on2 : on1) && !((b ? kb : ka)[0] & 1u)) q = proj_madd<C>(q, entry(b, 0, true));   // k was run as k | 1
    st_words(out + i, q);
}

// ---------------------------------------------------------------------------------------------------- pipeline kernels
// the c hash rows m_0 .. m_(len-1) | pk.x | a.x | b.x (u, v in proof_to_hash); a, b are normalize_kernel rows (n x 24 words)
__global__ void __launch_bounds__(256) c_rows_kernel(const uint64_t* __restrict__ msg, const uint64_t* __restrict__ pk_xy,
                                                     const uint8_t* __restrict__ pk_inf, const uint64_t* __restrict__ a_xy,
                                                     const uint64_t* __restrict__ b_xy, size_t n, size_t len, uint64_t* __restrict__ rows) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t* r = rows + i * (len + 3) * 12;
    for (size_t w = 0; w < len * 12; w++) r[w] = msg[i * len * 12 + w];
    const bool zero = pk_inf[i] != 0;
    for (int w = 0; w < 12; w++) {
        r[len * 12 + w] = zero ? 0ull : pk_xy[i * 24 + w];
        r[(len + 1) * 12 + w] = a_xy[i * 24 + w];
        r[(len + 2) * 12 + w] = b_xy[i * 24 + w];
    }
}

// the output hash rows m_0 .. m_(len-1) | gamma.x | gamma.y, gamma at infinity as (0, 1)
template <class C>
__global__ void __launch_bounds__(256) out_rows_kernel(const uint64_t* __restrict__ msg, const uint64_t* __restrict__ gamma_xy,
                                                       const uint8_t* __restrict__ gamma_inf, size_t n, size_t len,
                                                       uint64_t* __restrict__ rows) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t* r = rows + i * (len + 2) * 12;
    for (size_t w = 0; w < len * 12; w++) r[w] = msg[i * len * 12 + w];
    if (gamma_inf[i]) {
        for (int w = 0; w < 12; w++) r[len * 12 + w] = 0ull;
        fp_to_abi<PF>((uint32_t*)(r + (len + 1) * 12), F::one());
        return;
    }
    for (int w = 0; w < 24; w++) r[len * 12 + w] = gamma_xy[i * 24 + w];
}

// proof_to_hash, last step: status 2 (range) stays, then 3 for gamma off the curve, then 1 if c' == c, 0 if not; out rows zeroed
// unless the status is 1
__global__ void __launch_bounds__(256) verdict_kernel(const uint64_t* __restrict__ c2, const uint64_t* __restrict__ cs,
                                                      const uint8_t* __restrict__ gamma_ok, size_t n, uint64_t* __restrict__ out,
                                                      uint8_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t st = status[i];
    if (st != 2) {
        bool eq = true;
        for (int w = 0; w < 12; w++) eq &= c2[i * 12 + w] == cs[i * 24 + w];
        st = !gamma_ok[i] ? 3 : eq ? 1 : 0;
    }
    status[i] = st;
    if (st != 1)
        for (int w = 0; w < 12; w++) out[i * 12 + w] = 0ull;
}

// ---------------------------------------------------------------------------------------------------- host side
// the generators' table on the device, on first use
template <class C> int bh_ensure(gh_bh* b) {
    if (b->d_tab.get()) return GH_OK;
    const size_t ng = b->num_windows * b->window_size;
    gh_rt::DevMem d_gen, d_tab, d_inf;     // table and flags move into the handle once the table is built
    int rc;
    if ((rc = d_tab.alloc(ng * BH_ENTRIES * sizeof(Aff<C>))) || (rc = d_inf.alloc(ng)) || (rc = d_gen.alloc(ng * 192))) return rc;
    HIPCHK(hipMemcpyAsync(d_gen.get(), b->gen_xy.data(), ng * 192, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_inf.get(), b->gen_inf.data(), ng, hipMemcpyHostToDevice, g.stream));
    GH_LAUNCH(bh_table_kernel<C>, dim3(blocks(ng, BLOCK)), dim3(BLOCK), 0, g.stream, d_gen.as<const uint32_t>(),
              d_inf.as<const uint8_t>(), ng, d_tab.as<Aff<C>>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.stream));
    b->d_tab = std::move(d_tab);
    b->d_inf = std::move(d_inf);
    return GH_OK;
}

// d_p[i] = BH of row i (nbytes bytes at d_in + i * stride) as internal Proj<C>, on g.stream
template <class C> int bh_launch(gh_bh* b, const uint8_t* d_in, size_t stride, size_t nbytes, size_t n, Proj<C>* d_p) {
    if (int rc = bh_ensure<C>(b)) return rc;
    const size_t nchunks = (8 * nbytes + 2) / 3;
    GH_LAUNCH((bh_hash_kernel<C>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, b->d_tab.as<const Aff<C>>(), b->d_inf.as<const uint8_t>(),
              d_in, stride, nbytes, nchunks, n, d_p);
    HIPCHK(hipGetLastError());
    return GH_OK;
}

// out[i] = k1_i (+-) P1_i + k2_i (+-) P2_i, on g.stream
template <class C> int vb_joint(const void* d_xy1, const uint8_t* d_inf1, int neg1, const uint32_t* d_k1, const void* d_xy2,
                                const uint8_t* d_inf2, int neg2, const uint32_t* d_k2, size_t n, Proj<C>* d_out) {
    const size_t chunk = vb_chunk<VB_W>("vb_joint", n, 2);
    uint32_t *slab1 = nullptr, *slab2 = nullptr;
    if (int rc = gh_rt::pool_get("vb_slab", chunk * vb_row_bytes<VB_W>(), (void**)&slab1)) return rc;
    if (int rc = gh_rt::pool_get("vb_slab2", chunk * vb_row_bytes<VB_W>(), (void**)&slab2)) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t cnt = std::min(chunk, n - r0);
        GH_LAUNCH((vb_table_kernel<C, VB_W>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_xy1, d_inf1, r0, cnt,
                  neg1, slab1);
        GH_LAUNCH((vb_table_kernel<C, VB_W>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)d_xy2, d_inf2, r0, cnt,
                  neg2, slab2);
        GH_LAUNCH((vb_mul2_kernel<C, VB_W>), dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, g.stream, (const uint32_t*)slab1, d_k1, d_inf1,
                  (const uint32_t*)slab2, d_k2, d_inf2, r0, cnt, d_out);
    }
    HIPCHK(hipGetLastError());
    return GH_OK;
}

bool valid(const gh_bh* h) { return h && h->magic == 0x67684268u; }

// mh = BH(to_bytes(m_0) || ... ) of the Montgomery message rows on the device, normalised: x || y rows (n x 24 words) and infinity
template <class C> int message_on_curve(gh_bh* b, const uint64_t* d_msg, size_t n, size_t len, uint32_t* d_mint, Proj<C>* d_p, Fp* d_zp,
                                        uint64_t* d_mh, uint8_t* d_mhinf) {
    typedef typename Scheme<C>::PF PF;
    if (n * len) GH_LAUNCH((mont_to_int_kernel<PF>), dim3(blocks(n * len, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_msg, n * len, d_mint,
                           (uint8_t*)nullptr);
    if (int rc = bh_launch<C>(b, (const uint8_t*)d_mint, len * 96, len * 96, n, d_p)) return rc;
    if (int rc = launch_normalize<C>(d_p, nullptr, n, d_zp, d_mh, 48, 0, d_mhinf)) return rc;
    HIPCHK(hipGetLastError());
    return GH_OK;
}

template <class C> int run_bh_hash(gh_bh* b, const uint8_t* input, size_t n, size_t nbytes, uint64_t* out_xy, uint8_t* out_inf) {
    uint8_t *d_in, *d_inf;
    Proj<C>* d_p;
    Fp* d_zp;
    uint64_t* d_xy;
    int rc = dbuf("vb_in", n * nbytes, &d_in);
    if (!rc) rc = dbuf("vb_p", n, &d_p);
    if (!rc) rc = dbuf("vb_zp", n, &d_zp);
    if (!rc) rc = dbuf("vb_xy", n * 24, &d_xy);
    if (!rc) rc = dbuf("vb_inf", n, &d_inf);
    if (rc || (rc = up(d_in, input, n * nbytes)) || (rc = bh_ensure<C>(b))) return rc;
    if ((rc = g_tm.begin().mark()) || (rc = bh_launch<C>(b, d_in, nbytes, nbytes, n, d_p)) || (rc = g_tm.mark())) return rc;
    if ((rc = launch_normalize<C>(d_p, nullptr, n, d_zp, d_xy, 48, 0, d_inf))) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_xy, d_xy, n * 192, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_inf, d_inf, n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return g_tm.single(PH_GROUP_HASH);                         // the hash kernel
}

template <class C> int run_double_mul(const uint64_t* xy1, const uint8_t* inf1, const uint64_t* k1, const uint64_t* xy2, const uint8_t* inf2,
                                      const uint64_t* k2, size_t n, uint64_t* out_xyz) {
    uint64_t *d_xy, *d_k, *d_out;
    uint8_t* d_inf = nullptr;
    Proj<C>* d_p;
    int rc = dbuf("vb_pk", n * 48, &d_xy);
    if (!rc) rc = dbuf("vb_k", n * 24, &d_k);
    if (!rc) rc = dbuf("vb_p", n, &d_p);
    if (!rc) rc = dbuf("vb_rows", n * 36, &d_out);
    if (!rc && (inf1 || inf2)) rc = dbuf("vb_inf", 2 * n, &d_inf);
    if (rc || (rc = up(d_xy, xy1, n * 24)) || (rc = up(d_xy + n * 24, xy2, n * 24)) || (rc = up(d_k, k1, n * 12)) ||
        (rc = up(d_k + n * 12, k2, n * 12)))
        return rc;
    if (d_inf) {
        HIPCHK(hipMemsetAsync(d_inf, 0, 2 * n, g.stream));
        if ((inf1 && (rc = up(d_inf, inf1, n))) || (inf2 && (rc = up(d_inf + n, inf2, n)))) return rc;
    }
    if ((rc = g_tm.begin().mark()) ||
        (rc = vb_joint<C>(d_xy, d_inf, 0, (const uint32_t*)d_k, d_xy + n * 24, d_inf ? d_inf + n : nullptr, 0, (const uint32_t*)(d_k + n * 12),
                          n, d_p)) ||
        (rc = g_tm.mark()))
        return rc;
    GH_LAUNCH((proj_to_abi_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const Proj<C>*)d_p, n, (uint32_t*)d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_xyz, d_out, n * 288, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return g_tm.single(PH_VARIABLE_BASE);                      // the tables and the joint kernel
}

// prove: mh = BH(m); gamma = sk mh and b = r mh from ONE table of mh; a = r G on the fixed-base path; c = H(m || pk.x || a.x || b.x);
// s = r + sk c (sign_finish_kernel, with Schnorr's range checks)
template <class C> int run_prove(gh_ecvrf* h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n,
                                 size_t len, const uint64_t* nonce, uint64_t* out_gamma_xy, uint8_t* out_gamma_inf, uint64_t* out_cs,
                                 uint8_t* out_status) {
    typedef typename Scheme<C>::PF PF;
    typedef typename Scheme<C>::PS PS;
    if (int rc = h->gen.ensure(h->curve, n)) return rc;
    const size_t rw = (len + 3) * 12;
    uint64_t *d_sk, *d_nonce, *d_pk, *d_msg, *d_mh, *d_xy3, *d_rows, *d_c, *d_cs;
    uint8_t *d_pkinf, *d_mhinf, *d_inf3, *d_st;
    uint32_t *d_mint, *d_ski, *d_ri;
    Proj<C>* d_p3;                                           // a | b | gamma
    Fp* d_zp;
    int rc = dbuf("vb_in", n * 24, &d_sk);
    if (!rc) rc = dbuf("vb_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("vb_pkinf", n, &d_pkinf);
    if (!rc) rc = dbuf("vb_msg", n * len * 12, &d_msg);
    if (!rc) rc = dbuf("vb_msgint", n * len * 24, &d_mint);
    if (!rc) rc = dbuf("vb_gm", n * 24, &d_mh);
    if (!rc) rc = dbuf("vb_gminf", n, &d_mhinf);
    if (!rc) rc = dbuf("vb_k", n * 48, &d_ski);
    if (!rc) rc = dbuf("vb_p", 3 * n, &d_p3);
    if (!rc) rc = dbuf("vb_zp", 3 * n, &d_zp);
    if (!rc) rc = dbuf("vb_xy", 3 * n * 24, &d_xy3);
    if (!rc) rc = dbuf("vb_inf", 3 * n, &d_inf3);
    if (!rc) rc = dbuf("vb_rows", n * rw, &d_rows);
    if (!rc) rc = dbuf("vb_h", n * 12, &d_c);
    if (!rc) rc = dbuf("vb_cs", n * 24, &d_cs);
    if (!rc) rc = dbuf("vb_st", n, &d_st);
    if (rc) return rc;
    d_nonce = d_sk + n * 12;
    d_ri = d_ski + n * 24;
    Proj<C>*d_a = d_p3, *d_b = d_p3 + n, *d_g = d_p3 + 2 * n;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_sk, sk, n * 12)) || (rc = up(d_nonce, nonce, n * 12)) || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_pkinf, pk_inf, n)) ||
        (rc = up(d_msg, msg, n * len * 12)) || (rc = ph.mark()))
        return rc;
    if ((rc = message_on_curve<C>(h->bh, d_msg, n, len, d_mint, d_a, d_zp, d_mh, d_mhinf)) || (rc = ph.mark())) return rc;
    GH_LAUNCH((mont_to_int_kernel<PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_sk, n, d_ski, (uint8_t*)nullptr);
    GH_LAUNCH((mont_to_int_kernel<PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_nonce, n, d_ri, d_st);
    if ((rc = gh_rt::fixed_table_sums(h->gen.table, d_ri, n, d_a)) || (rc = ph.mark())) return rc;                       // a = r G
    const uint32_t* ks[2] = {d_ski, d_ri};
    Proj<C>* outs[2] = {d_g, d_b};
    if ((rc = vb_single<C, VB_W>(d_mh, d_mhinf, 0, ks, outs, 2, n)) || (rc = ph.mark())) return rc;                        // gamma, b
    if ((rc = launch_normalize<C>(d_p3, nullptr, 3 * n, d_zp, d_xy3, 48, 0, d_inf3))) return rc;
    GH_LAUNCH(c_rows_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_msg, (const uint64_t*)d_pk, (const uint8_t*)d_pkinf,
              (const uint64_t*)d_xy3, (const uint64_t*)(d_xy3 + n * 24), n, len, d_rows);
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    if ((rc = gh_rt::poseidon_hash_dev_locked(h->hash, d_rows, n, len + 3, d_c)) || (rc = ph.mark())) return rc;
    GH_LAUNCH((sign_finish_kernel<PF, PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_c, (const uint32_t*)d_sk,
              (const uint32_t*)d_nonce, n, (uint32_t*)d_cs, d_st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_cs, d_cs, n * 192, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_gamma_xy, d_xy3 + 2 * n * 24, n * 192, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_gamma_inf, d_inf3 + 2 * n, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

// proof_to_hash: range checks and gamma's on-curve test, mh = BH(m), u = s G + c (-pk), v = s mh + c (-gamma) in one joint kernel,
// c' = H(m || pk.x || u.x || v.x), the verdict, and the output H(m || gamma.x || gamma.y)
template <class C> int run_proof_to_hash(gh_ecvrf* h, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                                         const uint64_t* gamma_xy, const uint8_t* gamma_inf, const uint64_t* cs, uint64_t* out_hash,
                                         uint8_t* out_status) {
    typedef typename Scheme<C>::PF PF;
    if (int rc = h->gen.ensure(h->curve, n)) return rc;
    const size_t rw = (len + 3) * 12;
    uint64_t *d_cs, *d_pk, *d_gm, *d_msg, *d_mh, *d_xy2, *d_rows, *d_c2, *d_out;
    uint8_t *d_pkinf, *d_gminf, *d_mhinf, *d_st, *d_ok;
    uint32_t *d_mint, *d_ci;
    Proj<C>* d_p3;                                           // s G | c (-pk) | v
    Fp* d_zp;
    int rc = dbuf("vb_cs", n * 24, &d_cs);
    if (!rc) rc = dbuf("vb_pk", n * 24, &d_pk);
    if (!rc) rc = dbuf("vb_pkinf", n, &d_pkinf);
    if (!rc) rc = dbuf("vb_gamma", n * 24, &d_gm);
    if (!rc) rc = dbuf("vb_gammainf", n, &d_gminf);
    if (!rc) rc = dbuf("vb_msg", n * len * 12, &d_msg);
    if (!rc) rc = dbuf("vb_msgint", n * len * 24, &d_mint);
    if (!rc) rc = dbuf("vb_gm", n * 24, &d_mh);
    if (!rc) rc = dbuf("vb_gminf", n, &d_mhinf);
    if (!rc) rc = dbuf("vb_k", n * 48, &d_ci);
    if (!rc) rc = dbuf("vb_p", 3 * n, &d_p3);
    if (!rc) rc = dbuf("vb_zp", 2 * n, &d_zp);
    if (!rc) rc = dbuf("vb_xy", 2 * n * 24, &d_xy2);
    if (!rc) rc = dbuf("vb_rows", n * rw, &d_rows);
    if (!rc) rc = dbuf("vb_h", n * 24, &d_c2);
    if (!rc) rc = dbuf("vb_st", n, &d_st);
    if (!rc) rc = dbuf("vb_ok", n, &d_ok);
    if (rc) return rc;
    uint32_t* d_si = d_ci + n * 24;
    d_out = d_c2 + n * 12;
    Proj<C>*d_sg = d_p3, *d_cpk = d_p3 + n, *d_v = d_p3 + 2 * n;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if ((rc = up(d_cs, cs, n * 24)) || (rc = up(d_pk, pk_xy, n * 24)) || (rc = up(d_pkinf, pk_inf, n)) || (rc = up(d_gm, gamma_xy, n * 24)) ||
        (rc = up(d_gminf, gamma_inf, n)) || (rc = up(d_msg, msg, n * len * 12)) || (rc = ph.mark()))
        return rc;
    GH_LAUNCH((sig_prep_kernel<PF>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_cs, n, d_ci, d_si, d_st);
    GH_LAUNCH((on_curve_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_gm, (const uint8_t*)d_gminf, n,
              curve_b<C>(), d_ok);
    if ((rc = message_on_curve<C>(h->bh, d_msg, n, len, d_mint, d_sg, d_zp, d_mh, d_mhinf)) || (rc = ph.mark())) return rc;
    if ((rc = gh_rt::fixed_table_sums(h->gen.table, d_si, n, d_sg)) || (rc = ph.mark())) return rc;                      // s G
    const uint32_t* ks[1] = {d_ci};
    Proj<C>* outs[1] = {d_cpk};
    if ((rc = vb_single<C, VB_W>(d_pk, d_pkinf, 1, ks, outs, 1, n)) ||                                                      // c (-pk)
        (rc = vb_joint<C>(d_mh, d_mhinf, 0, d_si, d_gm, d_gminf, 1, d_ci, n, d_v)) || (rc = ph.mark()))              // s mh + c (-gamma)
        return rc;
    if ((rc = launch_normalize<C>(d_sg, d_cpk, n, d_zp, d_xy2, 48, 0, nullptr)) ||                                  // u
        (rc = launch_normalize<C>(d_v, nullptr, n, d_zp + n, d_xy2 + n * 24, 48, 0, nullptr)))                    // v
        return rc;
    GH_LAUNCH(c_rows_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_msg, (const uint64_t*)d_pk, (const uint8_t*)d_pkinf,
              (const uint64_t*)d_xy2, (const uint64_t*)(d_xy2 + n * 24), n, len, d_rows);
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    if ((rc = gh_rt::poseidon_hash_dev_locked(h->hash, d_rows, n, len + 3, d_c2))) return rc;                        // c'
    GH_LAUNCH((out_rows_kernel<C>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_msg, (const uint64_t*)d_gm,
              (const uint8_t*)d_gminf, n, len, d_rows);
    if ((rc = gh_rt::poseidon_hash_dev_locked(h->hash, d_rows, n, len + 2, d_out)) || (rc = ph.mark())) return rc;   // the output
    GH_LAUNCH(verdict_kernel, dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint64_t*)d_c2, (const uint64_t*)d_cs, (const uint8_t*)d_ok,
              n, d_out, d_st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_hash, d_out, n * 96, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(out_status, d_st, n, hipMemcpyDeviceToHost, g.stream));
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

// the checks prove / proof_to_hash share: sizes, the group hash's capacity, the moduli of pk and the message
template <class C> int check_common(const gh_ecvrf* h, const uint64_t* pk_xy, const uint64_t* msg, size_t n, size_t len) {
    if (len > h->bh->num_windows * h->bh->window_size / 256) {
        g_err = "the message is longer than the group hash takes (768 len > 3 num_windows window_size)";
        return GH_E_BAD_ARG;
    }
    return check_rows<C>(pk_xy, msg, n, len);
}

int checked(gh_ecvrf* h) {
    if (!h || h->magic != 0x67685672u) { g_err = "not an EC-VRF handle"; return GH_E_BAD_HANDLE; }
    return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

extern "C" {

int gh_bh_create(gh_curve_t curve, const uint64_t* gen_xy, const uint8_t* gen_inf, size_t num_windows, size_t window_size, gh_bh_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!out) return null_arg();
    *out = nullptr;
    if (!is_g1(curve)) { g_err = "the Bowe-Hopwood group must be a G1 curve"; return GH_E_BAD_ARG; }
    size_t ng = 0, b = 0;
    if (!num_windows || !window_size || mul_overflows(num_windows, window_size, &ng) || mul_overflows(ng, 192 * 8, &b)) {
        g_err = "num_windows and window_size must be positive and their product small enough";
        return GH_E_BAD_ARG;
    }
    if (!gen_xy) return null_arg();
    if (int rc = check_generators(curve, "", gen_xy, gen_inf, ng)) return rc;
    auto* h = new gh_bh();
    h->curve = curve;
    h->num_windows = num_windows;
    h->window_size = window_size;
    keep(h->gen_xy, h->gen_inf, gen_xy, gen_inf, ng);
    *out = h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_bh_free(gh_bh_t h) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!h) return GH_OK;
    if (!valid(h)) { g_err = "not a Bowe-Hopwood handle"; return GH_E_BAD_HANDLE; }
    if (h->d_tab.get()) (void)hipStreamSynchronize(g.stream);
    h->magic = 0;
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_bh_hash(gh_bh_t h, const uint8_t* input, size_t n, size_t nbytes, uint64_t* out_xy, uint8_t* out_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (!valid(h)) { g_err = "not a Bowe-Hopwood handle"; return GH_E_BAD_HANDLE; }
    if (n && ((nbytes && !input) || !out_xy || !out_inf)) return null_arg();
    size_t b = 0;
    if (mul_overflows(n, nbytes, &b) || mul_overflows(n, 1024, &b) || nbytes > (SIZE_MAX >> 4)) return too_large();
    if (8 * nbytes > 3 * h->num_windows * h->window_size) {
        g_err = "the input is longer than the parameters take (8 nbytes > 3 num_windows window_size)";
        return GH_E_BAD_ARG;
    }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_G1_DISPATCH(h->curve, run_bh_hash, h, input, n, nbytes, out_xy, out_inf);
} catch (...) { return gh_rt::api_exception(); }

int gh_batch_double_mul(gh_curve_t curve, const uint64_t* xy1, const uint8_t* inf1, const uint64_t* k1, const uint64_t* xy2, const uint8_t* inf2,
                        const uint64_t* k2, size_t n, uint64_t* out_xyz) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = check_batch("gh_batch_double_mul", curve, n, xy1 && k1 && xy2 && k2 && out_xyz)) return rc;
    if (!GH_G1_DISPATCH(curve, data_below, xy1, 2 * n) || !GH_G1_DISPATCH(curve, data_below, xy2, 2 * n)) {
        g_err = "a base coordinate is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (!below_2_753(k1, n) || !below_2_753(k2, n)) { g_err = "a scalar is not below 2^753"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_G1_DISPATCH(curve, run_double_mul, xy1, inf1, k1, xy2, inf2, k2, n, out_xyz);
} catch (...) { return gh_rt::api_exception(); }

int gh_ecvrf_create(gh_curve_t curve, gh_poseidon_t hash, gh_bh_t group_hash, int window, gh_ecvrf_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!hash || !group_hash || !out) return null_arg();
    *out = nullptr;
    if (int rc = check_create("EC-VRF", curve, hash, window)) return rc;
    if (!valid(group_hash)) { g_err = "not a Bowe-Hopwood handle"; return GH_E_BAD_ARG; }
    if (group_hash->curve != curve) { g_err = "the group hash is over another curve"; return GH_E_BAD_ARG; }
    auto* h = new gh_ecvrf();
    h->curve = curve;
    h->hash = hash;
    h->bh = group_hash;
    h->gen.window = window;
    *out = h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_ecvrf_free(gh_ecvrf_t h) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!h) return GH_OK;
    if (int rc = checked(h)) return rc;
    h->gen.destroy();
    h->magic = 0;
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_ecvrf_public_keys(gh_ecvrf_t h, const uint64_t* sk, size_t n, uint64_t* out_pk_xy, uint8_t* out_pk_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked(h)) return rc;
    return public_keys_api(h->gen, h->curve, sk, n, out_pk_xy, out_pk_inf);
} catch (...) { return gh_rt::api_exception(); }

int gh_ecvrf_prove(gh_ecvrf_t h, const uint64_t* sk, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                   const uint64_t* nonce, uint64_t* out_gamma_xy, uint8_t* out_gamma_inf, uint64_t* out_cs, uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked(h)) return rc;
    if (n && (!sk || !pk_xy || !pk_inf || (len && !msg) || !nonce || !out_gamma_xy || !out_gamma_inf || !out_cs || !out_status))
        return null_arg();
    if (int rc = GH_G1_DISPATCH(h->curve, check_common, h, pk_xy, len ? msg : nullptr, n, len)) return rc;
    if (!GH_G1_DISPATCH(h->curve, scalar_below, sk, n) || !GH_G1_DISPATCH(h->curve, scalar_below, nonce, n)) {
        g_err = "a secret key or nonce is not below the modulus";
        return GH_E_BAD_ARG;
    }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_G1_DISPATCH(h->curve, run_prove, h, sk, pk_xy, pk_inf, msg, n, len, nonce, out_gamma_xy, out_gamma_inf, out_cs, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_ecvrf_proof_to_hash(gh_ecvrf_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* msg, size_t n, size_t len,
                           const uint64_t* gamma_xy, const uint8_t* gamma_inf, const uint64_t* cs, uint64_t* out_hash, uint8_t* out_status) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked(h)) return rc;
    if (n && (!pk_xy || !pk_inf || (len && !msg) || !gamma_xy || !gamma_inf || !cs || !out_hash || !out_status))
        return null_arg();
    if (int rc = GH_G1_DISPATCH(h->curve, check_common, h, pk_xy, len ? msg : nullptr, n, len)) return rc;
    if (!GH_G1_DISPATCH(h->curve, data_below, gamma_xy, 2 * n)) { g_err = "a gamma coordinate is not below the modulus"; return GH_E_BAD_ARG; }
    if (!GH_G1_DISPATCH(h->curve, data_below, cs, 2 * n)) { g_err = "a proof element is not below the modulus"; return GH_E_BAD_ARG; }
    if (n == 0) return GH_OK;
    if (int rc = ensure_init()) return rc;
    return GH_G1_DISPATCH(h->curve, run_proof_to_hash, h, pk_xy, pk_inf, msg, n, len, gamma_xy, gamma_inf, cs, out_hash, out_status);
} catch (...) { return gh_rt::api_exception(); }

int gh_ecvrf_keyverify(gh_ecvrf_t h, const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n, uint8_t* out_ok) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    if (int rc = checked(h)) return rc;
    return keyverify_api(h->curve, pk_xy, pk_inf, n, out_ok);
} catch (...) { return gh_rt::api_exception(); }

int gh_ecvrf_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return g_tm.copy_out(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
