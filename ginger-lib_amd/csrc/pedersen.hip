// pedersen.hip -- the C ABI of include/ginger_hip_pedersen.h: the Pedersen hash (primitives/src/crh/pedersen) and the Pedersen
// commitment (primitives/src/commitment/pedersen) over the two G1 groups, on the host layer of unit_host.h and the normalisation
// and conversion kernels of vb_kernels.h.  DESIGN.md section 13a.
//
// Both are sums of fixed generators selected by input bits.  With t table bits (pedersen_digits.h) the generators are cut into
// groups of t and the table holds the 2^t - 1 subset sums of every group, so that a row costs one mixed addition per t bits:
//   ped_table_kernel        one lane per (position, m), 1 <= m < 2^t: the sum of the group's generators that m selects, by the
//                           complete out-of-line additions; generators at infinity are skipped
//   ped_table_norm_kernel   the sums to Aff<C> by Montgomery's trick over runs of NORM_RUN entries with ONE fp_inv per run, and
//                           an infinity byte per entry: a subset sum can cancel
//   ped_hash_kernel         one lane per row: the digit of every position, one inlined proj_madd where the digit is not zero
//                           and the entry not at infinity; a commitment goes on over the 753 bits of r with the table of the
//                           randomness generators.  proj_madd doubles where the accumulator equals the entry and gives
//                           infinity where it is the entry's negative; it never sees an entry at infinity.
// The randomness leaves Montgomery form on the device (mont_to_int_kernel): its 24 words are the bytes the loop reads.
#include <vector>
#include "vb_kernels.h"
#include "pedersen_digits.h"
#include "../../include/ginger_hip_pedersen.h"

struct gh_pedersen {
    static constexpr uint32_t MAGIC = 0x67685064u;
    uint32_t magic = MAGIC;
    gh_curve_t curve;
    size_t num_windows = 0, window_size = 0;
    size_t ng = 0;                        // G = num_windows * window_size
    int t = 0;                            // table bits
    std::vector<uint64_t> gen_xy, rand_xy;   // host copies, x || y rows; rand_xy empty: a handle that only hashes
    std::vector<uint8_t> gen_inf, rand_inf;
    gh_rt::DevMem d_tab, d_tinf;          // the generators' subset sums as Aff<C> and their infinity bytes, built on first use
    gh_rt::DevMem d_rtab, d_rtinf;        // the same of the randomness generators
};

namespace {

constexpr size_t RAND_BITS = VB_BITS;                 // 753 randomness generators: MODULUS_BITS of both scalar fields
constexpr int DEFAULT_TABLE_BITS = 8;
enum { PH_UPLOAD, PH_HASH, PH_NORMALISE, PH_FINISH, NPHASES };
PhaseTimer g_tm{NPHASES};

// entry e = ped_entry(t, p, m) of `count` generators: the sum of g_(p t + j) over the bits j of m, as Proj<C>
template <class C>
__global__ void __launch_bounds__(BLOCK) ped_table_kernel(const uint32_t* __restrict__ gen /* count x 48 words, ABI */,
                                                          const uint8_t* __restrict__ inf, size_t count, int t, size_t entries,
                                                          Proj<C>* __restrict__ sums) {
    typedef typename C::PF PF;
    const size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= entries) return;
    const size_t per = ped_entries_per_position(t), p = e / per;
    const uint32_t m = (uint32_t)(e % per) + 1;
    Proj<C> q = proj_zero<C>();
#pragma unroll 1
    for (int j = 0; j < t; j++) {
        const size_t f = p * (size_t)t + j;
        if (!((m >> j) & 1u) || f >= count || inf[f]) continue;   // beyond a partial group: no digit has that bit
        q = proj_madd_call<C>(q, Aff<C>{fp_from_abi<PF>(gen + f * 48), fp_from_abi<PF>(gen + f * 48 + 24)});
    }
    st_words(sums + e, q);
}

template <class C>
__global__ void __launch_bounds__(BLOCK) ped_table_norm_kernel(const Proj<C>* __restrict__ sums, size_t entries, Fp* __restrict__ zp,
                                                               Aff<C>* __restrict__ tab, uint8_t* __restrict__ tinf) {
    typedef typename C::FC F;
    typedef typename C::PF PF;
    const size_t i0 = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * NORM_RUN;
    if (i0 >= entries) return;
    const int cnt = (int)(entries - i0 < (size_t)NORM_RUN ? entries - i0 : (size_t)NORM_RUN);
    Fp run = F::one();
    for (int j = 0; j < cnt; j++) {
        const Fp z = ld_words(&sums[i0 + j].z);
        st_words(zp + i0 + j, run);
        if (!F::is_zero(z)) run = F::mul(run, z);
    }
    Fp inv = fp_inv<PF>(run);
    for (int j = cnt - 1; j >= 0; j--) {
        const Proj<C> p = ld_words(sums + i0 + j);
        const bool zero = F::is_zero(p.z);
        tinf[i0 + j] = zero;
        if (zero) {
            st_words(tab + i0 + j, Aff<C>{F::zero(), F::one()});     // never read
            continue;
        }
        const Fp zi = F::mul(inv, ld_words(zp + i0 + j));
        inv = F::mul(inv, p.z);
        st_words(tab + i0 + j, Aff<C>{F::mul(p.x, zi), F::mul(p.y, zi)});
    }
}

// row i: nbytes bytes at in + i * stride over the ng generators of tab, then (rnd != null) the 96 bytes of the canonical
// integer at rnd + 96 i over the RAND_BITS generators of rtab
template <class C>
__global__ void __launch_bounds__(BLOCK) ped_hash_kernel(const Aff<C>* __restrict__ tab, const uint8_t* __restrict__ tinf, size_t ng, int t,
                                                         const uint8_t* __restrict__ in, size_t stride, size_t nbytes,
                                                         const Aff<C>* __restrict__ rtab, const uint8_t* __restrict__ rtinf,
                                                         const uint8_t* __restrict__ rnd, size_t n, Proj<C>* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t npos = ped_row_positions(nbytes, t);
    const size_t total = npos + (rnd ? ped_positions(RAND_BITS, t) : 0);
    const uint8_t *row = in + i * stride, *rrow = rnd ? rnd + i * 96 : nullptr;
    Proj<C> q = proj_zero<C>();
#pragma unroll 1
    for (size_t s = 0; s < total; s++) {
        const bool second = s >= npos;                      // the same in every lane
        const size_t p = second ? s - npos : s;
        const uint32_t d = second ? ped_digit(rrow, 96, RAND_BITS, t, p) : ped_digit(row, nbytes, ng, t, p);
        if (!d) continue;
        const size_t e = ped_entry(t, p, d);
        if ((second ? rtinf : tinf)[e]) continue;
        q = proj_madd<C>(q, ld_words((second ? rtab : tab) + e));
    }
    st_words(out + i, q);
}

// ---------------------------------------------------------------------------------------------------- host side
size_t table_entries(size_t count, int t) { return ped_positions(count, t) * ped_entries_per_position(t); }

// the table of `count` generators on the device; moved into tab / tinf once it is built
template <class C>
int build_table(const std::vector<uint64_t>& xy, const std::vector<uint8_t>& inf, size_t count, int t, gh_rt::DevMem& tab, gh_rt::DevMem& tinf) {
    const size_t entries = table_entries(count, t);
    gh_rt::DevMem d_gen, d_inf, d_sums, d_zp, d_tab, d_tinf;
    int rc;
    if ((rc = d_gen.alloc(count * 192)) || (rc = d_inf.alloc(count)) || (rc = d_sums.alloc(entries * sizeof(Proj<C>))) ||
        (rc = d_zp.alloc(entries * sizeof(Fp))) || (rc = d_tab.alloc(entries * sizeof(Aff<C>))) || (rc = d_tinf.alloc(entries)))
        return rc;
    HIPCHK(hipMemcpyAsync(d_gen.get(), xy.data(), count * 192, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_inf.get(), inf.data(), count, hipMemcpyHostToDevice, g.stream));
    GH_LAUNCH(ped_table_kernel<C>, dim3(blocks(entries, BLOCK)), dim3(BLOCK), 0, g.stream, d_gen.as<const uint32_t>(), d_inf.as<const uint8_t>(),
              count, t, entries, d_sums.as<Proj<C>>());
    GH_LAUNCH(ped_table_norm_kernel<C>, dim3(blocks(blocks(entries, NORM_RUN), BLOCK)), dim3(BLOCK), 0, g.stream, d_sums.as<const Proj<C>>(),
              entries, d_zp.as<Fp>(), d_tab.as<Aff<C>>(), d_tinf.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.stream));
    tab = std::move(d_tab);
    tinf = std::move(d_tinf);
    return GH_OK;
}

template <class C> int ped_ensure(gh_pedersen* h, bool commit) {
    if (!h->d_tab.get())
        if (int rc = build_table<C>(h->gen_xy, h->gen_inf, h->ng, h->t, h->d_tab, h->d_tinf)) return rc;
    if (commit && !h->d_rtab.get())
        if (int rc = build_table<C>(h->rand_xy, h->rand_inf, RAND_BITS, h->t, h->d_rtab, h->d_rtinf)) return rc;
    return GH_OK;
}

// the hash (rnd null) or the commitment of n rows; dev: input, randomness and outputs are device pointers
template <class C>
int run_rows(gh_pedersen* h, const uint8_t* input, size_t n, size_t nbytes, const uint64_t* rnd, void* out_xy, uint8_t* out_inf, bool dev) {
    typedef typename Scheme<C>::PS PS;
    uint8_t *d_in = nullptr, *d_inf = nullptr;
    uint64_t *d_rnd = nullptr, *d_xy = nullptr;
    uint32_t* d_rint = nullptr;
    Proj<C>* d_p;
    Fp* d_zp;
    int rc = dbuf("vb_p", n, &d_p);
    if (!rc) rc = dbuf("vb_zp", n, &d_zp);
    if (!rc && rnd) rc = dbuf("vb_k", n * 24, &d_rint);
    if (!rc && !dev) rc = dbuf("vb_in", n * nbytes, &d_in);
    if (!rc && !dev && rnd) rc = dbuf("vb_sk", n * 12, &d_rnd);
    if (!rc && !dev) rc = dbuf("vb_xy", n * 24, &d_xy);
    if (!rc && !dev) rc = dbuf("vb_inf", n, &d_inf);
    if (rc || (rc = ped_ensure<C>(h, rnd != nullptr))) return rc;
    PhaseTimer& ph = g_tm.begin();
    if ((rc = ph.mark())) return rc;
    if (dev) {
        d_in = const_cast<uint8_t*>(input);
        d_rnd = const_cast<uint64_t*>(rnd);
        d_xy = (uint64_t*)out_xy;
        d_inf = out_inf;
    } else if ((rc = up(d_in, input, n * nbytes)) || (rnd && (rc = up(d_rnd, rnd, n * 12)))) {
        return rc;
    }
    if ((rc = ph.mark())) return rc;
    if (rnd) GH_LAUNCH((mont_to_int_kernel<PS>), dim3(blocks(n, 256)), dim3(256), 0, g.stream, (const uint32_t*)d_rnd, n, d_rint, (uint8_t*)nullptr);
    GH_LAUNCH((ped_hash_kernel<C>), dim3(blocks(n, BLOCK)), dim3(BLOCK), 0, g.stream, h->d_tab.as<const Aff<C>>(), h->d_tinf.as<const uint8_t>(), h->ng,
              h->t, (const uint8_t*)d_in, nbytes, nbytes, h->d_rtab.as<const Aff<C>>(), h->d_rtinf.as<const uint8_t>(), (const uint8_t*)d_rint, n, d_p);
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    if ((rc = launch_normalize<C>(d_p, nullptr, n, d_zp, d_xy, 48, 0, d_inf))) return rc;
    HIPCHK(hipGetLastError());
    if ((rc = ph.mark())) return rc;
    if (!dev) {
        HIPCHK(hipMemcpyAsync(out_xy, d_xy, n * 192, hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipMemcpyAsync(out_inf, d_inf, n, hipMemcpyDeviceToHost, g.stream));
    }
    if ((rc = ph.mark())) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return ph.finish();
}

int checked(const gh_pedersen* h) {
    if (!h || h->magic != gh_pedersen::MAGIC) { g_err = "not a Pedersen handle"; return GH_E_BAD_HANDLE; }
    return GH_OK;
}

// what the four compute entry points share; rnd_given: a commitment
int compute_api(gh_pedersen* h, const void* input, size_t n, size_t nbytes, bool rnd_given, const void* rnd, void* out_xy, void* out_inf, bool dev) {
    if (int rc = checked(h)) return rc;
    if (rnd_given && h->rand_xy.empty()) { g_err = "randomness: the handle was made without randomness generators (rand_xy)"; return GH_E_BAD_ARG; }
    if (n && ((nbytes && !input) || (rnd_given && !rnd) || !out_xy || !out_inf)) return null_arg();
    size_t b = 0;
    if (mul_overflows(n, nbytes, &b) || mul_overflows(n, 1024, &b) || nbytes > (SIZE_MAX >> 4)) return too_large();
    if (8 * nbytes > h->ng) {
        g_err = "nbytes: the input is longer than the parameters take (8 nbytes > num_windows window_size)";
        return GH_E_BAD_ARG;
    }
    if (rnd_given && !dev && !GH_G1_DISPATCH(h->curve, scalar_below, (const uint64_t*)rnd, n)) {
        g_err = "randomness: a row is not below the modulus of the scalar field";
        return GH_E_BAD_ARG;
    }
    if (n == 0) return GH_OK;
    if (int rc = gh_rt::ensure_init()) return rc;
    return GH_G1_DISPATCH(h->curve, run_rows, h, (const uint8_t*)input, n, nbytes, rnd_given ? (const uint64_t*)rnd : nullptr, out_xy, (uint8_t*)out_inf,
                          dev);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI
using namespace gh_rt;

extern "C" {

int gh_pedersen_create(gh_curve_t curve, const uint64_t* gen_xy, const uint8_t* gen_inf, size_t num_windows, size_t window_size,
                       const uint64_t* rand_xy, const uint8_t* rand_inf, size_t n_rand, int table_bits, gh_pedersen_t* out) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!out) return null_arg();
    *out = nullptr;
    if (curve == GH_MNT4753_G2 || curve == GH_MNT6753_G2) { g_err = "gh_pedersen_create: G1 curves only"; return GH_E_UNSUPPORTED; }
    if (!is_g1(curve)) { g_err = "unknown curve id"; return GH_E_BAD_ARG; }
    if (table_bits != 0 && !ped_table_bits_ok(table_bits)) { g_err = "table_bits must be 0, 1, 2, 4 or 8"; return GH_E_BAD_ARG; }
    size_t ng = 0, b = 0;
    if (!num_windows || !window_size || mul_overflows(num_windows, window_size, &ng) || mul_overflows(ng, (size_t)1 << 15, &b)) {
        g_err = "num_windows and window_size must be positive and their product small enough";
        return GH_E_BAD_ARG;
    }
    if (!gen_xy) return null_arg();
    if (n_rand ? (n_rand != RAND_BITS || !rand_xy) : rand_xy != nullptr) {
        g_err = "n_rand must be 753 with rand_xy (the scalar fields' MODULUS_BITS), or 0 with rand_xy null";
        return GH_E_BAD_ARG;
    }
    if (int rc = check_generators(curve, "gen_xy: ", gen_xy, gen_inf, ng)) return rc;
    if (n_rand)
        if (int rc = check_generators(curve, "rand_xy: ", rand_xy, rand_inf, n_rand)) return rc;
    auto* h = new gh_pedersen();
    h->curve = curve;
    h->num_windows = num_windows;
    h->window_size = window_size;
    h->ng = ng;
    h->t = table_bits ? table_bits : DEFAULT_TABLE_BITS;
    keep(h->gen_xy, h->gen_inf, gen_xy, gen_inf, ng);
    if (n_rand) keep(h->rand_xy, h->rand_inf, rand_xy, rand_inf, n_rand);
    *out = h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_pedersen_free(gh_pedersen_t h) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    if (!h) return GH_OK;
    if (int rc = checked(h)) return rc;
    if (h->d_tab.get()) (void)hipStreamSynchronize(g.stream);
    h->magic = 0;
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_pedersen_hash(gh_pedersen_t h, const uint8_t* input, size_t n, size_t nbytes, uint64_t* out_xy, uint8_t* out_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    return compute_api(h, input, n, nbytes, false, nullptr, out_xy, out_inf, false);
} catch (...) { return gh_rt::api_exception(); }

int gh_pedersen_hash_dev(gh_pedersen_t h, const void* d_input, size_t n, size_t nbytes, void* d_out_xy, void* d_out_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    return compute_api(h, d_input, n, nbytes, false, nullptr, d_out_xy, d_out_inf, true);
} catch (...) { return gh_rt::api_exception(); }

int gh_pedersen_commit(gh_pedersen_t h, const uint8_t* input, size_t n, size_t nbytes, const uint64_t* randomness, uint64_t* out_xy,
                       uint8_t* out_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    return compute_api(h, input, n, nbytes, true, randomness, out_xy, out_inf, false);
} catch (...) { return gh_rt::api_exception(); }

int gh_pedersen_commit_dev(gh_pedersen_t h, const void* d_input, size_t n, size_t nbytes, const void* d_randomness, void* d_out_xy,
                           void* d_out_inf) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    Trim trim_;
    return compute_api(h, d_input, n, nbytes, true, d_randomness, d_out_xy, d_out_inf, true);
} catch (...) { return gh_rt::api_exception(); }

int gh_pedersen_last_timing(float* phase_ms, int max_phases, float* total_ms) try {
    std::lock_guard<std::mutex> lk(api_mutex());
    return g_tm.copy_out(phase_ms, max_phases, total_ms);
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
