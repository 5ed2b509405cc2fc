// poseidon.hip -- the C ABI of include/ginger_hip_poseidon.h: Poseidon permutation / hash kernels over the two scalar
// fields, the level-by-level Merkle tree and batched path verification.  The permutation itself is poseidon_perm.h.
//
// One kernel, poseidon_kernel<P, K, SLAB>, serves every entry point: lane t of T carries the K inputs t, t + T, ...,
// t + (K - 1) T of a batch (so that the lanes of a wave read neighbouring inputs), absorbs them two elements at a time
// and permutes all K states together; a batch larger than K T is walked in steps of K T.  SLAB = false keeps the states
// in registers (RegStore: K = 1 only -- a second state and its prefix products would not fit next to a product's
// working set at 256 VGPRs), SLAB = true in a per-lane global slab (SlabStore, K = 1, 2, 4, 8).  DESIGN.md section 11
// has the measured A/B and the default.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>
#include "unit_host.h"
#include "poseidon_perm.h"
#include "../../include/ginger_hip_poseidon.h"

struct gh_poseidon {
    uint32_t magic = 0x706f7364u;
    gh_field_t field;
    int r_f = 0, r_p = 0;
    std::vector<Fp> host;          // internal form: rc[3 rounds] | mds[9] | c2 | azp[3]
    Fp* dev = nullptr;             // the same on the device (uploaded at the first device call)
    bool have_empty = false;
    uint64_t empty[12];            // evaluate([1]), ABI form
    int rounds() const { return 2 * r_f + r_p; }
    pos::Consts consts(const Fp* base) const {
        const int nrc = 3 * rounds();
        return pos::Consts{base, base + nrc, base + nrc + 9, base + nrc + 10, r_f, r_p};
    }
};

namespace {

constexpr size_t TAIL_DEFAULT = 256;  // host_tail_nodes default: the fastest of a sweep
int g_k = 0;                          // states per lane, 0 = auto
size_t g_tail = TAIL_DEFAULT;
std::vector<float> g_level_ms;
float g_total_ms = 0;
PhaseTimer g_level_tm;                // the bracket around one device level of a tree

constexpr int BLOCK = 64;

// ---------------------------------------------------------------------------------------------------- kernels
// mode 0: hash (out[i] = evaluate(in[i len ..])), mode 1: permute n states of 3 in place (in == out)
template <class P, int K, bool SLAB>
__global__ void __launch_bounds__(BLOCK) poseidon_kernel(pos::Consts c, const uint32_t* in, size_t n, size_t len, uint32_t* out,
                                                          int mode, uint32_t* slab, size_t T) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    using Store = typename std::conditional<SLAB, pos::SlabStore<K>, pos::RegStore<K>>::type;
    Store st;
    if constexpr (SLAB) { st.base = slab + t; st.stride = T; }
    for (size_t base = 0; base < n; base += (size_t)K * T) {
        pos::loop<!SLAB, K>([&](int k) {
            const size_t h = base + (size_t)k * T + t;
            GH_UNROLL for (int e = 0; e < 3; e++) {
                Fp v = c.azp[e];
                if (mode == 1) v = h < n ? fp_from_abi<P>(in + (h * 3 + e) * 24) : fp_zero();
                st.set(k, e, v);
            }
        });
        if (mode == 1) {
            pos::permute<P, K>(st, c);
        } else {
            for (size_t j = 0; j < len; j += 2) {
                pos::loop<!SLAB, K>([&](int k) {
                    const size_t h = base + (size_t)k * T + t;
                    Fp a = fp_zero(), b = fp_zero();
                    if (h < n) {
                        a = fp_from_abi<P>(in + (h * len + j) * 24);
                        if (j + 1 < len) b = fp_from_abi<P>(in + (h * len + j + 1) * 24);
                    }
                    pos::absorb<P>(st, k, a, b, c);
                });
                pos::permute<P, K>(st, c);
            }
        }
        pos::loop<!SLAB, K>([&](int k) {
            const size_t h = base + (size_t)k * T + t;
            if (h >= n) return;
            if (mode == 1) {
                GH_UNROLL for (int e = 0; e < 3; e++) fp_to_abi<P>(out + (h * 3 + e) * 24, st.get(k, e));
            } else {
                fp_to_abi<P>(out + h * 24, st.get(k, 0));
            }
        });
    }
}

// verification step s of n paths: pairs[i] = dir ? (sibling, cur) : (cur, sibling)
__global__ void __launch_bounds__(256) path_pairs_kernel(const uint64_t* cur, const uint64_t* sib, const uint8_t* dir, size_t n,
                                                         uint32_t steps, uint32_t s, uint64_t* pairs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool right = dir[i * steps + s] != 0;
    const uint64_t* a = right ? sib + (i * steps + s) * 12 : cur + i * 12;
    const uint64_t* b = right ? cur + i * 12 : sib + (i * steps + s) * 12;
    for (int w = 0; w < 12; w++) {
        pairs[i * 24 + w] = a[w];
        pairs[i * 24 + 12 + w] = b[w];
    }
}

// ---------------------------------------------------------------------------------------------------- launches
template <class P, int K, bool SLAB> int launch_k(const gh_poseidon* h, const void* d_in, size_t n, size_t len, void* d_out,
                                                  int mode, hipStream_t st) {
    const size_t cap = (size_t)g.num_cus * 512;                      // lanes of one pass over the batch
    const size_t T = std::min((n + K - 1) / K, cap);
    uint32_t* slab = nullptr;
    if (SLAB) {
        if (int rc = gh_rt::pool_get("poseidon_slab", T * pos::SlabStore<K>::kSlots * NL * 4, (void**)&slab)) return rc;
    }
    GH_LAUNCH((poseidon_kernel<P, K, SLAB>), dim3((unsigned)((T + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st,
              h->consts(h->dev), (const uint32_t*)d_in, n, len, (uint32_t*)d_out, mode, slab, T);
    HIPCHK(hipGetLastError());
    return GH_OK;
}

// The slab of K = 8 over a full pass is 48 slots x 104 B x num_cus x 512 lanes (654 MB on 256 CUs).  The pool would keep it
// for the life of the process; every entry point lets go of a slab above 64 MB when it returns (its work is finished then).
struct SlabTrim {
    ~SlabTrim() { gh_rt::pool_trim("poseidon_slab", gh_rt::SLAB_KEEP_BYTES); }
};

bool force_slab() {
    const char* v = getenv("GH_POSEIDON_LAYOUT");   // measurement knob: "slab" runs K = 1 from the slab as well
    return v && !strcmp(v, "slab");
}

// K for a batch of n: the largest whose lanes still fill the card (one wave per SIMD), 1 below that
int choose_k(size_t n) {
    if (g_k > 0) return g_k;
    const size_t full = (size_t)g.num_cus * 4 * 64;
    for (int k : {8, 4, 2})
        if (n >= (size_t)k * full) return k;
    return 1;
}

template <class P> int launch_t(const gh_poseidon* h, const void* d_in, size_t n, size_t len, void* d_out, int mode, hipStream_t st) {
    switch (choose_k(n)) {
        case 1: return force_slab() ? launch_k<P, 1, true>(h, d_in, n, len, d_out, mode, st) : launch_k<P, 1, false>(h, d_in, n, len, d_out, mode, st);
        case 2: return launch_k<P, 2, true>(h, d_in, n, len, d_out, mode, st);
        case 4: return launch_k<P, 4, true>(h, d_in, n, len, d_out, mode, st);
        case 8: return launch_k<P, 8, true>(h, d_in, n, len, d_out, mode, st);
    }
    g_err = "states_per_lane must be 1, 2, 4 or 8";
    return GH_E_BAD_ARG;
}

int launch(const gh_poseidon* h, const void* d_in, size_t n, size_t len, void* d_out, int mode, hipStream_t st = nullptr) {
    if (!st) st = g.stream;
    if (n == 0) return GH_OK;
    return h->field == GH_MNT4753_FR ? launch_t<P6>(h, d_in, n, len, d_out, mode, st) : launch_t<P4>(h, d_in, n, len, d_out, mode, st);
}

// ---------------------------------------------------------------------------------------------------- host side
bool valid(const gh_poseidon* h) { return h && h->magic == 0x706f7364u; }

int host_threads() {
    int n = 16;
    if (const char* v = getenv("OMP_NUM_THREADS")) {
        const int e = atoi(v);
        if (e > 0 && e < n) n = e;
    }
    return n;
}

template <class F> void parallel_for(size_t n, F f) {
    const size_t nt = std::min<size_t>((size_t)host_threads(), n);
    if (nt <= 1) {
        for (size_t i = 0; i < n; i++) f(i);
        return;
    }
    std::vector<std::thread> th;
    for (size_t w = 0; w < nt; w++)
        th.emplace_back([&, w] { for (size_t i = w; i < n; i += nt) f(i); });
    for (auto& x : th) x.join();
}

// evaluate([a, b]) on the host, ABI in and out
template <class P> void host_hash2_t(const gh_poseidon* h, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const pos::Consts c = h->consts(h->host.data());
    pos::RegStore<1> st;
    for (int e = 0; e < 3; e++) st.set(0, e, c.azp[e]);
    pos::absorb<P>(st, 0, fp_from_abi<P>((const uint32_t*)a), fp_from_abi<P>((const uint32_t*)b), c);
    pos::permute<P, 1>(st, c);
    fp_to_abi<P>((uint32_t*)out, st.get(0, 0));
}
void host_hash2(const gh_poseidon* h, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    if (h->field == GH_MNT4753_FR) host_hash2_t<P6>(h, a, b, out);
    else host_hash2_t<P4>(h, a, b, out);
}

// device constants and evaluate([1]), once per handle; API lock held
int prepare(gh_poseidon* h) {
    if (int rc = gh_rt::ensure_init()) return rc;
    if (!h->dev) {
        gh_rt::DevMem dev;          // the handle's only once the constants are in it
        if (int rc = dev.alloc(h->host.size() * sizeof(Fp))) return rc;
        HIPCHK(hipMemcpy(dev.get(), h->host.data(), h->host.size() * sizeof(Fp), hipMemcpyHostToDevice));
        h->dev = (Fp*)dev.release();
    }
    if (!h->have_empty) {
        uint64_t one[12];
        if (h->field == GH_MNT4753_FR) fp_to_abi<P6>((uint32_t*)one, fp_one<P6>());
        else fp_to_abi<P4>((uint32_t*)one, fp_one<P4>());
        void* d = nullptr;
        if (int rc = gh_rt::pool_get("poseidon_one", 2 * 96, &d)) return rc;
        HIPCHK(hipMemcpy(d, one, 96, hipMemcpyHostToDevice));
        if (int rc = launch(h, d, 1, 1, (char*)d + 96, 0)) return rc;
        HIPCHK(hipMemcpy(h->empty, (char*)d + 96, 96, hipMemcpyDeviceToHost));
        h->have_empty = true;
    }
    return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- lock-held helpers (runtime.h)
namespace gh_rt {
int poseidon_field(const gh_poseidon* h, gh_field_t* out) {
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    *out = h->field;
    return GH_OK;
}
int poseidon_hash_dev_locked(gh_poseidon* h, const void* d_in, size_t n, size_t len, void* d_out) {
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    if (n == 0) return GH_OK;
    if (int rc = prepare(h)) return rc;
    return launch(h, d_in, n, len, d_out, 0);
}
void poseidon_trim_slab() { SlabTrim trim_; }
}  // namespace gh_rt

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" {

int gh_poseidon_create(gh_field_t field, uint32_t r_f, uint32_t r_p, const uint64_t* round_cst, size_t n_round_cst,
                       const uint64_t* mds9, const uint64_t* c2, const uint64_t* after_zero_perm3, gh_poseidon_t* out) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    if (!round_cst || !mds9 || !c2 || !after_zero_perm3 || !out) return null_arg();
    *out = nullptr;
    if (field != GH_MNT4753_FR && field != GH_MNT6753_FR) { g_err = "unknown field"; return GH_E_BAD_ARG; }   // its own wording, kept
    if (r_f == 0 || r_f > 1024 || r_p > 1u << 20) { g_err = "r_f must be >= 1 (and the round counts sane)"; return GH_E_BAD_ARG; }
    const size_t nrc = 3 * (2 * (size_t)r_f + r_p);
    if (n_round_cst < nrc) { g_err = "too few round constants"; return GH_E_BAD_ARG; }
    std::vector<const uint64_t*> all;
    for (size_t i = 0; i < nrc; i++) all.push_back(round_cst + 12 * i);
    for (int i = 0; i < 9; i++) all.push_back(mds9 + 12 * i);
    all.push_back(c2);
    for (int i = 0; i < 3; i++) all.push_back(after_zero_perm3 + 12 * i);
    for (const uint64_t* x : all)
        if (!GH_FIELD_DISPATCH(field, below, x)) { g_err = "a Poseidon constant is not below the modulus"; return GH_E_BAD_ARG; }
    auto* h = new gh_poseidon();
    h->field = field;
    h->r_f = (int)r_f;
    h->r_p = (int)r_p;
    for (const uint64_t* x : all) h->host.push_back(GH_FIELD_DISPATCH(field, from_abi12, x));
    *out = h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_free(gh_poseidon_t h) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    if (!h) return GH_OK;
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    gh_rt::dev_free(h->dev);
    h->magic = 0;
    delete h;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_hash_dev(gh_poseidon_t h, const void* d_in, size_t n, size_t len, void* d_out) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    SlabTrim trim_;
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    if (n && (!d_out || (len && !d_in))) return null_arg();
    if (n == 0) return GH_OK;
    if (int rc = prepare(h)) return rc;
    if (int rc = launch(h, d_in, n, len, d_out, 0)) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_hash(gh_poseidon_t h, const uint64_t* in, size_t n, size_t len, uint64_t* out) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    SlabTrim trim_;
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    if (n && (!out || (len && !in))) return null_arg();
    size_t nin = 0, bin = 0;
    if (mul_overflows(n, len, &nin) || mul_overflows(nin, 96, &bin)) return too_large();
    if (n == 0) return GH_OK;
    if (int rc = prepare(h)) return rc;
    void *d_in = nullptr, *d_out = nullptr;
    if (int rc = gh_rt::pool_get("poseidon_in", bin ? bin : 96, &d_in)) return rc;
    if (int rc = gh_rt::pool_get("poseidon_out", n * 96, &d_out)) return rc;
    if (bin) HIPCHK(hipMemcpy(d_in, in, bin, hipMemcpyHostToDevice));
    if (int rc = launch(h, d_in, n, len, d_out, 0)) return rc;
    HIPCHK(hipMemcpy(out, d_out, n * 96, hipMemcpyDeviceToHost));
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_permute(gh_poseidon_t h, uint64_t* states, size_t n) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    SlabTrim trim_;
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    if (n && !states) return null_arg();
    size_t bytes = 0;
    if (mul_overflows(n, 3 * 96, &bytes)) return too_large();
    if (n == 0) return GH_OK;
    if (int rc = prepare(h)) return rc;
    void* d = nullptr;
    if (int rc = gh_rt::pool_get("poseidon_in", bytes, &d)) return rc;
    HIPCHK(hipMemcpy(d, states, bytes, hipMemcpyHostToDevice));
    if (int rc = launch(h, d, n, 0, d, 1)) return rc;
    HIPCHK(hipMemcpy(states, d, bytes, hipMemcpyDeviceToHost));
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_merkle_tree(gh_poseidon_t h, const uint64_t* leaves, size_t n_leaves, uint32_t height, uint64_t* out_tree,
                            uint64_t* out_padding, uint64_t* out_root) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    SlabTrim trim_;
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    if (!out_root || (n_leaves && !leaves)) return null_arg();
    if (n_leaves > ((size_t)1 << 40)) { g_err = "too many leaves"; return GH_E_BAD_ARG; }
    size_t L = 1;
    uint32_t th = 1;                                   // tree_height = log2(L) + 1
    while (L < n_leaves) { L <<= 1; th++; }
    if (th > height) { g_err = "the tree is taller than height"; return GH_E_BAD_ARG; }
    if (int rc = prepare(h)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    g_level_ms.clear();
    const size_t nodes = 2 * L - 1;
    uint64_t* d_tree = nullptr;
    if (int rc = gh_rt::pool_get("poseidon_tree", nodes * 96, (void**)&d_tree)) return rc;
    {   // leaves, padded with evaluate([1]), uploaded once
        std::vector<uint64_t> lv(L * 12);
        if (n_leaves) memcpy(lv.data(), leaves, n_leaves * 96);
        for (size_t i = n_leaves; i < L; i++) memcpy(&lv[i * 12], h->empty, 96);
        HIPCHK(hipMemcpy(d_tree + (L - 1) * 12, lv.data(), L * 96, hipMemcpyHostToDevice));
    }
    // device levels: m nodes at m - 1 from the 2m children at 2m - 1 (contiguous pairs: a hash batch of len 2)
    size_t m = L / 2;
    for (; m >= 1 && m > g_tail; m /= 2) {
        float ms = 0;
        int rc;
        if ((rc = g_level_tm.begin().mark()) || (rc = launch(h, d_tree + (2 * m - 1) * 12, m, 2, d_tree + (m - 1) * 12, 0)) ||
            (rc = g_level_tm.mark()) || (rc = g_level_tm.wait()) || (rc = g_level_tm.bracket(&ms)))
            return rc;
        g_level_ms.push_back(ms);
    }
    // host levels: the top 2 (2m) - 1 nodes, from the device's level of 2m nodes
    std::vector<uint64_t> top;
    if (m >= 1) {
        const size_t ntop = 4 * m - 1;
        top.resize(ntop * 12);
        HIPCHK(hipMemcpy(&top[(2 * m - 1) * 12], d_tree + (2 * m - 1) * 12, 2 * m * 96, hipMemcpyDeviceToHost));
        for (size_t lm = m; lm >= 1; lm /= 2) {
            const auto a = std::chrono::steady_clock::now();
            parallel_for(lm, [&](size_t j) {
                const size_t i = lm - 1 + j;
                host_hash2(h, &top[(2 * i + 1) * 12], &top[(2 * i + 2) * 12], &top[i * 12]);
            });
            g_level_ms.push_back(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - a).count());
        }
    }
    if (out_tree) {
        HIPCHK(hipMemcpy(out_tree, d_tree, nodes * 96, hipMemcpyDeviceToHost));
        if (m >= 1) memcpy(out_tree, top.data(), (2 * m - 1) * 96);
    }
    uint64_t cur[12];
    if (m >= 1) memcpy(cur, top.data(), 96);
    else HIPCHK(hipMemcpy(cur, d_tree, 96, hipMemcpyDeviceToHost));
    // padding chain: cur = evaluate([cur, empty]), height - tree_height times
    const size_t steps = height - th;
    const auto p0 = std::chrono::steady_clock::now();
    if (steps && g_tail > 0) {
        for (size_t s = 0; s < steps; s++) {
            host_hash2(h, cur, h->empty, cur);
            if (out_padding) memcpy(out_padding + s * 12, cur, 96);
        }
    } else if (steps) {
        std::vector<uint64_t> pad((2 * steps + 1) * 12);
        memcpy(pad.data(), cur, 96);
        for (size_t s = 0; s < steps; s++) memcpy(&pad[(2 * s + 1) * 12], h->empty, 96);
        uint64_t* d_pad = nullptr;
        if (int rc = gh_rt::pool_get("poseidon_pad", pad.size() * 8, (void**)&d_pad)) return rc;
        HIPCHK(hipMemcpy(d_pad, pad.data(), pad.size() * 8, hipMemcpyHostToDevice));
        for (size_t s = 0; s < steps; s++)
            if (int rc = launch(h, d_pad + 2 * s * 12, 1, 2, d_pad + (2 * s + 2) * 12, 0)) return rc;
        HIPCHK(hipMemcpy(pad.data(), d_pad, pad.size() * 8, hipMemcpyDeviceToHost));
        for (size_t s = 0; s < steps; s++)
            if (out_padding) memcpy(out_padding + s * 12, &pad[(2 * s + 2) * 12], 96);
        memcpy(cur, &pad[2 * steps * 12], 96);
    }
    g_level_ms.push_back(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - p0).count());
    memcpy(out_root, cur, 96);
    g_total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_merkle_verify(gh_poseidon_t h, const uint64_t* leaves, const uint64_t* siblings, const uint8_t* directions,
                              size_t n, uint32_t height, const uint64_t* root, uint8_t* out_ok) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    SlabTrim trim_;
    if (!valid(h)) { g_err = "not a Poseidon handle"; return GH_E_BAD_HANDLE; }
    if (n && (!leaves || !siblings || !directions || !root || !out_ok)) return null_arg();
    if (height < 2) { g_err = "a path needs height >= 2 (the reference rejects an empty path)"; return GH_E_BAD_ARG; }
    const uint32_t steps = height - 1;
    size_t nsib = 0, bsib = 0, bpairs = 0;
    if (mul_overflows(n, steps, &nsib) || mul_overflows(nsib, 96, &bsib) || mul_overflows(n, 192, &bpairs))
        return too_large();
    if (n == 0) return GH_OK;
    if (int rc = prepare(h)) return rc;
    uint64_t *d_cur = nullptr, *d_sib = nullptr, *d_pairs = nullptr;
    uint8_t* d_dir = nullptr;
    if (int rc = gh_rt::pool_get("poseidon_out", n * 96, (void**)&d_cur)) return rc;
    if (int rc = gh_rt::pool_get("poseidon_in", bpairs, (void**)&d_pairs)) return rc;
    if (int rc = gh_rt::pool_get("poseidon_sib", bsib, (void**)&d_sib)) return rc;
    if (int rc = gh_rt::pool_get("poseidon_dir", nsib, (void**)&d_dir)) return rc;
    HIPCHK(hipMemcpy(d_cur, leaves, n * 96, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sib, siblings, bsib, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_dir, directions, nsib, hipMemcpyHostToDevice));
    for (uint32_t s = 0; s < steps; s++) {
        GH_LAUNCH(path_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g.stream, d_cur, d_sib, d_dir, n, steps, s, d_pairs);
        if (int rc = launch(h, d_pairs, n, 2, d_cur, 0)) return rc;
    }
    std::vector<uint64_t> cur(n * 12);
    HIPCHK(hipMemcpy(cur.data(), d_cur, n * 96, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) out_ok[i] = memcmp(&cur[i * 12], root, 96) == 0;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_set_tuning(int states_per_lane, size_t host_tail_nodes) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    if (states_per_lane != 0 && states_per_lane != 1 && states_per_lane != 2 && states_per_lane != 4 && states_per_lane != 8) {
        g_err = "states_per_lane must be 0, 1, 2, 4 or 8";
        return GH_E_BAD_ARG;
    }
    g_k = states_per_lane;
    g_tail = host_tail_nodes == SIZE_MAX ? TAIL_DEFAULT : host_tail_nodes;
    return GH_OK;
} catch (...) { return gh_rt::api_exception(); }

int gh_poseidon_last_timing(float* level_ms, int max_levels, float* total_ms) try {
    std::lock_guard<std::mutex> lk(gh_rt::api_mutex());
    if ((!level_ms && max_levels > 0) || max_levels < 0) return null_arg();
    const int cnt = std::min<int>(max_levels, (int)g_level_ms.size());
    for (int i = 0; i < cnt; i++) level_ms[i] = g_level_ms[i];
    if (total_ms) *total_ms = g_total_ms;
    return cnt;
} catch (...) { return gh_rt::api_exception(); }

}  // extern "C"
