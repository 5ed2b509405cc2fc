// poseidon_perm.h -- the Poseidon permutation (T = 3, rate 2, S-box x -> x^-1 with 0 -> 0) over the 753-bit scalar
// fields, for K states at once: the same code runs in a gfx950 lane (poseidon.hip) and on the host (the host tail of a
// tree, tests/host_shim/poseidon_shim.cpp).
//
// The function (primitives/src/crh/poseidon/mod.rs:379-523, parameters in tests/golden/poseidon_params.json):
// R_F full rounds, R_P partial rounds, R_F full rounds; round r adds round_cst[3r .. 3r + 2], applies the S-box to all
// three elements (full) or to element 0 (partial), and -- except after the very last round -- replaces the state by
// M state with M the row-major MDS matrix of full-size field elements.
//
// Batching: a round inverts the S-box inputs of all K states with ONE Montgomery trick (3K inputs in a full round, K in
// a partial one): prefix products forward, one safegcd fp_inv, the inverses backward.  Zero inputs are skipped exactly
// as batch_inverse_kernel (ntt_kernels.h) skips them -- they do not enter the product and stay 0 -- so the result is the
// mathematical function for every input.  (The reference's batched form, mod.rs:245-251, leaves the LAST state of a
// batch un-inverted when a partial round's product is zero; that is not reproduced.)
// Cost per state and round: 3 products per S-box input, 3 three-term products (fp_mul3 = 2 products each) for the mix,
// plus one inversion (~40 products) per K states.
//
// Where the states live is the store S:
//   RegStore<K>  -- a register array: every loop is unrolled (compile-time indices), nothing touches memory.
//   SlabStore<K> -- a per-lane slab in global memory, limb-major with the lane index fastest (a wave's 64 lanes read
//                   256 consecutive bytes per limb); the loops over the K states stay rolled, so the code size does not
//                   grow with K and only a handful of elements are live in registers.
// Constants are read through plain pointers with indices that do not depend on the lane (uniform loads).
#pragma once
#include <stddef.h>
#include "fp29.h"

#if defined(__HIPCC__)
#define GH_NOUNROLL _Pragma("unroll 1")
#else
#define GH_NOUNROLL
#endif

namespace gh {
namespace pos {

// Internal-form (Montgomery 2^754) constants of one parameter set, as laid out by gh_poseidon_create:
//   rc[3 (2 r_f + r_p)] | mds[9] | c2 | azp[3]
struct Consts {
    const Fp* rc;
    const Fp* mds;
    const Fp* c2;
    const Fp* azp;
    int r_f, r_p;
};

template <int K> struct RegStore {
    static constexpr bool kRegs = true;
    Fp s[K][3];
    Fp w[3 * K];     // prefix products of the Montgomery trick; w[0..2] are the rows of the mix
    GH_HD Fp get(int k, int e) const { return s[k][e]; }
    GH_HD void set(int k, int e, const Fp& v) { s[k][e] = v; }
    GH_HD Fp getw(int i) const { return w[i]; }
    GH_HD void setw(int i, const Fp& v) { w[i] = v; }
};

// 6K slots of one element per lane: states (slot 3k + e), then prefix products / mix rows (slot 3K + i).
template <int K> struct SlabStore {
    static constexpr bool kRegs = false;
    static constexpr int kSlots = 6 * K;
    uint32_t* base;    // slab + lane
    size_t stride;     // lanes of the slab
    GH_HD Fp ld(int slot) const {
        Fp r;
        const uint32_t* q = base + (size_t)slot * NL * stride;
        GH_UNROLL for (int i = 0; i < NL; i++) r.l[i] = q[(size_t)i * stride];
        return r;
    }
    GH_HD void st(int slot, const Fp& v) const {
        uint32_t* q = base + (size_t)slot * NL * stride;
        GH_UNROLL for (int i = 0; i < NL; i++) q[(size_t)i * stride] = v.l[i];
    }
    GH_HD Fp get(int k, int e) const { return ld(3 * k + e); }
    GH_HD void set(int k, int e, const Fp& v) const { st(3 * k + e, v); }
    GH_HD Fp getw(int i) const { return ld(3 * K + i); }
    GH_HD void setw(int i, const Fp& v) const { st(3 * K + i, v); }
};

template <bool UNROLL, int N, class F> GH_HD void loop(F&& f) {
    if constexpr (UNROLL) {
        GH_UNROLL for (int i = 0; i < N; i++) f(i);
    } else {
        GH_NOUNROLL for (int i = 0; i < N; i++) f(i);
    }
}

// The same constant pointer, opaque to the optimizer once per round: otherwise it hoists the 9 MDS entries (234 words) out
// of the round loop into registers, and the kernel spills.
GH_HD const Fp* per_round(const Fp* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__ volatile("" : "+s"(p));
#endif
    return p;
}

GH_HD Fp sel(bool c, const Fp& a, const Fp& b) {
    Fp r;
    GH_UNROLL for (int i = 0; i < NL; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}

// Montgomery trick, forward half: acc <- product of the non-zero S-box inputs (1 if none), w[i] <- the product up to
// and including input i.  Input i is element i % NS of state i / NS (NS = 3: full round, NS = 1: partial round).
template <class P, int K, int NS, class S> GH_HD Fp sbox_forward(S& st) {
    constexpr int N = K * NS;
    Fp acc = fp_one<P>();
    loop<S::kRegs, N>([&](int i) {
        const Fp x = st.get(i / NS, i % NS);
        const Fp m = fp_mul<P>(acc, x);
        acc = sel(fp_is_zero(x), acc, m);
        if (i < N - 1) st.setw(i, acc);
    });
    return acc;
}
// backward half: inv = (product of the non-zero inputs)^-1; input i <- inv * w[i - 1], then inv <- inv * input i
template <class P, int K, int NS, class S> GH_HD void sbox_backward(S& st, Fp inv) {
    constexpr int N = K * NS;
    loop<S::kRegs, N>([&](int j) {
        const int i = N - 1 - j;
        const Fp x = st.get(i / NS, i % NS);
        const bool z = fp_is_zero(x);
        Fp y = inv;
        if (i > 0) {
            y = fp_mul<P>(inv, st.getw(i - 1));
            inv = sel(z, inv, fp_mul<P>(inv, x));
        }
        st.set(i / NS, i % NS, sel(z, x, y));
    });
}

template <class P, int K, class S> GH_HD void sbox(S& st, bool full) {
    const Fp acc = full ? sbox_forward<P, K, 3>(st) : sbox_forward<P, K, 1>(st);
    const Fp inv = fp_inv<P>(acc);            // one inversion per lane and round
    if (full) sbox_backward<P, K, 3>(st, inv);
    else sbox_backward<P, K, 1>(st, inv);
}

// state <- M state: one fp_mul3 (three products, one reduction) per row
template <class P, int K, class S> GH_HD void mix(S& st, const Fp* mds) {
    loop<S::kRegs, K>([&](int k) {
        const Fp a = st.get(k, 0), b = st.get(k, 1), c = st.get(k, 2);
        loop<S::kRegs, 3>([&](int i) { st.setw(i, fp_mul3<P>(mds[3 * i], a, mds[3 * i + 1], b, mds[3 * i + 2], c)); });
        loop<S::kRegs, 3>([&](int i) { st.set(k, i, st.getw(i)); });
    });
}

template <class P, int K, class S> GH_HD void add_rc(S& st, const Fp* rc) {
    loop<S::kRegs, K>([&](int k) {
        loop<S::kRegs, 3>([&](int e) { st.set(k, e, fp_add<P>(st.get(k, e), rc[e])); });
    });
}

template <class P, int K, class S> GH_HD void permute(S& st, const Consts& c) {
    const int rounds = 2 * c.r_f + c.r_p;
    GH_NOUNROLL for (int r = 0; r < rounds; r++) {
        add_rc<P, K>(st, per_round(c.rc + 3 * r));
        sbox<P, K>(st, r < c.r_f || r >= c.r_f + c.r_p);
        if (r != rounds - 1) mix<P, K>(st, per_round(c.mds));
    }
}

// evaluate() absorption step (mod.rs:594-611): state += (a, b, C2); b is zero for an odd leftover
template <class P, class S> GH_HD void absorb(S& st, int k, const Fp& a, const Fp& b, const Consts& c) {
    st.set(k, 0, fp_add<P>(st.get(k, 0), a));
    st.set(k, 1, fp_add<P>(st.get(k, 1), b));
    st.set(k, 2, fp_add<P>(st.get(k, 2), *c.c2));
}

}  // namespace pos
}  // namespace gh
