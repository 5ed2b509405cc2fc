// msm_kernels.h -- variable-base multi-scalar multiplication (Pippenger bucket method) on gfx950.
//
// Reference algorithm: algebra/src/msm/variable_base.rs:10-83 -- per c-bit window a *serial* loop
// over all pairs doing buckets[digit-1].add_assign_mixed(base) (:36-59), batch-normalise, running
// sum (:60-66), then a Horner fold of the windows (:73-82); parallelism = number of windows.
// The group sum is order-independent (only the affine image of the result is canonical),
// so the device uses its own schedule:
//
//   1. msm_digits_kernel     one thread per scalar: signed c-bit digits d in [-2^(c-1), 2^(c-1)]
//                            (halves the bucket count), histogram of |d| per (window, bucket).
//   2. exclusive scan of the histogram (msm_scan_*), bucket order by descending size
//      (msm_size_*: counting sort on the bucket size so the 64 lanes of a wave get equal work).
//   3. msm_scatter_kernel    counting-sort scatter: for every bucket the list of (pair index | sign).
//   4. msm_accumulate_xyzz_kernel  one thread per bucket walks its list: gather the base (internal
//                            layout, 208 B for G1), conditional negate, mixed add into XYZZ accumulators
//                            (madd-2008-s, 8 M + 2 S; its assembly build on G1 by default).  G2: one bucket per
//                            lane pair / triple (msm_accumulate_split_kernel) or the affine rounds (aff_kernels.h).
//                            ~94 % of all work (as in the reference).
//      chunk mode + msm_heavy_combine_kernel: buckets longer than the heavy threshold are cut into
//                            chunks that the same kernel sums like ordinary buckets, then combined
//                            (skewed real-world witnesses -- many equal small scalars -- and
//                            sparsely populated top windows).
//   5. msm_wave_reduce_kernel  sum_b b * B_b per window without the reference's per-window inversion
//                            and without doublings: "wave programs" whose every step is one
//                            projective addition from a single inlined call site (serial sums per
//                            lane, then tree / suffix scan / tree across the 64 lanes through LDS:
//                            the wavefront-wide bucket reduction); two launches.  In msm_reduce_kernels.h.
//   6. window fold           ~750 dependent doublings: latency-bound, done on the host
//                            (msm_fold.h fold_windows) with the reduction's powers of two merged in.
#pragma once
#include <hip/hip_runtime.h>
#include "ec29.h"
#include "aff_kernels.h"
#include "msm_plan.h"
#include "msm_schedule.h"

namespace gh {

// MSM_REDUCE_L, MSM_MAX_HEAVY_THRESHOLD, MSM_SIZE_BINS, MSM_PART_MAX_BINS, MSM_DUP_CHUNK: msm_plan.h (shared with the host's plans)

// ---------------------------------------------------------------- generic point load / store
template <class C> __device__ __forceinline__ Aff<C> ld_aff(const Aff<C>* p) {
    Aff<C> r;
    const uint2* q = reinterpret_cast<const uint2*>(p);
    uint2* d = reinterpret_cast<uint2*>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(Aff<C>) / 8); i++) d[i] = q[i];
    return r;
}
template <class C> __device__ __forceinline__ Proj<C> ld_proj(const Proj<C>* p) {
    Proj<C> r;
    const uint2* q = reinterpret_cast<const uint2*>(p);
    uint2* d = reinterpret_cast<uint2*>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(Proj<C>) / 8); i++) d[i] = q[i];
    return r;
}
template <class C> __device__ __forceinline__ void st_proj(Proj<C>* p, const Proj<C>& v) {
    uint2* q = reinterpret_cast<uint2*>(p);
    const uint2* s = reinterpret_cast<const uint2*>(&v);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(Proj<C>) / 8); i++) q[i] = s[i];
}

#ifndef GH_LD_ST_FP
#define GH_LD_ST_FP
__device__ __forceinline__ Fp ld_fp(const Fp* p) {
    Fp r;
    const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int i = 0; i < NL / 2; i++) { uint2 v = q[i]; r.l[2 * i] = v.x; r.l[2 * i + 1] = v.y; }
    return r;
}
__device__ __forceinline__ void st_fp(Fp* p, const Fp& a) {
    uint2* q = reinterpret_cast<uint2*>(p);
#pragma unroll
    for (int i = 0; i < NL / 2; i++) q[i] = make_uint2(a.l[2 * i], a.l[2 * i + 1]);
}
#endif
// Lane groups (4b, and the lane-group reduction of msm_reduce_kernels.h): a lane holds coefficient `comp` of a field element of LANES coefficients.
// Coordinate e of an Aff / Proj in memory is {c0, .., c_(LANES-1)}, so this lane's part is Fp number LANES e + comp of the point.
template <int LANES> __device__ __forceinline__ Fp ld_coeff(const void* pt, int e, int comp) {
    return ld_fp(reinterpret_cast<const Fp*>(pt) + LANES * e + comp);
}
template <int LANES> __device__ __forceinline__ void st_coeff(void* pt, int e, int comp, const Fp& v) {
    st_fp(reinterpret_cast<Fp*>(pt) + LANES * e + comp, v);
}

// ---------------------------------------------------------------- bases: ABI -> internal layout
// in: n x (2 * DEG * 24) words, x || y, either Montgomery 2^768 (the in-memory form, fp_768.rs:24-30) or --
// canonical != 0 -- plain integers < p (what ToBytes writes: into_repr(), fp_768.rs:784-789);
// out: n x Aff<C> (internal 2^754): one product by 2^740 resp. 2^1508 per coefficient.
template <class C>
__global__ void __launch_bounds__(256) msm_convert_bases_kernel(const uint32_t* in, Aff<C>* out, size_t n, int canonical) {
    typedef typename C::F F;
    typedef typename C::PF PF;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + i * (size_t)(48 * F::DEG);
    const Fp k = canonical ? fp_const<PF>(PF::R2I) : fp_const<PF>(PF::CIN);
    Aff<C> a;
#pragma unroll
    for (int d = 0; d < F::DEG; d++) {
        F::comp(a.x, d) = fp_mul<PF>(fp_unpack(p + 24 * d), k);
        F::comp(a.y, d) = fp_mul<PF>(fp_unpack(p + 24 * (F::DEG + d)), k);
    }
    uint2* q = reinterpret_cast<uint2*>(out + i);
    const uint2* s = reinterpret_cast<const uint2*>(&a);
#pragma unroll
    for (int w = 0; w < (int)(sizeof(Aff<C>) / 8); w++) q[w] = s[w];
}

// ---------------------------------------------------------------- 0. precomputed shift tables
// Bases are static per proving key (groth16/mod.rs:158-170), and 288 GB of HBM hold a lot of them:
// for a resident key the library can store, next to P_i, the points 2^(c w) P_i for every window w
// (table row w; W rows of n affine points).  Window w of scalar i then adds table[w][i] instead of
// P_i, all windows share ONE set of 2^(c-1) buckets, and the per-window reduction and the Horner
// fold over windows (variable_base.rs:60-82) collapse into a single bucket reduction.  With the
// bucket count decoupled from the window count, c can grow (c = 21 at n = 2^20: 36 additions per
// pair instead of 48).
//
// One thread per base: c doublings per row (out-of-line dbl-2007-bl), projective rows parked in the
// table / a scratch array, then ONE field inversion per base (Montgomery's trick over its W - 1 Z
// coordinates, as batch_normalization does: short_weierstrass_projective.rs:402-442) turns them
// into affine rows.
template <class P> __device__ __attribute__((noinline)) Fp dev_fp_inv(const Fp& a) {   // a^(p-2)
    uint32_t e[NL];
    int32_t bw = -2;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int32_t x = (int32_t)P::P[i] + bw;
        e[i] = (uint32_t)x & LM;
        bw = x >> 31;
    }
    Fp r = fp_one<P>();
#pragma unroll
    for (int i = NL - 1; i >= 0; i--) {
        const uint32_t ei = e[i];
#pragma nounroll
        for (int b = LB - 1; b >= 0; b--) {
            r = fp_sqr_call<P>(r);
            if ((ei >> b) & 1u) r = fp_mul_call<P>(r, a);
        }
    }
    return r;
}
template <class F> struct DevInv;
template <class P, bool I> struct DevInv<F1<P, I>> {
    static __device__ __forceinline__ Fp inv(const Fp& a) { return dev_fp_inv<P>(a); }
};
template <class P, int NR, bool I> struct DevInv<F2<P, NR, I>> {   // (a0 - a1 X) / (a0^2 - NR a1^2)   (fp2.rs inverse)
    static __device__ __forceinline__ Fp2T inv(const Fp2T& a) {
        Fp n = fp_sub<P>(fp_sqr_call<P>(a.c0), fp_mul_small<P, NR>(fp_sqr_call<P>(a.c1)));
        Fp ni = dev_fp_inv<P>(n);
        return Fp2T{fp_mul_call<P>(a.c0, ni), fp_neg<P>(fp_mul_call<P>(a.c1, ni))};
    }
};
template <class P, int NR, bool I> struct DevInv<F3<P, NR, I>> {   // norm-based inverse (fp3.rs inverse)
    static __device__ __forceinline__ Fp3T inv(const Fp3T& a) {
        Fp t0 = fp_sqr_call<P>(a.c0), t1 = fp_sqr_call<P>(a.c1), t2 = fp_sqr_call<P>(a.c2);
        Fp t3 = fp_mul_call<P>(a.c0, a.c1), t4 = fp_mul_call<P>(a.c0, a.c2), t5 = fp_mul_call<P>(a.c1, a.c2);
        Fp c0 = fp_sub<P>(t0, fp_mul_small<P, NR>(t5));
        Fp c1 = fp_sub<P>(fp_mul_small<P, NR>(t2), t3);
        Fp c2 = fp_sub<P>(t1, t4);
        Fp n = fp_add<P>(fp_mul_call<P>(a.c0, c0),
                         fp_mul_small<P, NR>(fp_add<P>(fp_mul_call<P>(a.c2, c1), fp_mul_call<P>(a.c1, c2))));
        Fp ni = dev_fp_inv<P>(n);
        return Fp3T{fp_mul_call<P>(c0, ni), fp_mul_call<P>(c1, ni), fp_mul_call<P>(c2, ni)};
    }
};

template <class T> __device__ __forceinline__ T ld_words(const T* p) {
    T r;
    const uint2* q = reinterpret_cast<const uint2*>(p);
    uint2* d = reinterpret_cast<uint2*>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 8); i++) d[i] = q[i];
    return r;
}
template <class T> __device__ __forceinline__ void st_words(T* p, const T& v) {
    uint2* q = reinterpret_cast<uint2*>(p);
    const uint2* s = reinterpret_cast<const uint2*>(&v);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 8); i++) q[i] = s[i];
}

// table: W rows of n points (row 0 = the bases themselves, already written by the caller);
// this launch covers bases [i0, i0 + cnt).  zs / zp: (W - 1) x slab field elements of scratch
// (Z_w and the running products Z_1 .. Z_w).  bad[0] is set when a doubling chain reaches infinity
// (a base of 2-power order: the caller then keeps the plain per-window path for this key).
// The doublings run in JACOBIAN coordinates (round 3): dbl-2007-bl is 1 M + 8 S + a ZZ^2 against the 5 M + 6 S of the
// homogeneous doubling; for the prime-field curves (G1) the products are inlined as well, where the homogeneous round-1/2 kernel
// called them out of line -- 2^20 G1 bases, c = 21: 0.85 -> 0.40 s.  Row w holds (X, Y) of 2^(c w) P until the backward
// sweep turns them into x = X / Z^2, y = Y / Z^3 with ONE inversion per base over the row Z's (Montgomery's trick).
template <class C, class F>
__global__ void __launch_bounds__(F::DEG == 1 ? 256 : 64)
msm_precompute_jac_kernel(Aff<C>* __restrict__ table, const uint8_t* __restrict__ infinity, size_t n, size_t i0, size_t cnt,
                          size_t slab, int c, int W, typename F::T* __restrict__ zs, typename F::T* __restrict__ zp,
                          uint32_t* __restrict__ bad) {
    typedef typename F::T T;          // F: the inlined prime field for G1, the out-of-line towers for G2 (same formulas)
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt) return;
    const size_t i = i0 + t;
    const Aff<C> b = ld_words(table + i);
    if (infinity != nullptr && infinity[i] != 0) {
        for (int w = 1; w < W; w++) st_words(table + (size_t)w * n + i, b);
        return;
    }
    T X = b.x, Y = b.y, Z = F::one(), run = F::one();
    for (int w = 1; w < W; w++) {
#pragma nounroll
        for (int d = 0; d < c; d++) {
            const T xx = F::sqr(X), yy = F::sqr(Y), zz = F::sqr(Z);
            const T yyyy = F::sqr(yy);
            const T s = F::dbl(F::sub(F::sub(F::sqr(F::add(X, yy)), xx), yyyy));
            const T m = F::add(F::add(F::dbl(xx), xx), C::mul_by_a(F::sqr(zz)));
            const T z3 = F::sub(F::sub(F::sqr(F::add(Y, Z)), yy), zz);
            X = F::sub(F::sqr(m), F::dbl(s));
            Y = F::sub(F::mul(m, F::sub(s, X)), F::dbl(F::dbl(F::dbl(yyyy))));
            Z = z3;
        }
        if (F::is_zero(Z)) { atomicOr(bad, 1u); return; }
        st_words(table + (size_t)w * n + i, Aff<C>{X, Y});
        st_words(zs + (size_t)(w - 1) * slab + t, Z);
        run = F::mul(run, Z);
        st_words(zp + (size_t)(w - 1) * slab + t, run);
    }
    T inv = DevInv<F>::inv(run);   // 1 / (Z_1 ... Z_(W-1))
    for (int w = W - 1; w >= 1; w--) {
        T zi = inv;
        if (w > 1) zi = F::mul(inv, ld_words(zp + (size_t)(w - 2) * slab + t));   // 1 / Z_w
        inv = F::mul(inv, ld_words(zs + (size_t)(w - 1) * slab + t));
        Aff<C> q = ld_words(table + (size_t)w * n + i);
        const T zi2 = F::sqr(zi);
        q.x = F::mul(q.x, zi2);
        q.y = F::mul(q.y, F::mul(zi2, zi));
        st_words(table + (size_t)w * n + i, q);
    }
}

// Wave-aggregated counter increment: returns the old value of base[key] as if every active lane
// had done atomicAdd(base + key, 1).  Up to `iters` distinct keys are combined into one atomic
// each (leader election by ballot); the rest fall back to per-lane atomics.  Random digits pay a
// few ballots; skewed digits (the top window holds only 0/1/2, witnesses are full of 0/1) no
// longer serialise a million atomics on one address.  Must be called by all 64 lanes of the wave.
static __device__ __forceinline__ uint32_t wave_agg_inc(uint32_t* base, uint32_t key, bool active, int iters) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    uint32_t result = 0;
    bool done = !active;
    for (int it = 0; it < iters && todo; it++) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lkey = __shfl(key, leader);
        const bool mine = !done && key == lkey;
        const unsigned long long same = __ballot(mine);
        uint32_t b = 0;
        if (lane == leader) b = atomicAdd(base + lkey, (uint32_t)__popcll(same));
        b = __shfl(b, leader);
        if (mine) { result = b + (uint32_t)__popcll(same & ((1ull << lane) - 1ull)); done = true; }
        todo &= ~same;
    }
    if (!done) result = atomicAdd(base + key, 1u);
    return result;
}

// ---------------------------------------------------------------- 1. digits + histogram
// scalars: n x 24 words canonical (< r).  digits[w * n + i] = signed digit (0 = no contribution).
// counts[(w % sets) * win_stride + |d| - slot_shift] += 1; sets = num_windows, win_stride = nb = 2^(c-1) + 1 (slot 0 unused,
// slot_shift 0) gives every window its own bucket set; sets = 1 files all windows into ONE bucket set (precomputed
// shift tables, section 0 above: window w then reads its bases from table row w), a partial table's sets = G files window w
// into set w % G and reads row w / G.  A merged set has win_stride = nb = 2^(c-1) and uses slot_shift 1:
// slot = |d| - 1, exactly 2^(c-1) slots -- a power of two, so the bucket reduction's segments tile it without a
// remainder (one straggling wave program on an already occupied SIMD doubled the whole launch); the weight of a slot
// is then slot + 1 and the fold adds the plain sum of all buckets once (msm_fold.h fold_merged).
//
// (a) sign folding: s > r/2 is replaced by r - s with the base negated (s P = (r - s)(-P)), so the
//     magnitude is below 2^752 and bit 752 never needs a window.
// (b) signed recoding of the c-bit windows: v = bits(s, wc, c) + carry; if v > 2^(c-1):
//     d = v - 2^c, carry = 1  (reference digit rule, unsigned: variable_base.rs:43-50).
// (c) the top window.  num_windows = floor(752 / c) + 1.  If c does not divide 752 the last window
//     holds the 752 mod c leftover bits plus the carry and never carries out.  If c divides 752
//     (c = 16: 47 * 16) the last window would hold nothing but the carry -- one bucket with n/2
//     entries.  Instead (top_unsigned) window W-2, the top real one, is taken UNSIGNED:
//     v <= 0.885 * 2^c + 1 is filed under slot v of window W-2 if v <= 2^(c-1), else under slot
//     v - 2^(c-1) of window W-1, which thereby is "region b" of window W-2 (same window weight,
//     slot offset 2^(c-1): the host adds 2^(c-1) * sum(region b), msm_fold.h fold_windows).
struct MsmModulus { uint32_t w[24]; };

// ---- equal bases.  A proving key holds the SAME point for every variable with the same polynomial (the `Benchmark` circuit's
// closing constraint puts L_last(t) into B for every recorded variable: half of b_query is one point), and
// sum s_i P = (sum s_i) P: the scalars of equal (or opposite) bases are added up front and the MSM runs on the distinct bases only
// (nothing in the reference does this; VariableBaseMSM::multi_scalar_mul's result is the same group element).  Without it every
// pair of equal bases that meet in a bucket is a doubling / a cancellation (swp.rs:492) -- millions per MSM on such a key.
// msm_base_hash_kernel: 128 bits over the abscissa's limbs per base (0, 0 for infinity); the host groups equal hashes
// (msm_key.h dedup_bases); msm_dup_verify_kernel compares every member with its group's first base limb for limb (a hash
// collision drops out of the group) and records the sign; msm_merge_scalars_kernel does the sums at MSM time.
template <class C>
static __global__ void __launch_bounds__(256)
msm_base_hash_kernel(const Aff<C>* __restrict__ pts, const uint8_t* __restrict__ inf, size_t n, uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t h1 = 0x9E3779B97F4A7C15ull, h2 = 0xC2B2AE3D27D4EB4Full;
    if (inf && inf[i]) { out[2 * i] = 0; out[2 * i + 1] = 0; return; }
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&pts[i].x);
    constexpr int NW = (int)(sizeof(pts[0].x) / 4);
    for (int k = 0; k < NW; k++) {
        const uint64_t x = w[k];
        h1 = ((h1 ^ x) * 0xFF51AFD7ED558CCDull); h1 ^= h1 >> 29;
        h2 = (h2 + x) * 0x94D049BB133111EBull; h2 = (h2 << 27) | (h2 >> 37);
    }
    if (h1 == 0 && h2 == 0) h1 = 1;
    out[2 * i] = h1; out[2 * i + 1] = h2;
}

// members[j]: base index (bit 31 clear); group g = members[starts[g] .. starts[g + 1]), its first entry the canonical base.
// Sets bit 31 where the member is the NEGATIVE of the canonical base; flags[j] = 1 where it is neither (not the same point).
template <class C>
static __global__ void __launch_bounds__(256)
msm_dup_verify_kernel(const Aff<C>* __restrict__ pts, const uint32_t* __restrict__ starts, uint32_t n_groups, uint32_t* __restrict__ members,
                      uint8_t* __restrict__ flags) {
    const uint32_t g = blockIdx.x;
    if (g >= n_groups) return;
    const uint32_t lo = starts[g], hi = starts[g + 1];
    const uint32_t canon = members[lo] & 0x7FFFFFFFu;
    constexpr int NW = (int)(sizeof(pts[0].x) / 4);
    const uint32_t* cx = reinterpret_cast<const uint32_t*>(&pts[canon].x);
    const uint32_t* cy = reinterpret_cast<const uint32_t*>(&pts[canon].y);
    for (uint32_t j = lo + 1 + threadIdx.x; j < hi; j += blockDim.x) {
        const uint32_t m = members[j] & 0x7FFFFFFFu;
        const uint32_t* mx = reinterpret_cast<const uint32_t*>(&pts[m].x);
        const uint32_t* my = reinterpret_cast<const uint32_t*>(&pts[m].y);
        bool same_x = true, same_y = true;
        for (int k = 0; k < NW; k++) { same_x &= mx[k] == cx[k]; same_y &= my[k] == cy[k]; }
        // equal x on the curve: y equal or opposite (y = 0 would be both: a point of order two never enters a key)
        flags[j] = same_x ? 0 : 1;
        members[j] = m | ((same_x && !same_y) ? 0x80000000u : 0u);
    }
}

// out = in with, per group, the canonical base's scalar replaced by the signed sum of the group's scalars mod r and the other
// members' scalars zeroed.  One block per group; scalars are canonical integers below r (12 x u64 as 24 words).
static __device__ __forceinline__ void scalar_add_mod(uint32_t* a, const uint32_t* b, const MsmModulus& r) {
    uint32_t cy = 0;
    uint32_t t[24];
#pragma unroll
    for (int k = 0; k < 24; k++) { const uint64_t x = (uint64_t)a[k] + b[k] + cy; a[k] = (uint32_t)x; cy = (uint32_t)(x >> 32); }
    uint32_t bw = 0;
#pragma unroll
    for (int k = 0; k < 24; k++) { const uint64_t x = (uint64_t)a[k] - r.w[k] - bw; t[k] = (uint32_t)x; bw = (uint32_t)(x >> 32) & 1u; }
    if (cy || !bw) {
#pragma unroll
        for (int k = 0; k < 24; k++) a[k] = t[k];
    }
}
// Two steps, so that one huge group (half a proving key's b_query can be ONE point) is not one block's work: the groups are cut
// into chunks of at most MSM_DUP_CHUNK members (chunks[3 k] = first member, [3 k + 1] = end, [3 k + 2] = group); step 1 sums a
// chunk's scalars into partial[k] and zeroes its non-canonical members in `out`, step 2 adds a group's partial sums into its
// canonical base's scalar.
static __global__ void __launch_bounds__(256)
msm_merge_scalars_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n, const uint32_t* __restrict__ starts,
                         const uint32_t* __restrict__ members, const uint32_t* __restrict__ chunks, uint32_t n_chunks,
                         uint32_t* __restrict__ partial, MsmModulus r) {
    __shared__ uint32_t part[256][25];
    const uint32_t ck = blockIdx.x;
    if (ck >= n_chunks) return;
    const uint32_t lo = chunks[3 * ck], hi = chunks[3 * ck + 1], first = starts[chunks[3 * ck + 2]];
    uint32_t acc[24];
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] = 0;
    for (uint32_t j = lo + threadIdx.x; j < hi; j += blockDim.x) {
        const uint32_t e = members[j], m = e & 0x7FFFFFFFu;
        if (m >= n) continue;                                      // the call uses fewer scalars than the key has bases
        uint32_t s[24];
        const uint4* q = reinterpret_cast<const uint4*>(in + (size_t)m * 24);
#pragma unroll
        for (int k = 0; k < 6; k++) { const uint4 v = q[k]; s[4 * k] = v.x; s[4 * k + 1] = v.y; s[4 * k + 2] = v.z; s[4 * k + 3] = v.w; }
        if (e >> 31) {                                             // - s = r - s (0 stays 0)
            uint32_t any = 0, bw = 0;
#pragma unroll
            for (int k = 0; k < 24; k++) any |= s[k];
            if (any) {
#pragma unroll
                for (int k = 0; k < 24; k++) { const uint64_t x = (uint64_t)r.w[k] - s[k] - bw; s[k] = (uint32_t)x; bw = (uint32_t)(x >> 32) & 1u; }
            }
        }
        scalar_add_mod(acc, s, r);
        if (j != first) {
            uint4* o = reinterpret_cast<uint4*>(out + (size_t)m * 24);
#pragma unroll
            for (int k = 0; k < 6; k++) o[k] = make_uint4(0, 0, 0, 0);
        }
    }
#pragma unroll
    for (int k = 0; k < 24; k++) part[threadIdx.x][k] = acc[k];
    __syncthreads();
    for (uint32_t step = 128; step > 0; step >>= 1) {
        if (threadIdx.x < step) {
            uint32_t a[24], b[24];
#pragma unroll
            for (int k = 0; k < 24; k++) { a[k] = part[threadIdx.x][k]; b[k] = part[threadIdx.x + step][k]; }
            scalar_add_mod(a, b, r);
#pragma unroll
            for (int k = 0; k < 24; k++) part[threadIdx.x][k] = a[k];
        }
        __syncthreads();
    }
    if (threadIdx.x < 24) partial[(size_t)ck * 24 + threadIdx.x] = part[0][threadIdx.x];
}
// gchunk[g] .. gchunk[g + 1]: the chunks of group g (consecutive)
static __global__ void __launch_bounds__(64)
msm_merge_groups_kernel(uint32_t* __restrict__ out, size_t n, const uint32_t* __restrict__ starts, const uint32_t* __restrict__ members,
                        const uint32_t* __restrict__ gchunk, uint32_t n_groups, const uint32_t* __restrict__ partial, MsmModulus r) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t canon = members[starts[g]] & 0x7FFFFFFFu;
    if (canon >= n) return;                                        // members ascend: none of the group is in this call
    uint32_t acc[24];
#pragma unroll
    for (int k = 0; k < 24; k++) acc[k] = 0;
    for (uint32_t ck = gchunk[g]; ck < gchunk[g + 1]; ck++) {
        uint32_t s[24];
#pragma unroll
        for (int k = 0; k < 24; k++) s[k] = partial[(size_t)ck * 24 + k];
        scalar_add_mod(acc, s, r);
    }
#pragma unroll
    for (int k = 0; k < 24; k++) out[(size_t)canon * 24 + k] = acc[k];
}

static __global__ void __launch_bounds__(256)
msm_digits_kernel(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ infinity, size_t n, int c,
                  int num_windows, uint32_t win_stride, int top_unsigned, MsmModulus r,
                  int32_t* __restrict__ digits, uint32_t* __restrict__ counts, int agg_iters, uint32_t slot_shift,
                  uint32_t sets /* bucket sets: window w files into set w % sets (per-window path: sets = num_windows) */) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    uint32_t s[25];
#pragma unroll
    for (int k = 0; k < 25; k++) s[k] = 0;
    if (valid) {
        const uint4* q = reinterpret_cast<const uint4*>(scalars + i * 24);
#pragma unroll
        for (int k = 0; k < 6; k++) { uint4 v = q[k]; s[4 * k] = v.x; s[4 * k + 1] = v.y; s[4 * k + 2] = v.z; s[4 * k + 3] = v.w; }
    }
    // (a) t = r - s;  negate if t < s
    uint32_t t[24];
    uint32_t bw = 0;
    bool lt = false;   // t < s, decided by the most significant differing word
#pragma unroll
    for (int k = 0; k < 24; k++) {
        uint64_t x = (uint64_t)r.w[k] - s[k] - bw;
        t[k] = (uint32_t)x;
        bw = (uint32_t)(x >> 32) & 1u;
        if (t[k] != s[k]) lt = t[k] < s[k];
    }
    const bool sneg = lt && bw == 0;   // bw != 0 would mean s > r (non-canonical input): leave as is
    if (sneg) {
#pragma unroll
        for (int k = 0; k < 24; k++) s[k] = t[k];
    }
    const bool skip = !valid || (infinity != nullptr && infinity[i] != 0);
    const uint32_t half = 1u << (c - 1), full_mask = (1u << c) - 1;
    uint32_t carry = 0;
    int32_t d_next = 0;   // region-b digit of the top_unsigned scheme, emitted for window W-1
    for (int w = 0; w < num_windows; w++) {
        const int bit = w * c;
        uint32_t v = 0;
        if (bit < 768) {
            const int wi = bit >> 5, sh = bit & 31;
            uint64_t two = (uint64_t)s[wi] | ((uint64_t)s[wi + 1] << 32);
            v = (uint32_t)(two >> sh) & full_mask;
        }
        v += carry;
        int32_t d;
        if (top_unsigned && w == num_windows - 2) {
            if (v > half) { d = 0; d_next = (int32_t)(v - half); } else { d = (int32_t)v; }
            carry = 0;
        } else if (top_unsigned && w == num_windows - 1) {
            d = d_next;
        } else if (v > half) { d = (int32_t)v - (int32_t)(1u << c); carry = 1; } else { d = (int32_t)v; carry = 0; }
        if (sneg) d = -d;
        if (skip) d = 0;
        if (valid) digits[(size_t)w * n + i] = d;
        const uint32_t mag = d < 0 ? (uint32_t)(-d) : (uint32_t)d;
        if (counts) wave_agg_inc(counts + (size_t)((uint32_t)w % sets) * win_stride, mag - slot_shift, d != 0, agg_iters);   // (uniform branch)
    }
}

// ---------------------------------------------------------------- 2a. bucket lists without global atomics (large inputs)
// The histogram + scatter pair above issues two device-scope atomics per list entry on a counter array that is
// far larger than LDS (2 x 37.7 M at 2^20 pairs: 3.4 ms, 12 ms at 2^22).  For large inputs the lists are built by a
// two-level counting sort whose atomics all stay in LDS:
//   A  the bucket range is cut into NB <= 1024 (2048 beyond 2^23 buckets) bins of 2^bin_shift buckets; every block takes a tile of consecutive
//      entries e = w n + i, counts them per bin in LDS (msm_part_hist_kernel -> block_hist[bin][block]), an exclusive
//      scan over that array gives every (bin, block) its slice of the partitioned array, and the same tile is read
//      again to write (bucket, list value) pairs there (msm_part_scatter_kernel);
//   B  one block per bin: per-bucket counts in LDS, block scan -> counts[] / starts[], second sweep -> sorted[].
// Result: the same counts / starts / sorted arrays as the atomic path (order inside a bucket is arbitrary in both).
constexpr int MSM_PART_THREADS = 256;
struct MsmPartArgs {
    const int32_t* digits;
    size_t entries;        // W * n
    size_t n;
    uint32_t win_stride, row_stride, slot_shift;
    uint32_t sets;         // window w: bucket set w % sets, table row w / sets (per-window path: sets = W; full table: 1)
    uint32_t bin_shift, n_bins, tile, n_blocks;
};
// entry e -> (bucket, value); returns false for a zero digit
static __device__ __forceinline__ bool msm_part_entry(const MsmPartArgs& a, size_t e, uint32_t w, size_t w_base, uint32_t& bucket, uint32_t& value) {
    const int32_t d = a.digits[e];
    if (d == 0) return false;
    const uint32_t mag = d < 0 ? (uint32_t)(-d) : (uint32_t)d;
    const uint32_t i = (uint32_t)(e - w_base);
    bucket = (w % a.sets) * a.win_stride + (mag - a.slot_shift);
    value = (i + (w / a.sets) * a.row_stride) | (d < 0 ? 0x80000000u : 0u);
    return true;
}
static __global__ void __launch_bounds__(MSM_PART_THREADS) msm_part_hist_kernel(MsmPartArgs a, uint32_t* __restrict__ block_hist) {
    __shared__ uint32_t h[MSM_PART_MAX_BINS];
    for (uint32_t i = threadIdx.x; i < a.n_bins; i += MSM_PART_THREADS) h[i] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * a.tile;
    const uint32_t w0 = (uint32_t)(base / a.n);               // a tile (<= n entries) spans at most two windows
    const size_t split = (size_t)(w0 + 1) * a.n;
    for (uint32_t j = threadIdx.x; j < a.tile; j += MSM_PART_THREADS) {
        const size_t e = base + j;
        if (e >= a.entries) break;
        const uint32_t w = e >= split ? w0 + 1 : w0;
        uint32_t b, v;
        if (msm_part_entry(a, e, w, (size_t)w * a.n, b, v)) atomicAdd(&h[b >> a.bin_shift], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.n_bins; i += MSM_PART_THREADS) block_hist[(size_t)i * a.n_blocks + blockIdx.x] = h[i];
}
static __global__ void __launch_bounds__(MSM_PART_THREADS) msm_part_scatter_kernel(MsmPartArgs a, const uint32_t* __restrict__ block_off,
                                                                                  uint2* __restrict__ part) {
    __shared__ uint32_t cur[MSM_PART_MAX_BINS];
    for (uint32_t i = threadIdx.x; i < a.n_bins; i += MSM_PART_THREADS) cur[i] = block_off[(size_t)i * a.n_blocks + blockIdx.x];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * a.tile;
    const uint32_t w0 = (uint32_t)(base / a.n);
    const size_t split = (size_t)(w0 + 1) * a.n;
    for (uint32_t j = threadIdx.x; j < a.tile; j += MSM_PART_THREADS) {
        const size_t e = base + j;
        if (e >= a.entries) break;
        const uint32_t w = e >= split ? w0 + 1 : w0;
        uint32_t b, v;
        if (msm_part_entry(a, e, w, (size_t)w * a.n, b, v)) {
            const uint32_t pos = atomicAdd(&cur[b >> a.bin_shift], 1u);
            part[pos] = make_uint2(b, v);
        }
    }
}
// one block per bin; dynamic LDS: 2^bin_shift counters.  block_off[bin * n_blocks] is where the bin's pairs start
// (block_off has n_bins * n_blocks + 1 elements: the last one is the total).
constexpr int MSM_BIN_THREADS = 1024;
constexpr int MSM_BIN_UNROLL = 8;
static __global__ void __launch_bounds__(MSM_BIN_THREADS) msm_bin_sort_kernel(const uint2* __restrict__ part, const uint32_t* __restrict__ block_off,
                                                                             uint32_t n_blocks, uint32_t bin_shift, uint32_t total,
                                                                             uint32_t* __restrict__ counts, uint32_t* __restrict__ starts,
                                                                             uint32_t* __restrict__ sorted) {
    extern __shared__ uint32_t cnt[];                 // 2^bin_shift
    __shared__ uint32_t wsum[MSM_BIN_THREADS / 64];
    const uint32_t bin = blockIdx.x, size = 1u << bin_shift, b0 = bin << bin_shift;
    const uint32_t lo = block_off[(size_t)bin * n_blocks], hi = block_off[(size_t)(bin + 1) * n_blocks];
    for (uint32_t i = threadIdx.x; i < size; i += MSM_BIN_THREADS) cnt[i] = 0;
    __syncthreads();
    // both sweeps read MSM_BIN_UNROLL pairs per thread before the first LDS atomic: a bin of 2^19 pairs (2^24 pairs per window) is
    // 512 dependent load -> atomic -> store rounds per thread otherwise (44 ms for the 1280 bins there; round 3)
    for (uint32_t k = lo + threadIdx.x; k < hi; k += MSM_BIN_THREADS * MSM_BIN_UNROLL) {
        uint32_t bx[MSM_BIN_UNROLL];
#pragma unroll
        for (int u = 0; u < MSM_BIN_UNROLL; u++) {
            const uint32_t kk = k + (uint32_t)u * MSM_BIN_THREADS;
            bx[u] = kk < hi ? part[kk].x : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < MSM_BIN_UNROLL; u++) if (bx[u] != 0xFFFFFFFFu) atomicAdd(&cnt[bx[u] - b0], 1u);
    }
    __syncthreads();
    // exclusive scan of cnt: each thread owns `per` consecutive counters
    const uint32_t per = size / MSM_BIN_THREADS > 0 ? size / MSM_BIN_THREADS : 1;
    const uint32_t first = threadIdx.x * per;
    uint32_t mine = 0;
    if (first < size) for (uint32_t k = 0; k < per; k++) mine += cnt[first + k];
    uint32_t incl = mine;                              // wave-inclusive scan, then across the 16 waves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if (lane >= off) incl += t; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int k = 0; k < wave; k++) wbase += wsum[k];
    uint32_t run = lo + wbase + incl - mine;
    if (first < size) {
        for (uint32_t k = 0; k < per; k++) {
            const uint32_t c = cnt[first + k], b = b0 + first + k;
            if (b < total) { counts[b] = c; starts[b] = run; }
            cnt[first + k] = run;                     // becomes the bucket's cursor
            run += c;
        }
    }
    __syncthreads();
    // Second sweep, in the order of the partitioned array: a bin's pairs arrive tile by tile, i.e. by ascending entry number
    // e = w n + i, and 1024 consecutive pairs of a bin are about one window's worth -- so with a barrier after every 1024 pairs
    // each bucket's list comes out ordered by window (merged buckets) / by base index (per-window buckets).  The accumulation
    // walks its lists in step, so ordered lists keep the gathers of the waves in flight closer together: 1-2 % on the
    // accumulation and on the pipelined batch at 2^20 .. 2^24, and the sweep itself is no slower with the barriers
    // (profiles/r03_sort_order_ab.txt).  The loads of eight steps are issued together.
    for (uint32_t base = lo; base < hi; base += MSM_BIN_THREADS * MSM_BIN_UNROLL) {      // uniform trip count: barriers inside
        uint2 pv[MSM_BIN_UNROLL];
#pragma unroll
        for (int u = 0; u < MSM_BIN_UNROLL; u++) {
            const uint32_t kk = base + (uint32_t)u * MSM_BIN_THREADS + threadIdx.x;
            pv[u] = kk < hi ? part[kk] : make_uint2(0xFFFFFFFFu, 0u);
        }
#pragma unroll
        for (int u = 0; u < MSM_BIN_UNROLL; u++) {
            if (pv[u].x != 0xFFFFFFFFu) sorted[atomicAdd(&cnt[pv[u].x - b0], 1u)] = pv[u].y;
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- 2b. bucket order by descending size
// size bin = min(count, heavy_thr + 1); bins are laid out so that larger sizes come first, i.e.
// order[0 .. n_heavy) are the heavy buckets (count > heavy_thr).  Bucket sizes cluster around the
// mean, so the bins are aggregated in LDS per block before touching the global counters.
static __device__ __forceinline__ uint32_t msm_size_bin(uint32_t cnt, uint32_t heavy_thr) {
    uint32_t bin = cnt > heavy_thr ? heavy_thr + 1 : cnt;
    return heavy_thr + 1 - bin;  // reversed: heavy -> 0, then sizes heavy_thr .. 0
}
static __global__ void __launch_bounds__(256)
msm_size_hist_kernel(const uint32_t* counts, size_t total, uint32_t heavy_thr, uint32_t* size_hist, uint32_t* max_count) {
    __shared__ uint32_t h[MSM_SIZE_BINS];
    __shared__ uint32_t bmax;
    for (int i = threadIdx.x; i < MSM_SIZE_BINS; i += 256) h[i] = 0;
    if (threadIdx.x == 0) bmax = 0;
    __syncthreads();
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) {
        const uint32_t c = counts[g];
        atomicAdd(&h[msm_size_bin(c, heavy_thr)], 1u);
        atomicMax(&bmax, c);      // the largest bucket (the affine rounds size their depth by it)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MSM_SIZE_BINS; i += 256) if (h[i]) atomicAdd(&size_hist[i], h[i]);
    if (threadIdx.x == 0 && bmax) atomicMax(max_count, bmax);
}
static __global__ void __launch_bounds__(256)
msm_size_scatter_kernel(const uint32_t* counts, size_t total, uint32_t heavy_thr, uint32_t* size_cursor, uint32_t* order) {
    __shared__ uint32_t h[MSM_SIZE_BINS];
    for (int i = threadIdx.x; i < MSM_SIZE_BINS; i += 256) h[i] = 0;
    __syncthreads();
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bin = 0, rank = 0;
    if (g < total) { bin = msm_size_bin(counts[g], heavy_thr); rank = atomicAdd(&h[bin], 1u); }
    __syncthreads();
    for (int i = threadIdx.x; i < MSM_SIZE_BINS; i += 256) { uint32_t c = h[i]; if (c) h[i] = atomicAdd(&size_cursor[i], c); }
    __syncthreads();
    if (g < total) order[h[bin] + rank] = (uint32_t)g;
}

// plan[0] = n_heavy, plan[1] = total number of chunks, plan[2] = list entries; chunk_start[h] for h in [0, n_heavy]
static __global__ void msm_heavy_plan_kernel(const uint32_t* size_hist, const uint32_t* counts, const uint32_t* order,
                                             const uint32_t* starts, uint32_t total, uint32_t chunk, uint32_t* chunk_start,
                                             uint32_t* plan) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t n_heavy = size_hist[0];
    uint32_t run = 0;
    for (uint32_t h = 0; h < n_heavy; h++) {
        chunk_start[h] = run;
        run += (counts[order[h]] + chunk - 1) / chunk;
    }
    chunk_start[n_heavy] = run;
    plan[0] = n_heavy;
    plan[1] = run;
    plan[2] = starts[total - 1] + counts[total - 1];   // list entries = additions the accumulation will issue
    plan[3] = 0;
}

// ---------------------------------------------------------------- 3. scatter
static __global__ void __launch_bounds__(256)
msm_scatter_kernel(const int32_t* __restrict__ digits, size_t n, int num_windows, uint32_t win_stride,
                   uint32_t row_stride /* 0, or the table's row length (merged windows) */,
                   uint32_t* __restrict__ cursor /* = copy of starts */, uint32_t* __restrict__ sorted, int agg_iters,
                   uint32_t slot_shift, uint32_t sets) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int w = blockIdx.y;
    const int32_t d = i < n ? digits[(size_t)w * n + i] : 0;
    const uint32_t mag = d < 0 ? (uint32_t)(-d) : (uint32_t)d;
    const uint32_t pos = wave_agg_inc(cursor + (size_t)((uint32_t)w % sets) * win_stride, mag - slot_shift, d != 0, agg_iters);
    if (d != 0) sorted[pos] = ((uint32_t)i + ((uint32_t)w / sets) * row_stride) | (d < 0 ? 0x80000000u : 0u);
}

// ---------------------------------------------------------------- 4. bucket accumulation
// order[] lists bucket ids by descending size: [0, n_heavy) are heavy (msm_heavy_*_kernel), whose lists are cut into
// chunks; the task list is [0, n_chunks) chunks of the heavy buckets (the longest tasks, scheduled first), then the buckets
// order[n_heavy ..], one task per thread (G1) or lane group (G2, 4b); empty buckets store infinity.  Every kernel of this
// section gets its task's (beg, cnt, destination) from ONE decode, msm_schedule.h acc_task_decode.
//
// The reference's `P == Q -> double` branch (swp.rs:492-495) is reached when a bucket's running sum equals the incoming
// base (duplicate bases); instead of a doubling formula the thread then takes a three-step detour through a fixed "salt"
// point S (S = G or 2G, whichever has x != q.x, so q != +-S):  acc <- ((q + S) + q) - S = 2q, each step a generic mixed
// addition.  P + (-P) needs no branch: the formula yields Z = 0 and the next addition restarts from infinity.
//
// AFFIN = true: the input is the output list of the affine rounds (aff_kernels.h): bucket g_first + t owns the records
// [starts[g] - list_base, + counts[g]) of `bases` directly (no index list, no signs) and infinity markers are skipped.

// ---------------------------------------------------------------- 4-asm. task table of the assembly accumulation kernel
// The task decode of section 4 (acc_task_decode: chunks of the heavy buckets first, then every other
// bucket by descending size) as a table, so that the assembly kernel (asmgen/g1_xyzz.py) starts from (beg, cnt, dst).
struct AccTaskRec {
    uint32_t beg, cnt;
    uint64_t dst;
};
template <class C>
__global__ void __launch_bounds__(256)
msm_acc_tasks_kernel(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ order,
                     uint32_t total, Proj<C>* __restrict__ buckets, const uint32_t* __restrict__ chunk_start, uint32_t n_heavy,
                     uint32_t n_chunks, uint32_t chunk, Proj<C>* __restrict__ partials, AccTaskRec* __restrict__ out,
                     uint32_t* __restrict__ tile_counter) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    // the persistent accumulation draws its tiles from this word (asmgen/g1_xyzz.py): it starts every launch at 0.  This kernel
    // is the accumulation's predecessor on its stream, so the reset costs no memset node and no launch of its own.
    if (t == 0) __hip_atomic_store(tile_counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t >= n_chunks + (total - n_heavy)) return;
    const auto k = acc_task_decode<false>(t, starts, counts, order, buckets, chunk_start, n_heavy, n_chunks, chunk, partials, 0, 0);
    AccTaskRec r;
    r.beg = k.beg; r.cnt = k.cnt;
    r.dst = (uint64_t)(uintptr_t)k.dst;
    out[t] = r;
}

// ---------------------------------------------------------------- 4a. G1 bucket accumulation on XYZZ accumulators
// The task list, list walk and salt detour of section 4, with the running sum in extended Jacobian coordinates (ec29.h, Xyzz):
// madd-2008-s, 8 M + 2 S, and Y3 as one dual product on a single accumulator chain (fp_mul2s) -- 12 194 v_mad_u64_u32 per bucket update where madd-1998-cmo issues 14 226.
// Register plan (256 VGPRs, two waves per SIMD): ZZ and ZZZ stay in registers; X and Y of the running sum live in LDS
// (word-major, 2 x 26 KiB per block) and are read where the formula needs them (X: P and Q; Y: R and Y3), so the loop
// never holds more than six field elements next to a product's own m / r arrays.
// Output: the projective image (X ZZZ : Y ZZ : ZZ ZZZ) the bucket reduction expects.
template <class C, bool AFFIN = false>
__global__ void __launch_bounds__(256, 2)
msm_accumulate_xyzz_kernel(const Aff<C>* __restrict__ bases, const uint32_t* __restrict__ sorted,
                           const uint32_t* __restrict__ starts, const uint32_t* __restrict__ counts,
                           const uint32_t* __restrict__ order, uint32_t total,
                           const Aff<C>* __restrict__ salts, Proj<C>* __restrict__ buckets,
                           const uint32_t* __restrict__ chunk_start, uint32_t n_heavy, uint32_t n_chunks, uint32_t chunk,
                           Proj<C>* __restrict__ partials, uint32_t g_first = 0, uint32_t list_base = 0) {
    typedef typename C::PF P;
    static_assert(C::F::DEG == 1, "XYZZ accumulation kernel: prime-field curves");
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_chunks + (total - n_heavy)) return;
    const auto tk = acc_task_decode<AFFIN>(t, starts, counts, order, buckets, chunk_start, n_heavy, n_chunks, chunk, partials, g_first, list_base);
    const uint32_t beg = tk.beg, cnt = tk.cnt;
    Proj<C>* dst = tk.dst;
    __shared__ uint32_t park[2][NL][256];     // [0]: X, [1]: Y of this thread's running sum
    auto put = [&](int s, const Fp& v) {
#pragma unroll
        for (int w = 0; w < NL; w++) park[s][w][threadIdx.x] = v.l[w];
    };
    auto get = [&](int s) {
        Fp v;
#pragma unroll
        for (int w = 0; w < NL; w++) v.l[w] = park[s][w][threadIdx.x];
        return v;
    };
#define GH_FENCE() __builtin_amdgcn_sched_barrier(0)
    Fp zz = fp_zero(), zzz = fp_zero();
    // The parked ordinate is V = sigma Y, sigma = -1 while `sneg`: the dual product below then needs no negated operand --
    // with W = sigma R = (sigma q.y) ZZZ - V:  W (X3 - Q) + V PPP = -sigma Y3, so sigma flips with every update and is absorbed
    // by the sign the incoming point gets anyway (one 26-limb negation less per update).
    bool sneg = false;
    uint32_t k = 0;
    int phase = 0, salt_id = 0;     // phase 0: list entry k; 1: +S; 2: entry k again; 3: -S
    uint32_t guard = 0;
    while (k < cnt && guard < 4 * cnt + 8) {
        guard++;
        Fp qx, qy;
        if (phase == 1 || phase == 3) {
            const Aff<C> s = ld_aff<C>(salts + salt_id);
            qx = s.x; qy = ((phase == 3) != sneg) ? fp_neg<P>(s.y) : s.y;
        } else {
            if constexpr (AFFIN) {
                const uint32_t e = beg + k;
                qx = t64_ld_x(bases, e >> 6, e & 63u);
                qy = t64_ld_y(bases, e >> 6, e & 63u);
                if (phase == 0 && qx.l[0] == AFF_MARK) { k++; continue; }   // a cancelled pair: nothing to add
                if (sneg) qy = fp_neg<P>(qy);
            } else {
                const uint32_t e = sorted[beg + k];
                const Aff<C> b = ld_aff<C>(bases + (e & 0x7FFFFFFFu));
                qx = b.x; qy = (((e >> 31) != 0) != sneg) ? fp_neg<P>(b.y) : b.y;
            }
        }
        if (fp_is_zero(zz)) {
            put(0, qx); put(1, qy);
            zz = fp_one<P>(); zzz = zz;
        } else {
            Fp pp = fp_mul<P>(qx, zz);                              // U2
            GH_FENCE();
            Fp r = fp_mul<P>(qy, zzz);                              // S2
            GH_FENCE();
            pp = fp_sub<P>(pp, get(0));                             // P = U2 - X1
            r = fp_sub<P>(r, get(1));                               // W = sigma (S2 - Y1) = sigma R
            if (phase == 0 && fp_is_zero(pp) && fp_is_zero(r)) {    // acc == q: the detour (swp.rs:492-495 doubles here)
                salt_id = fp_eq(qx, ld_aff<C>(salts).x) ? 1 : 0;
                phase = 1;
                continue;
            }
            GH_FENCE();
            Fp p2 = fp_sqr<P>(pp);                                  // PP
            GH_FENCE();
            zz = fp_mul<P>(zz, p2);                                 // ZZ3
            GH_FENCE();
            pp = fp_mul<P>(pp, p2);                                 // PPP
            GH_FENCE();
            zzz = fp_mul<P>(zzz, pp);                               // ZZZ3
            GH_FENCE();
            p2 = fp_mul<P>(get(0), p2);                             // Q = X1 PP
            GH_FENCE();
            Fp x3 = fp_sub<P>(fp_sub<P>(fp_sqr<P>(r), pp), fp_dbl<P>(p2));
            put(0, x3);
            GH_FENCE();
            p2 = fp_sub<P>(x3, p2);                                 // X3 - Q
            GH_FENCE();
            put(1, fp_mul2s<P>(r, p2, get(1), pp));                 // W (X3 - Q) + V PPP = -sigma Y3: the new V, sigma flips
            sneg = !sneg;
            GH_FENCE();
        }
        if (phase == 0 || phase == 3) { k++; phase = 0; } else phase++;
    }
#undef GH_FENCE
    Proj<C> out = proj_zero<C>();
    if (!fp_is_zero(zz)) {
        out.x = fp_mul<P>(get(0), zzz);
        out.y = fp_mul<P>(sneg ? fp_neg<P>(get(1)) : get(1), zz);
        out.z = fp_mul<P>(zz, zzz);
    }
    st_proj<C>(dst, out);
}

// ---------------------------------------------------------------- 4b. G2 over Fq2: lane-pair formulation
// An Fq2 element (c0, c1) lives in TWO adjacent lanes: c0 in the even lane, c1 in the odd one, so a
// G2 point costs each lane the registers of a G1 point and the kernel needs neither out-of-line
// products nor scratch (the call-based Fq2 kernel moved ~16 KB of scratch per mixed addition
// and was bandwidth bound).  Products use the schoolbook split, two Fp products per lane:
//   even lane: c0 = a0 b0 + NR a1 b1        odd lane: c1 = a1 b0 + a0 b1
// with the partner's coefficients fetched by DPP quad permutes (26 moves per operand: swap, broadcast of either half).
// 22 Fp-product times per mixed addition and lane pair, against 31 on one lane -- but in registers.
// Each lane issues one dual product with a single reduction (2028 mads, 4 operands + 2 accumulators live: 512 registers,
// 1 wave / SIMD).  Two plain products per lane at 2 waves / SIMD (2704 mads, 256 registers) spilled 0.8-1.8 KB and were
// slower: accumulation 166 against 119 ms, affine rounds 91 against 68 ms (2^20 pairs).
template <class P, int NR> struct F2S {
    typedef Fp T;
    static constexpr int DEG = 1;   // per-lane footprint
    static constexpr int LANES = 2;
    static constexpr int WAVES = 1;   // measured (twice): accumulation 119 ms at 1 wave / SIMD vs 135 ms at 2 (1.5 KB of spills), 2^20 pairs
    static __device__ __forceinline__ bool odd() { return (threadIdx.x & 1u) != 0; }
    static __device__ __forceinline__ T swap(const T& a) {
        T r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.l[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)a.l[i], 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
        return r;                                                     // (__shfl_xor(x, 1) compiles to ds_bpermute_b32: LDS round trips)
    }
    static __device__ __forceinline__ T sel(bool c, const T& x, const T& y) {   // c ? x : y
        T r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.l[i] = c ? x.l[i] : y.l[i];
        return r;
    }
    static __device__ __forceinline__ T zero() { return fp_zero(); }
    static __device__ __forceinline__ T one() { return odd() ? fp_zero() : fp_one<P>(); }
    static __device__ __forceinline__ T add(const T& a, const T& b) { return fp_add<P>(a, b); }
    static __device__ __forceinline__ T sub(const T& a, const T& b) { return fp_sub<P>(a, b); }
    static __device__ __forceinline__ T dbl(const T& a) { return fp_dbl<P>(a); }
    static __device__ __forceinline__ T neg(const T& a) { return fp_neg<P>(a); }
    // coefficient PART (0 / 1) of b in both lanes of the pair: one DPP move per limb (quad_perm [0,0,2,2] / [1,1,3,3])
    template <int PART> static __device__ __forceinline__ T bcast(const T& b) {
        T r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.l[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)b.l[i], PART ? 0xF5 : 0xA0, 0xF, 0xF, true);
        return r;
    }
    static __device__ __forceinline__ T mul(const T& a, const T& b) {
        const bool o = odd();
        // per lane:  even: a0 b0 + (NR a1) b1      odd: a1 b0 + a0 b1
        // = own a times b0, the partner's a (times NR on the even lane: fp_mul_small_rt with k = NR / 1) times b1
        const T ao = fp_mul_small_rt<P>(swap(a), o ? 1u : (uint32_t)NR), b0 = bcast<0>(b), b1 = bcast<1>(b);
        return fp_mul2<P>(a, b0, ao, b1);
    }
    static __device__ __forceinline__ T mul_sub_mul(const T& a, const T& b, const T& c, const T& d) { return sub(mul(a, b), mul(c, d)); }
    static __device__ __forceinline__ T sqr(const T& a) { return mul(a, a); }
    // (the dual product takes fully reduced operands only: (3 p^2 + R p) / R > 2p with a lazy one)
    static __device__ __forceinline__ T sub_lazy(const T& a, const T& b) { return fp_sub<P>(a, b); }
    // (a0 + a1 X)^-1 = (a0 - a1 X) / (a0^2 - NR a1^2)     (fp2.rs inverse): one Fp inversion per lane pair, run by both lanes
    static __device__ __forceinline__ T inv(const T& a) {
        const bool o = odd();
        const T s = fp_sqr<P>(a), t = swap(s);                       // own square, the partner's
        const T n = o ? fp_sub<P>(t, fp_mul_small<P, NR>(s)) : fp_sub<P>(s, fp_mul_small<P, NR>(t));
        const T r = fp_mul<P>(a, fp_inv<P>(n));
        return o ? fp_neg<P>(r) : r;
    }
    static __device__ __forceinline__ bool is_zero(const T& a) {
        const int z = fp_is_zero(a) ? 1 : 0;
        return (z & __shfl_xor(z, 1)) != 0;
    }
    static __device__ __forceinline__ bool eq(const T& a, const T& b) {
        const int z = fp_eq(a, b) ? 1 : 0;
        return (z & __shfl_xor(z, 1)) != 0;
    }
};

// Fq3 = Fp[X]/(X^3 - NR) over lane triples (lanes 3g, 3g+1, 3g+2 hold c0, c1, c2; lane 63 of a wave
// idles).  Schoolbook, three Fp products per lane:
//   c_j = sum_{m <= j} a_(j-m) b_m + NR sum_{m > j} a_(j-m+3) b_m
// A lane's three products are ONE triple product with a single reduction (fp_mul3: 2704 mads), issued as ONE out-of-line
// device function (f3s_mul_outlined: lane rotations, the two NR multiples, the operand selection and the triple product),
// at 1 wave / SIMD.  One body per kernel instead of one per product site is what lets hipcc get through the kernels at all:
// the same code inlined at every site had not compiled after an hour.  Measured against it (2^19 pairs): three plain
// products in a rolled loop (4056 mads, 2 waves / SIMD) took the projective accumulation 222 instead of 167 ms, the bucket
// reduction 17.4 instead of 13.6 ms and the affine rounds 133 instead of 98 ms; the outlined product at 2 waves / SIMD
// spilled 1.4 KB in the caller (140 ms).  Two Fp arguments and an Fp result travel in VGPRs / on the stack.
template <class P, int NR> __device__ __attribute__((noinline)) Fp f3s_mul_outlined(Fp a, Fp b) {
    const int lane = threadIdx.x & 63, j = lane % 3, base = lane - j;
    const int s1 = base + (j + 1) % 3, s2 = base + (j + 2) % 3;
    // c_j = a_j b_0 + [NR if j = 0] a_(j-1) b_1 + [NR if j < 2] a_(j-2) b_2     (indices mod 3): b_0, b_1, b_2 are the same
    // for the three lanes (broadcasts within the triple); the NR multiples by fp_mul_small_rt with k = NR / 1 per lane
    Fp an, ap, y1, y2, y3;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        an.l[i] = (uint32_t)__shfl((int)a.l[i], s1); ap.l[i] = (uint32_t)__shfl((int)a.l[i], s2);
        y1.l[i] = (uint32_t)__shfl((int)b.l[i], base); y2.l[i] = (uint32_t)__shfl((int)b.l[i], base + 1);
        y3.l[i] = (uint32_t)__shfl((int)b.l[i], base + 2);
    }
    const Fp x2 = fp_mul_small_rt<P>(ap, j == 0 ? (uint32_t)NR : 1u), x3 = fp_mul_small_rt<P>(an, j < 2 ? (uint32_t)NR : 1u);
    return fp_mul3<P>(a, y1, x2, y2, x3, y3);
}

template <class P, int NR> struct F3S {
    typedef Fp T;
    static constexpr int DEG = 1;
    static constexpr int LANES = 3;
    static constexpr int WAVES = 1;
    static __device__ __forceinline__ int comp() { return (int)((threadIdx.x & 63u) % 3u); }
    static __device__ __forceinline__ T rot(const T& a, int by) {   // coefficient held by lane (comp + by) mod 3 of this triple
        const int lane = threadIdx.x & 63, j = lane % 3, src = lane - j + (j + by) % 3;
        T r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.l[i] = (uint32_t)__shfl((int)a.l[i], src);
        return r;
    }
    static __device__ __forceinline__ T zero() { return fp_zero(); }
    static __device__ __forceinline__ T one() { return comp() == 0 ? fp_one<P>() : fp_zero(); }
    static __device__ __forceinline__ T add(const T& a, const T& b) { return fp_add<P>(a, b); }
    static __device__ __forceinline__ T sub(const T& a, const T& b) { return fp_sub<P>(a, b); }
    static __device__ __forceinline__ T dbl(const T& a) { return fp_dbl<P>(a); }
    static __device__ __forceinline__ T neg(const T& a) { return fp_neg<P>(a); }
    static __device__ __forceinline__ T mul(const T& a, const T& b) { return f3s_mul_outlined<P, NR>(a, b); }
    static __device__ __forceinline__ T sqr(const T& a) { return mul(a, a); }
    static __device__ __forceinline__ T mul_sub_mul(const T& a, const T& b, const T& c, const T& d) { return sub(mul(a, b), mul(c, d)); }
    static __device__ __forceinline__ T sub_lazy(const T& a, const T& b) { return fp_sub<P>(a, b); }   // the triple product takes reduced operands
    // norm-based inverse in Fp[X]/(X^3 - NR) (fp3.rs inverse), one Fp inversion per lane triple:
    //   c0 = a0^2 - NR a1 a2,  c1 = NR a2^2 - a0 a1,  c2 = a1^2 - a0 a2,  n = a0 c0 + NR (a2 c1 + a1 c2),  a^-1 = c / n
    // lane j holds a_j: it forms its own square and the product a_j a_(j+1), the rest travels by lane rotation.
    static __device__ __forceinline__ T inv(const T& a) {
        const int j = comp();
        const T a1 = rot(a, 1), a2 = rot(a, 2);                      // a_(j+1), a_(j+2)
        const T sq = fp_sqr<P>(a), pr = fp_mul<P>(a, a1);            // a_j^2, a_j a_(j+1):  pr = (a0 a1, a1 a2, a2 a0)
        const T sq1 = rot(sq, 1), sq2 = rot(sq, 2), pr1 = rot(pr, 1), pr2 = rot(pr, 2);
        // c_j:  j = 0: sq_0 - NR pr_1     j = 1: NR sq_2 - pr_0     j = 2: sq_1 - pr_2
        const T u = j == 0 ? sq : (j == 1 ? fp_mul_small<P, NR>(sq1) : sq2);      // lane 1: sq_2 = sq_(j+1); lane 2: sq_1 = sq_(j+2)
        const T v = j == 0 ? fp_mul_small<P, NR>(pr1) : (j == 1 ? pr2 : pr);      // lane 0: pr_1; lane 1: pr_0 = pr_(j+2); lane 2: pr_2 = own
        const T c = fp_sub<P>(u, v);
        // n = a0 c0 + NR (a2 c1 + a1 c2): lane j multiplies c_j by a_0, a_2, a_1
        const T q = fp_mul<P>(j == 0 ? a : (j == 1 ? a1 : a2), c);  // lane 1: a_2 = a_(j+1); lane 2: a_1 = a_(j+2)
        const T q1 = rot(q, 1), q2 = rot(q, 2);
        const T q0v = j == 0 ? q : (j == 1 ? q2 : q1);              // q_0 as seen from lane j
        const T qs = j == 0 ? fp_add<P>(q1, q2) : (j == 1 ? fp_add<P>(q, q1) : fp_add<P>(q2, q));   // q_1 + q_2
        const T n = fp_add<P>(q0v, fp_mul_small<P, NR>(qs));
        return fp_mul<P>(c, fp_inv<P>(n));
    }
    static __device__ __forceinline__ bool all3(bool z) {
        const int lane = threadIdx.x & 63, j = lane % 3, b = lane - j;
        const int v = z ? 1 : 0;
        return (__shfl(v, b) & __shfl(v, b + 1) & __shfl(v, b + 2)) != 0;
    }
    static __device__ __forceinline__ bool is_zero(const T& a) { return all3(fp_is_zero(a)); }
    static __device__ __forceinline__ bool eq(const T& a, const T& b) { return all3(fp_eq(a, b)); }
};

// Same task list, salt detour and addition (madd-1998-cmo) as section 4, LANES lanes per task (2: Fq2 pairs, 3: Fq3
// triples; a wave carries 64 / LANES tasks, the remaining lane of a triple wave idles).
// AFFIN: as in section 4 -- the input is the T64 output list of the affine rounds.
template <class C, class F, int LANES, bool AFFIN = false>
__global__ void __launch_bounds__(256, F::WAVES)
msm_accumulate_split_kernel(const Aff<C>* __restrict__ bases, const uint32_t* __restrict__ sorted,
                           const uint32_t* __restrict__ starts, const uint32_t* __restrict__ counts,
                           const uint32_t* __restrict__ order, uint32_t total,
                           const Aff<C>* __restrict__ salts, Proj<C>* __restrict__ buckets,
                           const uint32_t* __restrict__ chunk_start, uint32_t n_heavy, uint32_t n_chunks, uint32_t chunk,
                           Proj<C>* __restrict__ partials, uint32_t g_first = 0, uint32_t list_base = 0) {
    constexpr uint32_t TPW = 64 / LANES;                       // tasks per wave
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t t = wave * TPW + lane / LANES;
    const int comp = (int)(lane % LANES);
    const uint32_t ntasks = n_chunks + (total - n_heavy);
    const bool live = lane < TPW * LANES && t < ntasks;       // all lanes of a group agree
    uint32_t beg = 0, cnt = 0;
    Proj<C>* dst = buckets;
    if (live) {
        const auto tk = acc_task_decode<AFFIN>(t, starts, counts, order, buckets, chunk_start, n_heavy, n_chunks, chunk, partials, g_first, list_base);
        beg = tk.beg; cnt = tk.cnt; dst = tk.dst;
    }
    __shared__ uint32_t park[NL][256];
    Fp ax = fp_zero(), ay = F::one(), az = fp_zero();   // (0, 1, 0)
    uint32_t k = 0;
    int phase = 0, salt_id = 0;
    uint32_t guard = 0;
    // the loop condition is uniform within a lane group (its lanes share cnt, k, phase)
    while (k < cnt && guard < 4 * cnt + 8) {
        guard++;
        Fp qx, qy;
        if (phase == 1 || phase == 3) {
            qx = ld_coeff<LANES>(salts + salt_id, 0, comp);
            qy = ld_coeff<LANES>(salts + salt_id, 1, comp);
            if (phase == 3) qy = F::neg(qy);
        } else if constexpr (AFFIN) {
            const uint32_t e = beg + k;
            const size_t tile = e / TPW;
            const uint32_t slot = (e % TPW) * LANES + (uint32_t)comp;
            qx = t64_ld_x(bases, tile, slot);
            qy = t64_ld_y(bases, tile, slot);
            if (phase == 0 && k < cnt && qx.l[0] == AFF_MARK) { k++; continue; }   // a cancelled pair (every lane of the group sees the marker)
        } else {
            const uint32_t e = sorted[beg + k];
            const Aff<C>* b = bases + (e & 0x7FFFFFFFu);
            qx = ld_coeff<LANES>(b, 0, comp);
            qy = ld_coeff<LANES>(b, 1, comp);
            if (e >> 31) qy = F::neg(qy);
        }
        if (F::is_zero(az)) {
            ax = qx; ay = qy; az = F::one();
        } else {
            Fp v = F::mul(qx, az);
            Fp u = F::mul(qy, az);
            if (phase == 0 && F::eq(u, ay) && F::eq(v, ax)) {
                salt_id = F::eq(qx, ld_coeff<LANES>(salts, 0, comp)) ? 1 : 0;
                phase = 1;
                continue;
            }
            u = F::sub(u, ay);
            v = F::sub(v, ax);
#pragma unroll
            for (int w = 0; w < NL; w++) park[w][threadIdx.x] = ay.l[w];
            __builtin_amdgcn_sched_barrier(0);
            Fp vv = F::sqr(v);
            __builtin_amdgcn_sched_barrier(0);
            Fp r = F::mul(vv, ax);
            __builtin_amdgcn_sched_barrier(0);
            Fp vvv = F::mul(v, vv);
            __builtin_amdgcn_sched_barrier(0);
            Fp uu = F::sqr(u);
            __builtin_amdgcn_sched_barrier(0);
            Fp a = F::sub(F::sub(F::mul(uu, az), vvv), F::dbl(r));
            __builtin_amdgcn_sched_barrier(0);
            ax = F::mul(v, a);
            __builtin_amdgcn_sched_barrier(0);
            Fp t1 = F::mul(u, F::sub(r, a));
            __builtin_amdgcn_sched_barrier(0);
            Fp y1;
#pragma unroll
            for (int w = 0; w < NL; w++) y1.l[w] = park[w][threadIdx.x];
            ay = F::sub(t1, F::mul(vvv, y1));
            __builtin_amdgcn_sched_barrier(0);
            az = F::mul(vvv, az);
        }
        if (phase == 0 || phase == 3) { k++; phase = 0; } else phase++;
    }
    if (live) {
        st_coeff<LANES>(dst, 0, comp, ax);
        st_coeff<LANES>(dst, 1, comp, ay);
        st_coeff<LANES>(dst, 2, comp, az);
    }
}

// wave-level sum of one projective point per lane through LDS; result valid in lane 0.
// sh must hold 64 Proj<C>.  All 64 lanes must call.
template <class C>
__device__ __forceinline__ Proj<C> wave_tree_sum(Proj<C> v, Proj<C>* sh, int lane) {
    for (int off = 32; off > 0; off >>= 1) {
        if (lane >= off && lane < 2 * off) st_proj<C>(sh + lane, v);
        __syncthreads();
        if (lane < off) v = proj_add_call<C>(v, ld_proj<C>(sh + lane + off));
        __syncthreads();
    }
    return v;
}

// Heavy buckets (skewed scalars, sparsely populated top windows) are cut into chunks of heavy_thr
// entries that the accumulation kernel sums like ordinary buckets (chunk mode above, into
// partials[]); this kernel then adds the chunk sums of each heavy bucket: lanes stride through
// them, then a tree through LDS.
template <class C>
__global__ void __launch_bounds__(64, 2)
msm_heavy_combine_kernel(const Proj<C>* __restrict__ partials, const uint32_t* __restrict__ order,
                         const uint32_t* __restrict__ chunk_start, Proj<C>* __restrict__ buckets) {
    extern __shared__ uint32_t lds_raw[];
    Proj<C>* sh = reinterpret_cast<Proj<C>*>(lds_raw);
    const int lane = threadIdx.x;
    const uint32_t h = blockIdx.x;
    const uint32_t beg = chunk_start[h], end = chunk_start[h + 1];
    Proj<C> acc = proj_zero<C>();
    for (uint32_t k = beg + lane; k < end; k += 64) acc = proj_add_call<C>(acc, ld_proj<C>(partials + k));
    acc = wave_tree_sum<C>(acc, sh, lane);
    if (lane == 0) st_proj<C>(buckets + order[h], acc);
}

}  // namespace gh

// ---------------------------------------------------------------- 5. bucket reduction: msm_reduce_kernels.h
#include "msm_reduce_kernels.h"
