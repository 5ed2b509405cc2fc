// msm_reduce_kernels.h -- step 5 of the MSM (msm_kernels.h): the bucket reduction.
//
// sum_b b * B_b per window, without the reference's per-window inversion (variable_base.rs:60-66)
// and without any doubling or function call on the device.
//
// The reduction is a "wave program": one wave per segment of TPW * L consecutive items of one window, TPW = 2^LT groups per
// wave, group g owns items g, g + TPW, g + 2 TPW, ... (stride TPW).  Every step of the program is
// one projective addition issued from a SINGLE inlined call site (operands are selected per
// step; the earlier call-based version moved ~7 KB of scratch per addition and was
// scratch-bandwidth bound).  The program's accumulators are parked in a global slab between steps
// (WaveSlab below).  The steps:
//   steps 0 .. 2L-2   serial:  run += item_i  (i = L-1 .. 0),  wacc += run      -> run_g = sum_i x,
//                                                                                   wacc_g = sum_i i * x
//   LT steps          tree over groups of wacc                   -> A  = sum_g wacc_g
//   LT steps          suffix scan over groups of run             -> S_g = sum_{m >= g} run_m;  runW = S_0
//   LT steps          tree over groups g >= 1 of S               -> Bv = sum_g g * run_g
// With item index = g + TPW i:   sum_items index * x = TPW * A + Bv,  sum_items x = runW.
// mode 1 (plain sum) stops after the serial part and a tree over run.
// mode 2 ("lean" level 1, msm_impl.h; G1 only) stops after the serial part and stores every lane's (run_l, wacc_l) -- out[(program * 64
// + l) * 2 + {0, 1}] -- for a second level that works on LANES instead of segments: the 18 cross-lane steps, in which most
// lanes idle, are then issued once per window instead of once per segment.
// Equal operands (acc == x as points, the reference's doubling branch) are detected in the
// addition; the whole wave then spends three extra steps on a detour through a salt point
// (p + S) + q - S for the affected groups.  Powers of two (TPW, TPW L) that weight the outputs are
// NOT applied here: they are folded into the host's Horner loop over the windows, where the
// doublings are needed anyway (msm_fold.h: fold_windows).
//
// The loop exists three times.  wave_reduce_program<View> is the form to read and to change first: it runs over the HIP-free
// schedule and detour state of msm_schedule.h, which tests/test_msm_host.py runs on the host, and a view (GroupView: one
// coefficient of a P3 per lane of a pair / triple) says how a lane reaches its point.  The Fq3 build of
// msm_wave_reduce_split_kernel runs it.  msm_wave_reduce_kernel (G1, a whole Proj<C> per lane) and the Fq2 build of the split
// kernel keep the loop WRITTEN OUT, because their register allocation does not survive a shared piece: the notes above the two
// kernels have the figures.  A change to the program has to be repeated in both.  tests/test_msm_host.py sees msm_schedule.h
// only; the three copies themselves are compared on the card, build by build, with sums written down by definition
// (tests/test_gpu_msm_reduce.py over tests/device_shim/msm_reduce.hip: every step kind and tree offset with equal operands,
// both salts, infinite operands, all shapes of count, valid, stride and run_if).
#pragma once
#include "msm_kernels.h"

namespace gh {

template <class C> struct WaveReduceIn {
    const Proj<C>* base;   // item (w, k) = base[(w * count + k) * stride + offset]
    uint32_t stride, offset, count, mode;
    uint32_t valid;        // items with flat index w * count + k >= valid are padding (infinity)
};

template <class C> struct ReduceField { typedef typename C::F type; };          // G1: inlined products
template <> struct ReduceField<Mnt4G2> { typedef Mnt4G2::FC type; };                 // towers: out of line (code size)
template <> struct ReduceField<Mnt6G2> { typedef Mnt6G2::FC type; };

// A block may carry blockDim.x / 64 INDEPENDENT waves (each its own program and LDS region, so the
// exchanges need wave-level ordering only, no s_barrier).  Measured at 2^20 buckets: 1, 2, 3 or 4
// waves per block, with or without a block barrier per step, all take the same time for level 1
// -- the default is 1.
#define GH_WAVE_SYNC()                                           \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)
// Branch-free projective addition; same = (p == q as points).  WITHOUT final selects for the infinity cases: p and q are dead
// after the first five products, which is what lets the step fit the register budget; the caller patches the lanes with an
// infinite operand (pz / qz) from re-loaded operands.
template <class C> __device__ __forceinline__ Proj<C> proj_add_raw(const Proj<C>& p, const Proj<C>& q, bool& same, bool& pz, bool& qz) {
    typedef typename ReduceField<C>::type F;
#define GH_RFENCE() __builtin_amdgcn_sched_barrier(0)      // keep the written order: at most eight field elements live
    pz = F::is_zero(p.z); qz = F::is_zero(q.z);
    typename F::T y1z2 = F::mul(p.y, q.z);
    GH_RFENCE();
    typename F::T u = F::sub(F::mul(p.z, q.y), y1z2);
    GH_RFENCE();
    typename F::T x1z2 = F::mul(p.x, q.z);
    GH_RFENCE();
    typename F::T v = F::sub(F::mul(p.z, q.x), x1z2);
    GH_RFENCE();
    typename F::T z1z2 = F::mul(p.z, q.z);                 // p, q dead
    GH_RFENCE();
    same = !pz && !qz && F::is_zero(u) && F::is_zero(v);
    typename F::T vv = F::sqr(v);
    GH_RFENCE();
    typename F::T r = F::mul(vv, x1z2);                    // x1z2 dead
    GH_RFENCE();
    typename F::T vvv = F::mul(v, vv);                     // vv dead
    GH_RFENCE();
    typename F::T uu = F::sqr(u);
    GH_RFENCE();
    typename F::T a = F::sub(F::sub(F::mul(uu, z1z2), vvv), F::dbl(r));   // uu dead
    GH_RFENCE();
    Proj<C> o;
    o.x = F::mul(v, a);                                    // v dead
    GH_RFENCE();
    o.z = F::mul(vvv, z1z2);                               // z1z2 dead
    GH_RFENCE();
    // Y3 = (r - a) u - vvv y1z2 as ONE dual product on a single accumulator chain (fp_mul2s, as in the XYZZ accumulation: one
    // Montgomery reduction of fourteen saved; the kernel's scratch frame is unchanged by it: 736 -> 640 B per lane in the
    // 512-register build, 1760 -> 1792 B in the 256-register one).  The towers keep two products.
    o.y = F::mul_sub_mul1(F::sub(r, a), u, vvv, y1z2);
#undef GH_RFENCE
    return o;
}

// A point of the lane-group view: one coefficient of each coordinate per lane.
struct P3 { Fp x, y, z; };
template <class FS> __device__ __forceinline__ P3 p3_zero() { return P3{fp_zero(), FS::one(), fp_zero()}; }
// without the final operand selects (see proj_add_raw): the caller patches lanes with an infinite operand
template <class FS> __device__ __forceinline__ P3 p3_add_raw(const P3& p, const P3& q, bool& same, bool& pz, bool& qz) {
    pz = FS::is_zero(p.z); qz = FS::is_zero(q.z);
    Fp y1z2 = FS::mul(p.y, q.z);
    Fp u = FS::sub(FS::mul(p.z, q.y), y1z2);
    Fp x1z2 = FS::mul(p.x, q.z);
    Fp v = FS::sub(FS::mul(p.z, q.x), x1z2);
    Fp z1z2 = FS::mul(p.z, q.z);
    same = !pz && !qz && FS::is_zero(u) && FS::is_zero(v);
    Fp vv = FS::sqr(v);
    Fp r = FS::mul(vv, x1z2);
    Fp vvv = FS::mul(v, vv);
    Fp uu = FS::sqr(u);
    Fp a = FS::sub(FS::sub(FS::mul(uu, z1z2), vvv), FS::dbl(r));
    P3 o;
    o.x = FS::mul(v, a);
    o.z = FS::mul(vvv, z1z2);
    o.y = FS::sub(FS::mul(FS::sub(r, a), u), FS::mul(vvv, y1z2));
    return o;
}

// The three accumulators of a program (run, wacc, and tmp of the salt detour) live in a per-program slab of global memory,
// word-major (slab[(slot * NW + word) * 64 + lane]: one 256-byte row per wave instruction), and only the operand of the
// current step is in registers: with all three held in registers next to the operands of the addition the compiler
// spilled 2.4 KB per lane -- 848 scratch instructions per step against the 156-234 explicit ones now.
// T: what a lane holds of a point (Proj<C> on G1, P3 in a lane group).
template <class T> struct WaveSlab {
    static constexpr int NW = (int)(sizeof(T) / 4);
    static constexpr size_t WORDS = (size_t)3 * NW * 64;      // per program
    static __device__ __forceinline__ T ld(const uint32_t* slab, int slot, int lane) {
        T v;
        uint32_t* w = reinterpret_cast<uint32_t*>(&v);
        const uint32_t* p = slab + (size_t)slot * NW * 64 + lane;
#pragma unroll
        for (int k = 0; k < NW; k++) w[k] = p[(size_t)k * 64];
        return v;
    }
    static __device__ __forceinline__ void st(uint32_t* slab, int slot, int lane, const T& v) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
        uint32_t* p = slab + (size_t)slot * NW * 64 + lane;
#pragma unroll
        for (int k = 0; k < NW; k++) p[(size_t)k * 64] = w[k];
    }
};

// r = p + q where an operand is infinity, word by word: q if p is (pz), p if q is (qz), else r as computed
template <class T> __device__ __forceinline__ void wave_select(T& r, const T& p, const T& q, bool pz, bool qz) {
    uint32_t* rw = reinterpret_cast<uint32_t*>(&r);
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(&p);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(&q);
#pragma unroll
    for (int k = 0; k < WaveSlab<T>::NW; k++) rw[k] = pz ? qw[k] : (qz ? pw[k] : rw[k]);
}

// ---------------------------------------------------------------- the view of a lane group
// G2: TPW groups of LANES lanes, lane comp of group g holds coefficient comp of each coordinate; the lanes from TPW * LANES
// on idle (g = TPW).  Every addition runs on inlined Fp products in registers (the split field policies of msm_kernels.h 4b).
template <class C, class FS, int LANES, int TPW_> struct GroupView {
    typedef P3 T;
    static constexpr int TPW = TPW_, LT = TPW == 32 ? 5 : (TPW == 16 ? 4 : 6);
    static_assert((1 << LT) == TPW && TPW * LANES <= 64, "groups per wave");
    int lane, g, comp;
    P3* sh;
    __device__ __forceinline__ bool live() const { return lane < TPW * LANES; }
    __device__ __forceinline__ T zero() const { return p3_zero<FS>(); }
    __device__ __forceinline__ T ld_item(const Proj<C>* pt) const {
        return P3{ld_coeff<LANES>(pt, 0, comp), ld_coeff<LANES>(pt, 1, comp), ld_coeff<LANES>(pt, 2, comp)};
    }
    __device__ __forceinline__ T ld_salt(const Aff<C>* s, bool negate) const {
        P3 q{ld_coeff<LANES>(s, 0, comp), ld_coeff<LANES>(s, 1, comp), FS::one()};
        if (negate) q.y = FS::neg(q.y);
        return q;
    }
    __device__ __forceinline__ void st_out(Proj<C>* pt, const T& v) const {
        st_coeff<LANES>(pt, 0, comp, v.x); st_coeff<LANES>(pt, 1, comp, v.y); st_coeff<LANES>(pt, 2, comp, v.z);
    }
    __device__ __forceinline__ void sh_store(const T& v) const {
        uint2* d = reinterpret_cast<uint2*>(sh + lane);
        const uint2* sv = reinterpret_cast<const uint2*>(&v);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(P3) / 8); k++) d[k] = sv[k];
    }
    __device__ __forceinline__ T sh_load(int off) const {
        P3 v;
        const uint2* sv = reinterpret_cast<const uint2*>(sh + lane + off * LANES);
        uint2* d = reinterpret_cast<uint2*>(&v);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(P3) / 8); k++) d[k] = sv[k];
        return v;
    }
    __device__ __forceinline__ T add(const T& p, const T& q, bool& same, bool& pz, bool& qz) const {
        return p3_add_raw<FS>(p, q, same, pz, qz);
    }
    // salt with x != p.x / p.z  (all lanes run the product: the group shuffles need their partners)
    __device__ __forceinline__ int choose_salt(const Aff<C>* salts, const uint32_t* slab, int src, bool same, int cur) const {
        const T p = WaveSlab<T>::ld(slab, src, lane);
        const bool s0_hits = FS::eq(FS::mul(ld_coeff<LANES>(salts, 0, comp), p.z), p.x);
        return same ? (s0_hits ? 1 : 0) : cur;
    }
};

// ---------------------------------------------------------------- the program
// Program gb = which * blocks_per_input + blk reduces segment blk of its input; slab: this program's WaveSlab.  Modes 0 and 1
// only: mode 2 (lean) is NOT SUPPORTED here, not merely unused -- its serial-only sums would be stored as (A, Bv).  The plan
// asks for it on G1 alone (msm_plan.h), whose kernel has it.
template <class V, class C>
__device__ __forceinline__ void wave_reduce_program(const V& v, const WaveReduceIn<C>& in, uint32_t gb, uint32_t blk,
                                                    uint32_t segs_per_window, int L, const Aff<C>* __restrict__ salts,
                                                    Proj<C>* __restrict__ out, uint32_t* __restrict__ slab) {
    typedef typename V::T T;
    typedef WaveSlab<T> SL;
    enum { RUN = 0, WACC = 1, TMP = 2 };
    const int lane = v.lane;
    const uint32_t w = blk / segs_per_window, seg = blk % segs_per_window;
    const uint32_t item0 = seg * (uint32_t)V::TPW * (uint32_t)L;
    Proj<C>* o = out + (size_t)gb * 3;                      // runW, A, Bv  (mode 1: the sum)
    if ((size_t)w * in.count + item0 >= (size_t)in.valid) {   // segment of padding slots only: all sums are infinity
        const T z = v.zero();
        if (v.g == 0) { v.st_out(o, z); v.st_out(o + 1, z); v.st_out(o + 2, z); }
        return;
    }
    {
        const T z = v.zero();
        SL::st(slab, RUN, lane, z); SL::st(slab, WACC, lane, z); SL::st(slab, TMP, lane, z);
    }
    const int NST = wave_total_steps(in.mode, L, V::LT);
    WaveCursor c;
    while (c.step < NST) {
        const WaveStep s = wave_step(in.mode, L, V::LT, c.step);
        if (s.publish && c.det == 0 && v.g == 0) {   // between scan and the last tree: publish runW = S_0, drop group 0 from the tree
            v.st_out(o, SL::ld(slab, RUN, lane)); SL::st(slab, RUN, lane, v.zero());
        }
        const bool exch = s.kind >= WS_TREE_WACC;
        if (exch && c.det == 0) v.sh_store(SL::ld(slab, s.kind == WS_TREE_WACC ? WACC : RUN, lane));
        if (exch) GH_WAVE_SYNC();
        const int dst = (s.kind == WS_WACC || s.kind == WS_TREE_WACC) ? WACC : RUN;
        const uint32_t k = item0 + (uint32_t)v.g + (uint32_t)V::TPW * (uint32_t)s.i;   // the group's item i
        const bool in_step = v.live() && wave_step_active(s, v.g, V::TPW, k < in.count);
        const bool active = c.det > 0 ? c.mydet : in_step;
        // the step's second operand (re-loadable: it is read again below for the lanes whose sum is one of the operands)
        auto load_q = [&]() -> T {
            if (c.salted()) return v.ld_salt(salts + c.salt_id, c.det == 3);
            if (s.kind == WS_WACC) return SL::ld(slab, RUN, lane);
            T q = v.zero();
            if (in_step) {
                if (s.kind == WS_ITEM) q = v.ld_item(in.base + ((size_t)w * in.count + k) * in.stride + in.offset);
                else q = v.sh_load(s.off);
            }
            return q;
        };
        const int src = c.detour_reads_tmp() ? TMP : dst;
        bool same, pz, qz;
        T r;
        {
            const T q = load_q();
            const T p = SL::ld(slab, src, lane);
            r = v.add(p, q, same, pz, qz);
        }
        if (__any((pz || qz) && active)) {   // p + infinity = p, infinity + q = q: patch those lanes from the operands, read again
            const T q = load_q();
            const T p = SL::ld(slab, src, lane);
            wave_select(r, p, q, pz, qz);
        }
        if (exch) GH_WAVE_SYNC();
        same = same && active;
        if (c.det == 0) {
            const bool any_same = __any(same) != 0;
            if (active && !same) SL::st(slab, dst, lane, r);
            if (any_same) c.salt_id = v.choose_salt(salts, slab, src, same, c.salt_id);
            c.advance(same, any_same);
        } else {
            if (c.mydet) SL::st(slab, c.detour_writes_tmp() ? TMP : dst, lane, r);
            c.advance(false, false);
        }
    }
    if (v.g == 0) {
        if (in.mode == 1) {
            v.st_out(o, SL::ld(slab, RUN, lane));
        } else {
            v.st_out(o + 1, SL::ld(slab, WACC, lane));
            v.st_out(o + 2, SL::ld(slab, RUN, lane));
        }
    }
}

// ---------------------------------------------------------------- G1: one point per lane
// The loop of wave_reduce_program, WRITTEN OUT with group = lane, every lane live, the salt choice in the `same` lanes only
// (out-of-line C::FC product) and the lean mode 2.  It does not call the program or its pieces: the four builds of this kernel
// (two curves, 512 and 256 registers) sit at 656 / 1824 / 672 / 1872 B of scratch per lane, and every shared piece moves them,
// up or down, by 16 or 32 B -- the program itself (672 / 1856 / 688 / 1904), and this loop calling only wave_step (672 / 1824 /
// 672 / 1872, VGPR spills 11 / 323 / 11 / 322 for 6 / 321 / 9 / 319), only WaveCursor (672 / 1840 / 688 / 1872) or only wave_select
// (640 / 1824 / 656 / 1840), a function that holds nothing but the loop of the patch below (profiles/msm_kernel_parity.md).
template <class C, int WAVES = 2>
__global__ void __launch_bounds__(256, WAVES)
msm_wave_reduce_kernel(WaveReduceIn<C> in0, WaveReduceIn<C> in1, WaveReduceIn<C> in2, uint32_t blocks_per_input,
                       uint32_t n_inputs, uint32_t segs_per_window, int L, const Aff<C>* __restrict__ salts,
                       Proj<C>* __restrict__ out, uint32_t* __restrict__ slabs, const uint32_t* __restrict__ run_if) {
    typedef typename C::F F;
    typedef WaveSlab<Proj<C>> SL;
    enum { RUN = 0, WACC = 1, TMP = 2 };
    extern __shared__ uint32_t lds_raw[];
    const int lane = threadIdx.x & 63;
    Proj<C>* sh = reinterpret_cast<Proj<C>*>(lds_raw) + 64 * (threadIdx.x >> 6);
    const uint32_t gb = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // one program per wave
    if (gb >= n_inputs * blocks_per_input) return;
    // run_if (lean level 1 behind the generated kernel, asmgen/g1_reduce.py): only the programs that kernel flagged -- they met a
    // doubling, which it leaves to the detour below -- are computed, whole, from the buckets
    if (run_if && run_if[gb] == 0) return;
    const uint32_t which = gb / blocks_per_input, blk = gb % blocks_per_input;
    const WaveReduceIn<C> in = which == 0 ? in0 : (which == 1 ? in1 : in2);
    const uint32_t w = blk / segs_per_window, seg = blk % segs_per_window;
    const uint32_t item0 = seg * 64u * (uint32_t)L;
    if ((size_t)w * in.count + item0 >= (size_t)in.valid) {   // segment of padding slots only: all sums are infinity
        if (in.mode == 2) {
            const Proj<C> z = proj_zero<C>();
            st_proj<C>(out + ((size_t)blk * 64 + lane) * 2, z); st_proj<C>(out + ((size_t)blk * 64 + lane) * 2 + 1, z);
        } else if (lane == 0) {
            Proj<C>* oz = out + ((size_t)which * blocks_per_input + blk) * 3;
            const Proj<C> z = proj_zero<C>();
            st_proj<C>(oz, z); st_proj<C>(oz + 1, z); st_proj<C>(oz + 2, z);
        }
        return;
    }
    const int NS1 = in.mode == 1 ? L : 2 * L - 1;
    const int NST = in.mode == 1 ? L + 6 : (in.mode == 2 ? NS1 : NS1 + 18);
    uint32_t* slab = slabs + (size_t)gb * SL::WORDS;
    {
        const Proj<C> z = proj_zero<C>();
        SL::st(slab, RUN, lane, z); SL::st(slab, WACC, lane, z); SL::st(slab, TMP, lane, z);
    }
    int step = 0, det = 0, salt_id = 0;
    bool mydet = false, mid_done = false;
    Proj<C>* o = out + ((size_t)which * blocks_per_input + blk) * 3;
    while (step < NST) {
        int kind, off = 0, i = 0;
        if (step < NS1) {
            if (in.mode == 1) { kind = 0; i = L - 1 - step; }
            else { kind = (step & 1) ? 1 : 0; i = L - 1 - (step >> 1); }
        } else if (in.mode == 1) { kind = 4; off = 32 >> (step - NS1); }
        else if (step < NS1 + 6) { kind = 2; off = 32 >> (step - NS1); }
        else if (step < NS1 + 12) { kind = 3; off = 1 << (step - NS1 - 6); }
        else {
            kind = 4; off = 32 >> (step - NS1 - 12);
            if (!mid_done) {   // between scan and the last tree: publish runW = S_0, drop lane 0 from the tree
                if (lane == 0) { st_proj<C>(o, SL::ld(slab, RUN, lane)); SL::st(slab, RUN, lane, proj_zero<C>()); }
                mid_done = true;
            }
        }
        const bool exch = kind >= 2;
        if (exch && det == 0) st_proj<C>(sh + lane, SL::ld(slab, kind == 2 ? WACC : RUN, lane));
        if (exch) GH_WAVE_SYNC();
        const bool to_wacc = kind == 1 || kind == 2;
        const int dst = to_wacc ? WACC : RUN;
        bool active;
        if (kind == 0) active = item0 + (uint32_t)lane + 64u * (uint32_t)i < in.count;
        else if (kind == 1) active = true;
        else active = kind == 3 ? lane + off < 64 : lane < off;
        if (det > 0) active = mydet;
        // the step's second operand (re-loadable: it is read again below for the lanes whose sum is one of the operands)
        auto load_q = [&]() -> Proj<C> {
            Proj<C> q = proj_zero<C>();
            if (det == 1 || det == 3) {
                const Aff<C> sp = ld_aff<C>(salts + salt_id);
                q.x = sp.x; q.y = det == 3 ? F::neg(sp.y) : sp.y; q.z = F::one();
            } else if (kind == 0) {
                const uint32_t k = item0 + (uint32_t)lane + 64u * (uint32_t)i;
                if (k < in.count) q = ld_proj<C>(in.base + ((size_t)w * in.count + k) * in.stride + in.offset);
            } else if (kind == 1) {
                q = SL::ld(slab, RUN, lane);
            } else {
                const int partner = lane + off;
                if (kind == 3 ? partner < 64 : lane < off) q = ld_proj<C>(sh + partner);
            }
            return q;
        };
        const int src = det >= 2 ? TMP : dst;
        bool same, pz, qz;
        Proj<C> r;
        {
            const Proj<C> q = load_q();
            const Proj<C> p = SL::ld(slab, src, lane);
            r = proj_add_raw<C>(p, q, same, pz, qz);
        }
        if (__any((pz || qz) && active)) {   // p + infinity = p, infinity + q = q: patch those lanes from the operands, read again
            const Proj<C> q = load_q();
            const Proj<C> p = SL::ld(slab, src, lane);
            uint32_t* rw = reinterpret_cast<uint32_t*>(&r);
            const uint32_t* pw = reinterpret_cast<const uint32_t*>(&p);
            const uint32_t* qw = reinterpret_cast<const uint32_t*>(&q);
#pragma unroll
            for (int k = 0; k < SL::NW; k++) rw[k] = pz ? qw[k] : (qz ? pw[k] : rw[k]);
        }
        if (exch) GH_WAVE_SYNC();
        same = same && active;
        if (det == 0) {
            const bool any_same = __any(same) != 0;
            if (active && !same) SL::st(slab, dst, lane, r);
            if (any_same) {
                mydet = same;
                if (same) {   // salt with x != p.x / p.z  (rare path: out-of-line product)
                    const Proj<C> p = SL::ld(slab, src, lane);
                    Aff<C> s0 = ld_aff<C>(salts);
                    salt_id = C::FC::eq(C::FC::mul(s0.x, p.z), p.x) ? 1 : 0;
                }
                det = 1;
            } else {
                step++;
            }
        } else {
            if (mydet) SL::st(slab, det < 3 ? TMP : dst, lane, r);
            if (det == 3) { det = 0; mydet = false; step++; } else det++;
        }
    }
    if (in.mode == 2) {
        st_proj<C>(out + ((size_t)blk * 64 + lane) * 2, SL::ld(slab, RUN, lane));
        st_proj<C>(out + ((size_t)blk * 64 + lane) * 2 + 1, SL::ld(slab, WACC, lane));
    } else if (lane == 0) {
        if (in.mode == 1) {
            st_proj<C>(o, SL::ld(slab, RUN, lane));
        } else {
            st_proj<C>(o + 1, SL::ld(slab, WACC, lane));
            st_proj<C>(o + 2, SL::ld(slab, RUN, lane));
        }
    }
}

// ---------------------------------------------------------------- G2: lane groups
// The same wave program over the split field policies of msm_kernels.h 4b: a point of the program lives in a
// lane pair (Fq2) or triple (Fq3), one coefficient per lane, so a wave carries TPW = 32 / 16 items (Fq3:
// lanes 48..63 idle) and every addition runs on inlined Fp products in registers -- the tower version of
// msm_wave_reduce_kernel has to call out-of-line products whose operands travel through scratch.
// Item index = g + TPW * i (g = group, i = slot of the group), so  sum index * x = TPW * A + Bv.
//
// The Fq3 build runs wave_reduce_program over a GroupView.  The Fq2 build keeps the loop WRITTEN OUT below, the text the program
// was made from: with the program as its body the Fq2 kernel needs 324 instead of 148 B of scratch per lane, and still 308 to
// 320 B when its own loop merely calls wave_select, WaveCursor or wave_step (profiles/msm_kernel_parity.md has the remark lines);
// its access lambdas stay for the same reason.  A change to the program has to be made in that loop as well.
// (A 256-register build of this kernel -- two waves per SIMD, so that inside a batch a program would share its SIMD with a wave of
// the next MSM's round kernels -- was measured at the end of round 4: 2.4 KB of scratch per lane on Fq3, batches 2-3 % SLOWER.)
template <class C, class FS, int LANES, int TPW>
__global__ void __launch_bounds__(64, 1)
msm_wave_reduce_split_kernel(WaveReduceIn<C> in0, WaveReduceIn<C> in1, WaveReduceIn<C> in2, uint32_t blocks_per_input,
                             uint32_t n_inputs, uint32_t segs_per_window, int L, const Aff<C>* __restrict__ salts,
                             Proj<C>* __restrict__ out, uint32_t* __restrict__ slabs) {
    extern __shared__ uint32_t lds_raw[];
    if constexpr (LANES != 2) {
        const int lane = threadIdx.x & 63;
        const uint32_t gb = blockIdx.x;
        if (gb >= n_inputs * blocks_per_input) return;
        const uint32_t which = gb / blocks_per_input, blk = gb % blocks_per_input;
        const WaveReduceIn<C> in = which == 0 ? in0 : (which == 1 ? in1 : in2);
        const GroupView<C, FS, LANES, TPW> v{lane, lane < TPW * LANES ? lane / LANES : TPW, lane % LANES, reinterpret_cast<P3*>(lds_raw)};
        wave_reduce_program(v, in, gb, blk, segs_per_window, L, salts, out, slabs + (size_t)gb * WaveSlab<P3>::WORDS);
    } else {
        typedef WaveSlab<P3> SL;
        enum { RUN = 0, WACC = 1, TMP = 2 };
        constexpr int LT = TPW == 32 ? 5 : (TPW == 16 ? 4 : 6);
        static_assert((1 << LT) == TPW && TPW * LANES <= 64, "groups per wave");
        P3* sh = reinterpret_cast<P3*>(lds_raw);
        const int lane = threadIdx.x & 63;
        const bool live = lane < TPW * LANES;
        const int g = live ? lane / LANES : TPW, comp = lane % LANES;
        const uint32_t gb = blockIdx.x;
        if (gb >= n_inputs * blocks_per_input) return;
        const uint32_t which = gb / blocks_per_input, blk = gb % blocks_per_input;
        const WaveReduceIn<C> in = which == 0 ? in0 : (which == 1 ? in1 : in2);
        const uint32_t w = blk / segs_per_window, seg = blk % segs_per_window;
        const uint32_t item0 = seg * (uint32_t)TPW * (uint32_t)L;
        // coefficient `comp` of coordinate e of a projective / affine point in memory
        auto ld_c = [&](const void* pt, int e) { return ld_coeff<LANES>(pt, e, comp); };
        auto st_c = [&](void* pt, int e, const Fp& v) { st_coeff<LANES>(pt, e, comp, v); };
        auto st_p3 = [&](Proj<C>* pt, const P3& v) { st_c(pt, 0, v.x); st_c(pt, 1, v.y); st_c(pt, 2, v.z); };
        Proj<C>* o = out + ((size_t)which * blocks_per_input + blk) * 3;
        if ((size_t)w * in.count + item0 >= (size_t)in.valid) {   // segment of padding slots only
            if (g == 0) { const P3 z = p3_zero<FS>(); st_p3(o, z); st_p3(o + 1, z); st_p3(o + 2, z); }
            return;
        }
        const int NS1 = in.mode == 1 ? L : 2 * L - 1;
        const int NST = in.mode == 1 ? L + LT : NS1 + 3 * LT;
        uint32_t* slab = slabs + (size_t)gb * SL::WORDS;
        {
            const P3 z = p3_zero<FS>();
            SL::st(slab, RUN, lane, z); SL::st(slab, WACC, lane, z); SL::st(slab, TMP, lane, z);
        }
        int step = 0, det = 0, salt_id = 0;
        bool mydet = false, mid_done = false;
        auto sh_store = [&](const P3& v) {
            uint2* d = reinterpret_cast<uint2*>(sh + lane);
            const uint2* sv = reinterpret_cast<const uint2*>(&v);
#pragma unroll
            for (int k = 0; k < (int)(sizeof(P3) / 8); k++) d[k] = sv[k];
        };
        auto sh_load = [&](int src_lane) {
            P3 v;
            const uint2* sv = reinterpret_cast<const uint2*>(sh + src_lane);
            uint2* d = reinterpret_cast<uint2*>(&v);
#pragma unroll
            for (int k = 0; k < (int)(sizeof(P3) / 8); k++) d[k] = sv[k];
            return v;
        };
        while (step < NST) {
            int kind, off = 0, i = 0;
            if (step < NS1) {
                if (in.mode == 1) { kind = 0; i = L - 1 - step; }
                else { kind = (step & 1) ? 1 : 0; i = L - 1 - (step >> 1); }
            } else if (in.mode == 1) { kind = 4; off = (TPW / 2) >> (step - NS1); }
            else if (step < NS1 + LT) { kind = 2; off = (TPW / 2) >> (step - NS1); }
            else if (step < NS1 + 2 * LT) { kind = 3; off = 1 << (step - NS1 - LT); }
            else {
                kind = 4; off = (TPW / 2) >> (step - NS1 - 2 * LT);
                if (!mid_done) {   // between scan and the last tree: publish runW = S_0, drop group 0 from the tree
                    if (g == 0) { st_p3(o, SL::ld(slab, RUN, lane)); SL::st(slab, RUN, lane, p3_zero<FS>()); }
                    mid_done = true;
                }
            }
            const bool exch = kind >= 2;
            if (exch && det == 0) sh_store(SL::ld(slab, kind == 2 ? WACC : RUN, lane));
            if (exch) GH_WAVE_SYNC();
            const bool to_wacc = kind == 1 || kind == 2;
            const int dst = to_wacc ? WACC : RUN;
            bool active;
            if (kind == 0) active = live && item0 + (uint32_t)g + (uint32_t)TPW * (uint32_t)i < in.count;
            else if (kind == 1) active = live;
            else active = live && (kind == 3 ? g + off < TPW : g < off);
            if (det > 0) active = mydet;
            auto load_q = [&]() -> P3 {   // the step's second operand; read again below for the lanes whose sum is one of the operands
                P3 q = p3_zero<FS>();
                if (det == 1 || det == 3) {
                    q.x = ld_c(salts + salt_id, 0);
                    q.y = ld_c(salts + salt_id, 1);
                    if (det == 3) q.y = FS::neg(q.y);
                    q.z = FS::one();
                } else if (kind == 0) {
                    const uint32_t k = item0 + (uint32_t)g + (uint32_t)TPW * (uint32_t)i;
                    if (live && k < in.count) {
                        const Proj<C>* pt = in.base + ((size_t)w * in.count + k) * in.stride + in.offset;
                        q.x = ld_c(pt, 0); q.y = ld_c(pt, 1); q.z = ld_c(pt, 2);
                    }
                } else if (kind == 1) {
                    q = SL::ld(slab, RUN, lane);
                } else {
                    if (live && (kind == 3 ? g + off < TPW : g < off)) q = sh_load(lane + off * LANES);
                }
                return q;
            };
            const int src = det >= 2 ? TMP : dst;
            bool same, pz, qz;
            P3 r;
            {
                const P3 q = load_q();
                const P3 p = SL::ld(slab, src, lane);
                r = p3_add_raw<FS>(p, q, same, pz, qz);
            }
            if (__any((pz || qz) && active)) {   // p + infinity = p, infinity + q = q
                const P3 q = load_q();
                const P3 p = SL::ld(slab, src, lane);
                uint32_t* rw = reinterpret_cast<uint32_t*>(&r);
                const uint32_t* pw = reinterpret_cast<const uint32_t*>(&p);
                const uint32_t* qw = reinterpret_cast<const uint32_t*>(&q);
#pragma unroll
                for (int k = 0; k < SL::NW; k++) rw[k] = pz ? qw[k] : (qz ? pw[k] : rw[k]);
            }
            if (exch) GH_WAVE_SYNC();
            same = same && active;
            if (det == 0) {
                const bool any_same = __any(same) != 0;
                if (active && !same) SL::st(slab, dst, lane, r);
                if (any_same) {
                    mydet = same;
                    // salt with x != p.x / p.z (all lanes run the product: the group shuffles need their partners)
                    const P3 p = SL::ld(slab, src, lane);
                    const bool s0_hits = FS::eq(FS::mul(ld_c(salts, 0), p.z), p.x);
                    if (same) salt_id = s0_hits ? 1 : 0;
                    det = 1;
                } else {
                    step++;
                }
            } else {
                if (mydet) SL::st(slab, det < 3 ? TMP : dst, lane, r);
                if (det == 3) { det = 0; mydet = false; step++; } else det++;
            }
        }
        if (g == 0) {
            if (in.mode == 1) {
                st_p3(o, SL::ld(slab, RUN, lane));
            } else {
                st_p3(o + 1, SL::ld(slab, WACC, lane));
                st_p3(o + 2, SL::ld(slab, RUN, lane));
            }
        }
    }
}

}  // namespace gh
