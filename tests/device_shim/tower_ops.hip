// tower_ops.hip -- the lane-split field forms of the G2 kernels (F2S, F3S of ginger-lib_amd/csrc/msm_kernels.h), the one-lane
// form F1S of aff_kernels.h behind the same interface, and the out-of-line inverses of the table builder (dev_fp_inv, DevInv),
// one operation per launch, so that each can be compared with Python integers limb for limb (tests/test_gpu_tower_ops.py).
// F2S, F3S and the inverses are __device__ only: no host shim reaches them.
// Test infrastructure: built by the test into its own code object (hipcc --genco), never linked into the product, no ABI.
//
// Rows: every buffer holds one row of NL raw limbs per lane, row = global lane index.  Group g of wave w sits in lanes
// LANES g .. LANES g + LANES - 1 of that wave, as msm_accumulate_split_kernel maps its tasks; lane 63 of a triple wave has no
// group.  Lanes of groups >= n and the idle lane skip the operation (no early return) and write nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../ginger-lib_amd/csrc/msm_kernels.h"

using namespace gh;

enum TowerOp {
    OP_ADD = 0, OP_SUB, OP_DBL, OP_NEG, OP_MUL, OP_SQR, OP_MUL_SUB_MUL, OP_SUB_LAZY, OP_INV, OP_IS_ZERO, OP_EQ, OP_ONE, OP_SEL,
    OP_SWAP, OP_BCAST0, OP_BCAST1   // the last four: F2S only; F1S has no mul_sub_mul either (such a launch stores zeros)
};

// mode 0: every live group runs op(a, b, c, d) in the first pass.
// mode 1: even groups run op(a, b, c, d) in the first pass, odd groups op(b, a, d, c) in the second (a unary op takes its first
//         operand), so the DPP moves and the shuffles of one wave execute under two complementary partial EXEC masks, as they do
//         in the accumulation's while loop.  The loop is not unrolled: both sets of lanes run the same instructions.
template <class F>
__device__ __forceinline__ void tower_ops_body(int op, int mode, uint32_t n, const uint32_t* __restrict__ a,
                                               const uint32_t* __restrict__ b, const uint32_t* __restrict__ c,
                                               const uint32_t* __restrict__ d, uint32_t* __restrict__ out,
                                               uint32_t* __restrict__ flags) {
    constexpr uint32_t LANES = F::LANES, TPW = 64 / LANES;
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = row >> 6;
    const uint32_t g = wave * TPW + lane / LANES;
    const bool live = lane < TPW * LANES && g < n;                 // all lanes of a group agree
    const Fp* pa = reinterpret_cast<const Fp*>(a) + row;
    const Fp* pb = reinterpret_cast<const Fp*>(b) + row;
    const Fp* pc = reinterpret_cast<const Fp*>(c) + row;
    const Fp* pd = reinterpret_cast<const Fp*>(d) + row;
#pragma nounroll
    for (uint32_t pass = 0; pass < 2; pass++) {
        const bool take = live && (mode == 0 ? pass == 0 : (g & 1u) == pass);
        if (take) {
            const Fp x = ld_fp(pass ? pb : pa), y = ld_fp(pass ? pa : pb);
            Fp r = fp_zero();
            int flag = -1;
            switch (op) {
            case OP_ADD: r = F::add(x, y); break;
            case OP_SUB: r = F::sub(x, y); break;
            case OP_DBL: r = F::dbl(x); break;
            case OP_NEG: r = F::neg(x); break;
            case OP_MUL: r = F::mul(x, y); break;
            case OP_SQR: r = F::sqr(x); break;
            case OP_MUL_SUB_MUL:
                if constexpr (LANES > 1) r = F::mul_sub_mul(x, y, ld_fp(pass ? pd : pc), ld_fp(pass ? pc : pd));
                break;
            case OP_SUB_LAZY: r = F::sub_lazy(x, y); break;
            case OP_INV: r = F::inv(x); break;
            case OP_IS_ZERO: flag = F::is_zero(x) ? 1 : 0; break;
            case OP_EQ: flag = F::eq(x, y) ? 1 : 0; break;
            case OP_ONE: r = F::one(); break;
            default:
                if constexpr (LANES == 2) {
                    // sel is a per-lane select: the condition is bit 0 of this lane's row of c
                    if (op == OP_SEL) r = F::sel((ld_fp(pc).l[0] & 1u) != 0, x, y);
                    else if (op == OP_SWAP) r = F::swap(x);
                    else if (op == OP_BCAST0) r = F::template bcast<0>(x);
                    else if (op == OP_BCAST1) r = F::template bcast<1>(x);
                }
                break;
            }
            if (flag >= 0) flags[row] = (uint32_t)flag;
            else st_fp(reinterpret_cast<Fp*>(out) + row, r);
        }
    }
}

typedef F2S<P4, 13> TowerF2;
typedef F3S<P6, 11> TowerF3;

extern "C" __global__ void __launch_bounds__(256, TowerF2::WAVES)
tower_ops_f2s(int op, int mode, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
              uint32_t* out, uint32_t* flags) {
    tower_ops_body<TowerF2>(op, mode, n, a, b, c, d, out, flags);
}

extern "C" __global__ void __launch_bounds__(256, TowerF3::WAVES)
tower_ops_f3s(int op, int mode, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
              uint32_t* out, uint32_t* flags) {
    tower_ops_body<TowerF3>(op, mode, n, a, b, c, d, out, flags);
}

extern "C" __global__ void __launch_bounds__(256, F1S<P4>::WAVES)
tower_ops_f1s_p4(int op, int mode, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                 uint32_t* out, uint32_t* flags) {
    tower_ops_body<F1S<P4>>(op, mode, n, a, b, c, d, out, flags);
}

extern "C" __global__ void __launch_bounds__(256, F1S<P6>::WAVES)
tower_ops_f1s_p6(int op, int mode, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                 uint32_t* out, uint32_t* flags) {
    tower_ops_body<F1S<P6>>(op, mode, n, a, b, c, d, out, flags);
}

// ---- the inverses of msm_precompute_jac_kernel, with the template arguments precompute_bases gives them (C::F for the prime
//      fields, C::FC for the towers); one element per lane, rows of DEG x NL limbs
template <class P> __device__ __forceinline__ void dev_inv_fp_body(uint32_t n, const uint32_t* a, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st_fp(reinterpret_cast<Fp*>(out) + i, DevInv<F1<P, true>>::inv(ld_fp(reinterpret_cast<const Fp*>(a) + i)));
}
template <class FC> __device__ __forceinline__ void dev_inv_tower_body(uint32_t n, const uint32_t* a, uint32_t* out) {
    typedef typename FC::T T;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st_words(reinterpret_cast<T*>(out) + i, DevInv<FC>::inv(ld_words(reinterpret_cast<const T*>(a) + i)));
}
extern "C" __global__ void __launch_bounds__(256) dev_inv_p4(uint32_t n, const uint32_t* a, uint32_t* out) { dev_inv_fp_body<P4>(n, a, out); }
extern "C" __global__ void __launch_bounds__(256) dev_inv_p6(uint32_t n, const uint32_t* a, uint32_t* out) { dev_inv_fp_body<P6>(n, a, out); }
extern "C" __global__ void __launch_bounds__(64) dev_inv_fq2(uint32_t n, const uint32_t* a, uint32_t* out) {
    dev_inv_tower_body<Mnt4G2::FC>(n, a, out);
}
extern "C" __global__ void __launch_bounds__(64) dev_inv_fq3(uint32_t n, const uint32_t* a, uint32_t* out) {
    dev_inv_tower_body<Mnt6G2::FC>(n, a, out);
}
