// msm_reduce.hip -- the MSM's bucket reduction (ginger-lib_amd/csrc/msm_reduce_kernels.h: the G1 wave program in its 512- and
// 256-register builds, the lane-group program of Fq2 and Fq3) and msm_heavy_combine_kernel (msm_kernels.h), one host launcher
// per kernel build, so that each written-out copy of the wave program can be run on operands chosen for it and its output
// compared with a Python-integer model (tests/test_gpu_msm_reduce.py, tests/msm_reduce_ref.py).
// Test infrastructure: built by the test into build/libmsm_reduce_<curve>.so (hipcc -shared, one shared object per curve:
// -DRD_CURVE=0 mnt4753_g1, 1 mnt4753_g2, 2 mnt6753_g1, 3 mnt6753_g2; without the macro all four), never linked into the product.
//
// Every launcher takes plain values and device pointers, launches on the null stream with the grid, block and LDS size of
// msm_impl.h (reduce_level: per_input * n_inputs programs of 64 lanes, 64 points of LDS; launch_accumulate: n_heavy blocks),
// synchronises and returns the hipError_t (-1: this shared object does not hold the curve).  A WaveReduceIn travels as six
// host words: base, stride, offset, count, mode, valid.  The lane-group field of a G2 curve is the one msm_impl.h SplitFS
// chooses: F2S<P4, 13> at 32 groups per wave, F3S<P6, 11> at 16.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../ginger-lib_amd/csrc/msm_kernels.h"

using namespace gh;

#ifdef RD_CURVE
#define RD_HAS(k) (RD_CURVE == (k))
#else
#define RD_HAS(k) 1
#endif

static int finish() {
    hipError_t e = hipGetLastError();
    const hipError_t s = hipDeviceSynchronize();
    if (e == hipSuccess) e = s;
    return (int)e;
}
template <class C> static WaveReduceIn<C> wave_in(const uint64_t* v) {
    return WaveReduceIn<C>{(const Proj<C>*)(uintptr_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]};
}
template <class C, int WAVES>
static int wave_g1(const uint64_t* in0, const uint64_t* in1, const uint64_t* in2, uint32_t per_input, uint32_t n_inputs, uint32_t segs,
                   int L, const void* salts, void* out, uint32_t* slabs, const uint32_t* run_if) {
    msm_wave_reduce_kernel<C, WAVES><<<dim3(per_input * n_inputs), dim3(64), 64 * sizeof(Proj<C>)>>>(
        wave_in<C>(in0), wave_in<C>(in1), wave_in<C>(in2), per_input, n_inputs, segs, L, (const Aff<C>*)salts, (Proj<C>*)out, slabs, run_if);
    return finish();
}
template <class C, class FS, int TPW>
static int wave_g2(const uint64_t* in0, const uint64_t* in1, const uint64_t* in2, uint32_t per_input, uint32_t n_inputs, uint32_t segs,
                   int L, const void* salts, void* out, uint32_t* slabs) {
    msm_wave_reduce_split_kernel<C, FS, FS::LANES, TPW><<<dim3(per_input * n_inputs), dim3(64), 64 * sizeof(P3)>>>(
        wave_in<C>(in0), wave_in<C>(in1), wave_in<C>(in2), per_input, n_inputs, segs, L, (const Aff<C>*)salts, (Proj<C>*)out, slabs);
    return finish();
}
template <class C>
static int heavy(const void* partials, const uint32_t* order, const uint32_t* chunk_start, uint32_t n_heavy, void* buckets) {
    msm_heavy_combine_kernel<C><<<dim3(n_heavy), dim3(64), 64 * sizeof(Proj<C>)>>>((const Proj<C>*)partials, order, chunk_start,
                                                                                  (Proj<C>*)buckets);
    return finish();
}
template <class C, class T> static uint32_t size_of(int which) {
    switch (which) {
        case 0: return (uint32_t)sizeof(Aff<C>);
        case 1: return (uint32_t)sizeof(Proj<C>);
        case 2: return (uint32_t)WaveSlab<T>::WORDS;
        case 3: return (uint32_t)sizeof(P3);
    }
    return 0;
}

extern "C" {

// curve: 0 mnt4753_g1, 1 mnt4753_g2, 2 mnt6753_g1, 3 mnt6753_g2; which: 0 sizeof(Aff<C>), 1 sizeof(Proj<C>), 2 WaveSlab<T>::WORDS of
// the curve's program (T = Proj<C> on G1, P3 on G2), 3 sizeof(P3); 0: not in this shared object
uint32_t rd_sizeof(int curve, int which) {
#if RD_HAS(0)
    if (curve == 0) return size_of<Mnt4G1, Proj<Mnt4G1>>(which);
#endif
#if RD_HAS(1)
    if (curve == 1) return size_of<Mnt4G2, P3>(which);
#endif
#if RD_HAS(2)
    if (curve == 2) return size_of<Mnt6G1, Proj<Mnt6G1>>(which);
#endif
#if RD_HAS(3)
    if (curve == 3) return size_of<Mnt6G2, P3>(which);
#endif
    return 0;
}

// msm_wave_reduce_kernel<Mnt{4,6}G1, waves>: curve 4 | 6, waves 1 (512 registers) | 2 (256 registers)
int rd_wave_g1(int curve, int waves, const uint64_t* in0, const uint64_t* in1, const uint64_t* in2, uint32_t per_input, uint32_t n_inputs,
               uint32_t segs, int L, const void* salts, void* out, uint32_t* slabs, const uint32_t* run_if) {
#if RD_HAS(0)
    if (curve == 4 && waves == 1) return wave_g1<Mnt4G1, 1>(in0, in1, in2, per_input, n_inputs, segs, L, salts, out, slabs, run_if);
    if (curve == 4 && waves == 2) return wave_g1<Mnt4G1, 2>(in0, in1, in2, per_input, n_inputs, segs, L, salts, out, slabs, run_if);
#endif
#if RD_HAS(2)
    if (curve == 6 && waves == 1) return wave_g1<Mnt6G1, 1>(in0, in1, in2, per_input, n_inputs, segs, L, salts, out, slabs, run_if);
    if (curve == 6 && waves == 2) return wave_g1<Mnt6G1, 2>(in0, in1, in2, per_input, n_inputs, segs, L, salts, out, slabs, run_if);
#endif
    return -1;
}

// msm_wave_reduce_split_kernel: curve 4 (Fq2: the written-out loop, 32 groups) | 6 (Fq3: wave_reduce_program over GroupView, 16)
int rd_wave_g2(int curve, const uint64_t* in0, const uint64_t* in1, const uint64_t* in2, uint32_t per_input, uint32_t n_inputs,
               uint32_t segs, int L, const void* salts, void* out, uint32_t* slabs) {
#if RD_HAS(1)
    if (curve == 4) return wave_g2<Mnt4G2, F2S<P4, 13>, 32>(in0, in1, in2, per_input, n_inputs, segs, L, salts, out, slabs);
#endif
#if RD_HAS(3)
    if (curve == 6) return wave_g2<Mnt6G2, F3S<P6, 11>, 16>(in0, in1, in2, per_input, n_inputs, segs, L, salts, out, slabs);
#endif
    return -1;
}

// msm_heavy_combine_kernel<C>: curve as rd_sizeof
int rd_heavy_combine(int curve, const void* partials, const uint32_t* order, const uint32_t* chunk_start, uint32_t n_heavy, void* buckets) {
#if RD_HAS(0)
    if (curve == 0) return heavy<Mnt4G1>(partials, order, chunk_start, n_heavy, buckets);
#endif
#if RD_HAS(1)
    if (curve == 1) return heavy<Mnt4G2>(partials, order, chunk_start, n_heavy, buckets);
#endif
#if RD_HAS(2)
    if (curve == 2) return heavy<Mnt6G1>(partials, order, chunk_start, n_heavy, buckets);
#endif
#if RD_HAS(3)
    if (curve == 3) return heavy<Mnt6G2>(partials, order, chunk_start, n_heavy, buckets);
#endif
    return -1;
}

}  // extern "C"
