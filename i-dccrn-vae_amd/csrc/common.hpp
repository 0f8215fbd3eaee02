// Shared device helpers for the I-DCCRN-VAE MI355X (gfx950) kernels.
//
// Activation layout used by every kernel in this library ("planar-J"):
//   act[ri][C][F][Jp]   fp32, ri = 0 real / 1 imag plane
//   column j = b * Tp + tp,  Tp = T_stft + 1,  tp = t + 1
//   tp == 0 is a zero guard column in front of every utterance (it provides the causal
//   x[t-1] = 0 tap without a branch), columns tp > T_valid are zero as well.
//   Jp (row stride) = J rounded up to 4; buffers carry IDV_SLACK floats in front and behind.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#define IDV_SLACK 256

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define IDV_OK 0
#define IDV_EINVAL (-1)
#define IDV_ELAUNCH (-2)

static inline int idv_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? IDV_OK : IDV_ELAUNCH;
}

// Allow `Kernel` more than 64 KB of dynamic LDS, once per kernel and device: setting the attribute on every launch is host time, a lot
// of it under a profiler.  smem must be a constant of the kernel (it is: every caller derives it from the template arguments).  The
// kernel is a template ARGUMENT, not a function argument: the instantiations of one kernel template share one pointer type, and a flag
// per type would skip all of them but the first.  Two threads that both find the flag clear both set the same value.
template <auto Kernel>
int idv_dyn_smem_once(size_t smem) {
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return IDV_ELAUNCH;
    if (smem > 64 * 1024 && !attr_set[dev].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return IDV_ELAUNCH;
        attr_set[dev].store(true, std::memory_order_release);
    }
    return IDV_OK;
}

// Argument checks of the latent entries (reduce.hip, backward.hip): a channel group [off, off + zdim) lies inside the latent's H
// channels; a guard column stands in front of the T frames and every utterance lies inside the pitch.
static inline bool idv_group_ok(int off, int zdim, int H) { return off >= 0 && off <= H - zdim; }
static inline bool idv_planar_ok(int B, int T, int Tp, int Jp) { return Tp >= T + 1 && (long long)Jp >= (long long)B * Tp; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// gate non-linearities on the hardware exp2 / rcp (about 1 ulp each): absolute error ~1e-7, which is what the
// LSTM cell needs; tanh(x) = 2 sigmoid(2x) - 1.  They sit on the per-step critical path of the recurrence.
__device__ __forceinline__ float sigmoidf_(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
__device__ __forceinline__ float tanhf_(float x) {
    return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.88539008177792681f * x)) - 1.0f;
}

// Train-mode moment sums with less atomic contention: the conv epilogues add their per-wave partials to one of `rep` replicas
// [rep][C][5] of the sums (chosen by workgroup index) instead of all to the same C x 5 doubles -- at 32 or 64 channels and
// ~10^4 workgroups the same-address atomics cost more than the contraction (enc1, B = 32: 4.1 ms against 1.65) -- and this
// kernel folds the replicas into stats[C][5] (+=, fixed order).  elementwise.hip
int idv_launch_stats_collapse(const double* work, int rep, int n, double* stats, hipStream_t st);
// Zero the guard columns tp == 0 and tp > T of every utterance in `planes` planar rows of pitch Jp (the layout invariant above).
// backward.hip
void idv_launch_zero_guard_cols(float* act, int planes, int B, int T, int Tp, int Jp, hipStream_t st);
// one more launch of a time-Winograd kernel with two co tiles per workgroup (the count behind idv_tw_pair_launches).  cgemm_tw.hip
void idv_tw_pair_note_launch();

