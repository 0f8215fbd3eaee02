// Shared pieces of the kernels that work on rows of samples or frames of different lengths: trim.hip, mix.hip, assemble.hip,
// reverb.hip, resample.hip, stoi.hip, sdr.hip, bss.hip, moments.hip, latent.hip.
//
// THE FIXED ORDER of a sum over the samples of a row, which trim.hip, mix.hip and assemble.hip share and tests/rows_ref.py restates in
// numpy (tests/test_gpu_rows_order.py holds the kernels to it bit for bit):
//   a row is cut into windows of win samples (a multiple of 4), one wave per window;
//   sample i of a window belongs to quad i / 4, quad q to lane q % 64;
//   a lane adds its quads in increasing q, the four terms of a quad in increasing i (double; the square of a float32 is exact);
//   the 64 lanes meet in an xor butterfly, v += v[lane ^ o] for o = 32 .. 1 (wave_sum_d; maxima alike in wave_max_d);
//   a row adds its windows k = t, t + 256, ... in thread t, and the 256 threads meet in an LDS tree, sh[t] += sh[t + o] for
//   t < o, o = 128 .. 1 (tree256).
// A sample that does not exist enters as +0, which changes no sum and no maximum of absolute values.  So the order follows from the
// sample's index in its window and the window's index in its row alone: a row's bits do not depend on the batch, on the other rows, on
// the row pitch, on the alignment of its base or on what lies behind its end.  No atomics.
#pragma once
#include "common.hpp"

#include <initializer_list>

// internal linkage like the kernels that use these (every unit keeps its code in an unnamed namespace, where quad_t hides the C
// library's type of that name)
namespace {

constexpr int ROWS_MAX_LEN = 1 << 27;         // samples per row
constexpr int ROWS_MAX_ROWS = 65535;          // rows of one call (grid.y)

// ---- wave reductions: the xor butterfly of wave_sum
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- workgroup reductions
// the 256 threads' values folded by op in an LDS tree (the same order whatever the values), in every thread.  sh: 256 values that no
// thread still reads (block_sum / block_max put a barrier in front for back-to-back use of one array).
template <typename T, typename Op>
__device__ __forceinline__ T tree256(T v, T* sh, int tid, Op op) {
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const T up = sh[tid + o];
            sh[tid] = op(sh[tid], up);
        }
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ double block_sum(double v, double* sh, int tid) {
    __syncthreads();
    return tree256(v, sh, tid, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ double block_max(double v, double* sh, int tid) {
    __syncthreads();
    return tree256(v, sh, tid, [](double a, double b) { return fmax(a, b); });
}

// the sum over a workgroup of NW waves: the butterfly within every wave, then the waves left to right, ((w0 + w1) + w2) + ..., in
// every thread.  sh: NW doubles, free again after the call.  LEAD0: the fold starts from 0 in front of w0, as the 16-wave form of
// stoi.hip always has.  0 + w0 differs from w0 only for w0 = -0, which no partial is (every accumulator starts at +0, and +0 + -0 =
// +0), but dropping the addition changes the code of rmse_kernel, and that trial did not stay inside its speed window
// (profiles/rows/code_diff.md).
template <int NW, bool LEAD0 = false>
__device__ __forceinline__ double waves_sum(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = LEAD0 ? 0.0 + sh[0] : sh[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) s += sh[q];
    return s;
}

// ---- quad access
// four floats at any 4-byte aligned address, one 16-byte load or store
struct __attribute__((packed, aligned(4))) quad_t {
    float x, y, z, w;
};

// samples p .. p + 3 of a row's cnt samples; those that do not exist are +0
__device__ __forceinline__ float4 load4(const float* __restrict__ x, int p, int cnt) {
    float4 r;
    if (p + 3 < cnt) {
        const quad_t q = *reinterpret_cast<const quad_t*>(x + p);
        return make_float4(q.x, q.y, q.z, q.w);
    }
    r.x = p < cnt ? x[p] : 0.f;
    r.y = p + 1 < cnt ? x[p + 1] : 0.f;
    r.z = p + 2 < cnt ? x[p + 2] : 0.f;
    r.w = 0.f;
    return r;
}

// positions p .. p + 3 of a row of n positions <- v; the last quad of a row may be short
__device__ __forceinline__ void store4(float* __restrict__ y, int p, int n, float4 v) {
    if (p + 3 < n) {
        *reinterpret_cast<quad_t*>(y + p) = quad_t{v.x, v.y, v.z, v.w};
        return;
    }
    const float t[4] = {v.x, v.y, v.z, v.w};
    for (int e = 0; p + e < n; ++e) y[p + e] = t[e];
}

__device__ __forceinline__ void acc_sq(double& s, double& mx, float a) {
    const double d = (double)a;
    s += d * d;
    mx = fmax(mx, fabs(d));
}

// ---- row geometry
// the samples of row b: lens[b] (lens == NULL: L) clamped to 0 .. L
__device__ __forceinline__ int row_len(const int* __restrict__ lens, int b, int L) { return max(0, min(lens ? lens[b] : L, L)); }

// row b of a pool (off: its int64 sample offsets) or of a padded batch of pitch ld (off == NULL)
__device__ __forceinline__ const float* row_base(const float* __restrict__ base, const long long* __restrict__ off, long long ld, int b) {
    return base + (off ? off[b] : (long long)b * ld);
}

// one wave per window, four to a workgroup: wave w of workgroup x takes window k = 4 x + w.  A kernel leaves with k >= nwin before it
// reads anything of its row; then cut(win, n): samples w0 .. w0 + cnt - 1 of the row's n, the lanes take the quads q = lane,
// lane + 64, ... < nquad.  false (wave-uniform): the window starts at or past n and has no samples.
struct Window {
    int k, lane, w0, cnt, nquad;
    __device__ __forceinline__ bool cut(int win, int n) {
        const long long s0 = (long long)k * win;
        w0 = (int)s0;
        cnt = min(win, n - w0);
        nquad = (cnt + 3) >> 2;
        return s0 < n;
    }
};
__device__ __forceinline__ Window wave_window() {
    return Window{(int)(blockIdx.x * 4 + (threadIdx.x >> 6)), (int)(threadIdx.x & 63), 0, 0, 0};
}

// ---- host side
// the limits every entry of this family puts on a batch: grid.y and an int sample index with room to spare
static inline bool row_limits_ok(long long rows, long long L) { return rows >= 1 && rows <= ROWS_MAX_ROWS && L >= 1 && L <= ROWS_MAX_LEN; }

// every pointer (NULL included) a multiple of `bytes`, a power of two
static inline bool aligned_to(uintptr_t bytes, std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((uintptr_t)p & (bytes - 1)) return false;
    return true;
}

// bytes of `fields` doubles per win-sample window of `rows` rows of L samples; -1: a batch or a window that is not supported
static inline long long window_work_bytes(int rows, int L, int win, int fields) {
    if (!row_limits_ok(rows, L) || win < 4 || win > ROWS_MAX_LEN || win % 4 != 0) return -1;
    return (long long)rows * (((long long)L + win - 1) / win) * fields * (long long)sizeof(double);
}

}  // namespace
