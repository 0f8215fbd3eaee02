// Silence trimming for a padded batch of signals of different lengths: inference.trim / trim_list and the trimmed segment index of
// dataset/dataload.py.  The definition is librosa.effects.trim of librosa 0.10 with ref = np.max:
//
//   T_b = 1 + n_b / hop frames; frame t covers samples [t hop - frame/2, t hop + frame/2) of the row, zeros outside [0, n_b);
//   P[t] = mean of the squares over the frame;  db[t] = 10 log10(max(1e-10, P[t])) - 10 log10(max(1e-10, max_t P[t]));
//   t0 / t1 the first / last frame with db[t] > -top_db:  start = t0 hop,  end = min(n_b, (t1 + 1) hop);  none: (0, 0).
//
//   (a) block_energy_kernel  one wave per hop-sample block k of a row: E[b][k] = sum of the squares of x[b][k hop .. min(n_b, (k + 1) hop))
//                            in double (the square of a float32 is exact in double).  Every sample is read once, 16 bytes per lane.
//   (b) row_scan_kernel      one workgroup per row: P[t] = (E[t - r/2] + ... + E[t + r/2 - 1]) / frame with r = frame / hop, blocks
//                            outside the row counting as zero; the row maximum, the comparison above in double, first and last frame.
//   (c) gather_kernel        y[b][i] = x[b][start_b + i] for i < end_b - start_b, zeros behind, bounds read on the device.
//
// A block's sum is taken in the fixed order of rows.hpp (the block is the window).  Where a row's base is not 16-byte aligned (ldx is
// arbitrary) the lanes still load ALIGNED 16-byte quads, and a lane takes the first 1 .. 3 samples of its quad from the lane below
// (the block's first samples and its ragged end are scalar loads; a sample that does not exist enters as +0, which changes no sum).
// So E, P and the bounds of a row do not depend on B, on the other rows, on what lies at or past n_b (it is never read) or on the row
// pitch.  No atomics.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

#include <cmath>

namespace {

constexpr int TR_MAX_BLOCKS = 64;             // frame / hop

// the aligned quad j of a block: samples h + 4 j .. h + 4 j + 3 of the block's cnt samples (j = -1: the h samples before the first
// aligned address); one 16-byte load where all four exist, guarded scalar loads otherwise
__device__ __forceinline__ float4 load_quad(const float* __restrict__ blk, int h, int j, int cnt) {
    const int p0 = h + 4 * j;
    if (p0 >= 0 && p0 + 3 < cnt) return *reinterpret_cast<const float4*>(blk + p0);
    float4 v;
    v.x = (p0 >= 0 && p0 < cnt) ? blk[p0] : 0.f;
    v.y = (p0 + 1 >= 0 && p0 + 1 < cnt) ? blk[p0 + 1] : 0.f;
    v.z = (p0 + 2 >= 0 && p0 + 2 < cnt) ? blk[p0 + 2] : 0.f;
    v.w = (p0 + 3 >= 0 && p0 + 3 < cnt) ? blk[p0 + 3] : 0.f;
    return v;
}

__device__ __forceinline__ double add_squares(double acc, float a, float b, float c, float d) {
    acc += (double)a * (double)a;
    acc += (double)b * (double)b;
    acc += (double)c * (double)c;
    acc += (double)d * (double)d;
    return acc;
}

// H = number of samples in front of the block's first 16-byte aligned address (0 .. 3)
template <int H>
__device__ __forceinline__ double block_energy(const float* __restrict__ blk, int cnt, int lane) {
    const int nquad = (cnt + 3) >> 2;                      // logical quads, the last one may be short
    double acc = 0;
    float4 below = make_float4(0.f, 0.f, 0.f, 0.f);        // lane 0: the aligned quad in front of its logical one
    if (H > 0 && lane == 0) below = load_quad(blk, H, -1, cnt);
    for (int q0 = 0; q0 < nquad; q0 += 64) {               // wave-uniform trip count
        const float4 a = load_quad(blk, H, q0 + lane, cnt);
        if (H == 0) {
            acc = add_squares(acc, a.x, a.y, a.z, a.w);
            continue;
        }
        float4 p = a;                                      // aligned quad q - 1: the lane below, lane 0 from the pass before
        p.y = __shfl_up(a.y, 1, 64);
        p.z = __shfl_up(a.z, 1, 64);
        p.w = __shfl_up(a.w, 1, 64);
        if (lane == 0) p = below;
        below.y = __shfl(a.y, 63, 64);
        below.z = __shfl(a.z, 63, 64);
        below.w = __shfl(a.w, 63, 64);
        if (H == 1) acc = add_squares(acc, p.w, a.x, a.y, a.z);
        if (H == 2) acc = add_squares(acc, p.z, p.w, a.x, a.y);
        if (H == 3) acc = add_squares(acc, p.y, p.z, p.w, a.x);
    }
    return wave_sum_d(acc);
}

__global__ __launch_bounds__(256) void block_energy_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lens, int Lmax,
                                                           int hop, int nblk, double* __restrict__ E) {
    const int b = blockIdx.y;
    Window w = wave_window();
    if (w.k >= nblk) return;
    double e = 0;
    if (w.cut(hop, row_len(lens, b, Lmax))) {              // wave-uniform
        const float* blk = x + (size_t)b * ldx + w.w0;
        const int h = (int)((4 - (((uintptr_t)blk >> 2) & 3)) & 3);
        e = h == 0 ? block_energy<0>(blk, w.cnt, w.lane)
          : h == 1 ? block_energy<1>(blk, w.cnt, w.lane)
          : h == 2 ? block_energy<2>(blk, w.cnt, w.lane)
                   : block_energy<3>(blk, w.cnt, w.lane);
    }
    if (w.lane == 0) E[(size_t)b * nblk + w.k] = e;
}

// P[t]: the r blocks around frame t in increasing order (those outside the row are zeros and left out), over the frame length
__device__ __forceinline__ double frame_power(const double* __restrict__ Er, int nb, int t, int r, int frame) {
    double s = 0;
    const int k0 = t - r / 2;
    for (int k = max(k0, 0); k < min(k0 + r, nb); ++k) s += Er[k];
    return s / (double)frame;
}

__global__ __launch_bounds__(256) void row_scan_kernel(const double* __restrict__ E, const int* __restrict__ lens, int Lmax, int frame, int hop,
                                                       int nblk, double top_db, int* __restrict__ bounds, double* __restrict__ power,
                                                       long long ldp) {
    __shared__ double shd[256];
    __shared__ int2 shb[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = row_len(lens, b, Lmax);
    const int T = 1 + n / hop, nb = (n + hop - 1) / hop, r = frame / hop;
    const double* Er = E + (size_t)b * nblk;
    double pmax = 0;
    for (int t = tid; t < T; t += 256) pmax = fmax(pmax, frame_power(Er, nb, t, r, frame));
    pmax = tree256(pmax, shd, tid, [](double a, double c) { return fmax(a, c); });
    const double ref_db = 10.0 * log10(fmax(1e-10, pmax));
    int t0 = 0x7fffffff, t1 = -1;
    const int Tall = 1 + Lmax / hop;
    for (int t = tid; t < Tall; t += 256) {
        double P = 0;
        if (t < T) {
            P = frame_power(Er, nb, t, r, frame);
            const double db = 10.0 * log10(fmax(1e-10, P)) - ref_db;
            if (db > -top_db) {
                t0 = min(t0, t);
                t1 = max(t1, t);
            }
        } else if (!power) {
            break;
        }
        if (power) power[(size_t)b * ldp + t] = P;
    }
    // (first, last): the min and the max in one tree
    const int2 span = tree256(make_int2(t0, t1), shb, tid, [](int2 a, int2 c) { return make_int2(min(a.x, c.x), max(a.y, c.y)); });
    if (tid == 0) {
        t0 = span.x;
        t1 = span.y;
        const bool any = t1 >= 0;
        bounds[2 * b] = any ? t0 * hop : 0;
        bounds[2 * b + 1] = any ? (int)min((long long)n, (long long)(t1 + 1) * hop) : 0;
    }
}

__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ bounds, int Lout,
                                                     float* __restrict__ y, long long ldy) {
    const int b = blockIdx.y;
    const int start = bounds[2 * b], cnt = max(0, bounds[2 * b + 1] - start);
    const float* src = x + (size_t)b * ldx + start;
    float* dst = y + (size_t)b * ldy;
    const long long i0 = 4LL * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= Lout) return;
    const bool aligned = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
    if (aligned && i0 + 3 < Lout) {
        float4 v;
        if (i0 + 3 < cnt) {
            v = *reinterpret_cast<const float4*>(src + i0);
        } else {
            v.x = i0 < cnt ? src[i0] : 0.f;
            v.y = i0 + 1 < cnt ? src[i0 + 1] : 0.f;
            v.z = i0 + 2 < cnt ? src[i0 + 2] : 0.f;
            v.w = 0.f;
        }
        *reinterpret_cast<float4*>(dst + i0) = v;
        return;
    }
    for (long long i = i0; i < min(i0 + 4, (long long)Lout); ++i) dst[i] = i < cnt ? src[i] : 0.f;
}

}  // namespace

// hop > 0 and hop % 4 == 0 is the window_work_bytes condition win >= 4
extern "C" long long idv_trim_work_bytes(int B, int L, int hop) { return window_work_bytes(B, L, hop, 1); }

extern "C" int idv_trim_bounds(const float* x, long long ldx, const int* lens, int B, int L, int frame, int hop, double top_db, void* work,
                               long long work_bytes, int* bounds, double* power, long long ldp, void* stream) {
    const long long need = idv_trim_work_bytes(B, L, hop);
    if (!x || !work || !bounds || need < 0 || work_bytes < need || ldx < L || !aligned_to(8, {work})) return IDV_EINVAL;
    if (frame <= 0 || frame % (2LL * hop) != 0 || frame / hop > TR_MAX_BLOCKS) return IDV_EINVAL;
    if (!(top_db > 0) || !std::isfinite(top_db)) return IDV_EINVAL;
    if (power && (ldp < 1 + L / hop || !aligned_to(8, {power}))) return IDV_EINVAL;
    const int nblk = (int)(((long long)L + hop - 1) / hop);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(block_energy_kernel, dim3((nblk + 3) / 4, B), dim3(256), 0, st, x, ldx, lens, L, hop, nblk, (double*)work);
    hipLaunchKernelGGL(row_scan_kernel, dim3(B), dim3(256), 0, st, (const double*)work, lens, L, frame, hop, nblk, top_db, bounds, power, ldp);
    return idv_launch_status();
}

extern "C" int idv_trim_gather(const float* x, long long ldx, const int* bounds, int B, int Lout, float* y, long long ldy, void* stream) {
    if (!x || !bounds || !y || !row_limits_ok(B, Lout) || ldy < Lout) return IDV_EINVAL;
    const unsigned gx = (unsigned)(((long long)Lout + 1023) / 1024);
    hipLaunchKernelGGL(gather_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, ldx, bounds, Lout, y, ldy);
    return idv_launch_status();
}
