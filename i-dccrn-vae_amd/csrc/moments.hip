// Per-bin mean and variance of the STFT of a corpus, accumulated batch by batch on the device: dataset/stats.py SpecMoments (DESIGN.md
// 3.9; what the reference's dataset/cal_mean_std.py computes from every frame of the corpus held in host memory).
//
// Input: the planar spectrum spec[rows = 2F][Jp] the DFT GEMM writes (real rows, then imaginary rows; frame t of utterance b in column
// b*Tp + t + 1).  Only the valid columns count: t < T_b = min(Tmax, 1 + lens[b]/hop); guard columns and the frames past a row's end
// are skipped, not counted as zeros.
//
//   (a) tile_kernel    grid (column chunks of MO_CH, rows): the workgroup's valid values stay in registers; pass 1 their count and
//                      sum -> the tile's own mean, pass 2 the sum of squared deviations from it (M2).  With a DC offset the mean of
//                      bin 0 is ~100 and its std < 1: a one-pass sum / sum of squares would cancel, this does not.
//   (b) merge_kernel   one workgroup, one thread per row: the tiles' (n, mean, M2) are folded in increasing chunk order by Chan's
//                      formula  n = na + nb, d = mb - ma, mean = ma + d nb/n, M2 = M2a + M2b + d^2 na nb/n  and then into the
//                      persistent state[1 + 2*rows] = (n, mean[rows], M2[rows]), all double.
// Every sum has a fixed order (xor butterfly within a wave, waves and chunks in increasing order) and there is no atomic: the same
// sequence of calls gives the same bits.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int MO_CH = 2048, MO_PER = MO_CH / 256;          // columns per tile, per thread

__global__ __launch_bounds__(256) void tile_kernel(const float* __restrict__ spec, const int* __restrict__ lens, int B, int hop, int Tmax,
                                                   int Tp, int Jp, int rows, int nch, double* __restrict__ part) {
    __shared__ double sh[4];
    const int r = blockIdx.y, ch = blockIdx.x;
    const float* row = spec + (size_t)r * Jp;
    const int J = B * Tp;
    float v[MO_PER];
    bool ok[MO_PER];
    double s = 0, cnt = 0;
#pragma unroll
    for (int q = 0; q < MO_PER; ++q) {
        const int col = ch * MO_CH + q * 256 + threadIdx.x;
        ok[q] = false;
        v[q] = 0.f;
        if (col < J) {
            const int b = col / Tp, t = col - b * Tp - 1;
            int Tb = Tmax;
            if (lens) {
                const int L = max(lens[b], 0);
                Tb = min(Tmax, 1 + L / hop);
            }
            if (t >= 0 && t < Tb) {
                ok[q] = true;
                v[q] = row[col];
                s += (double)v[q];
                cnt += 1.0;
            }
        }
    }
    cnt = waves_sum<4>(cnt, sh);
    s = waves_sum<4>(s, sh);
    const double mean = cnt > 0 ? s / cnt : 0.0;
    double m2 = 0;
#pragma unroll
    for (int q = 0; q < MO_PER; ++q)
        if (ok[q]) {
            const double d = (double)v[q] - mean;
            m2 += d * d;
        }
    m2 = waves_sum<4>(m2, sh);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)ch * rows + r) * 3;
        o[0] = cnt;
        o[1] = mean;
        o[2] = m2;
    }
}

__device__ __forceinline__ void chan(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
    if (nb == 0) return;
    if (na == 0) {
        na = nb;
        ma = mb;
        Ma = Mb;
        return;
    }
    const double n = na + nb, d = mb - ma;
    ma += d * (nb / n);
    Ma += Mb + d * d * (na * (nb / n));
    na = n;
}

// one workgroup; part == nullptr: `other` is a state to merge (idv_spec_moments_merge)
__global__ __launch_bounds__(1024) void merge_kernel(const double* __restrict__ part, int nch, const double* __restrict__ other, int rows,
                                                     double* __restrict__ state) {
    const double n_old = state[0];
    double n_new = n_old;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        double na = n_old, ma = state[1 + r], Ma = state[1 + rows + r];
        if (part) {
            for (int c = 0; c < nch; ++c) {
                const double* o = part + ((size_t)c * rows + r) * 3;
                chan(na, ma, Ma, o[0], o[1], o[2]);
            }
        } else {
            chan(na, ma, Ma, other[0], other[1 + r], other[1 + rows + r]);
        }
        state[1 + r] = ma;
        state[1 + rows + r] = Ma;
        n_new = na;                                        // the same for every row: the count of valid columns
    }
    __syncthreads();                                       // every thread has read state[0]
    if (threadIdx.x == 0) state[0] = n_new;
}

}  // namespace

extern "C" long long idv_spec_moments_work_bytes(int rows, int B, int Tp) {
    if (rows <= 0 || B <= 0 || Tp <= 1 || (long long)B * Tp > 2147483647LL - MO_CH) return -1;
    const long long nch = ((long long)B * Tp + MO_CH - 1) / MO_CH;
    return nch * rows * 3 * (long long)sizeof(double);
}

extern "C" int idv_spec_moments_update(const float* spec, const int* lens, int B, int hop, int Tmax, int Tp, int Jp, int rows,
                                       double* state, void* work, long long work_bytes, void* stream) {
    const long long need = idv_spec_moments_work_bytes(rows, B, Tp);
    if (!spec || !state || !work || need < 0 || work_bytes < need || hop <= 0 || Tmax < 1 || Tp < Tmax + 1 || rows > 65535 ||
        (long long)Jp < (long long)B * Tp || ((uintptr_t)work & 7) || ((uintptr_t)state & 7))
        return IDV_EINVAL;
    const int nch = (B * Tp + MO_CH - 1) / MO_CH;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tile_kernel, dim3(nch, rows), dim3(256), 0, st, spec, lens, B, hop, Tmax, Tp, Jp, rows, nch, (double*)work);
    hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(1024), 0, st, (const double*)work, nch, (const double*)nullptr, rows, state);
    return idv_launch_status();
}

extern "C" int idv_spec_moments_merge(double* state, const double* other, int rows, void* stream) {
    if (!state || !other || state == other || rows <= 0 || ((uintptr_t)state & 7) || ((uintptr_t)other & 7)) return IDV_EINVAL;
    hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)nullptr, 0, other, rows, state);
    return idv_launch_status();
}
