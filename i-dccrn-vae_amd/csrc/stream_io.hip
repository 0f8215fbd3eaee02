// Signal ends of streaming.StreamingDCCRN: framing from the carried input ring, the ring update, and the overlap-add with the
// carried overlap, the istft envelope and emission of the samples that became final.
//
// Index conventions (torch.stft / torch.istft, center=True, reflect padding; model/pvae_module.py:12-42): half = n_fft/2,
// left = (n_fft - win)/2.  Frame t holds original samples s = hop*t + left - half + i, i in [0, win); s < 0 reads x[-s], and
// at the end of the signal (L known) s >= L reads x[2(L-1) - s].  Output sample m sits at padded position P = m + half and
// collects frame t at window index P - hop*t - left.  The host-side schedule (streaming.StreamPlan) computes every range
// these kernels are given.
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

inline int grid_of(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

// frames[i][b*Tp + 1 + tl] for the k frames t0 .. t0+k-1; samples below n_prev come from ring[b][s mod R], the others from
// x[b][s - n_prev] (this push's input, row stride ldx)
__global__ void stream_frames_kernel(const float* __restrict__ ring, int R, const float* __restrict__ x, long long ldx, long long n_prev,
                                     long long L_end, int B, int n_fft, int win, int hop, long long t0, int k,
                                     float* __restrict__ frames, int Tp, int Jp) {
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long n = (long long)win * B * k;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int tl = (int)(e % k);
        const int b = (int)((e / k) % B);
        const int i = (int)(e / ((long long)k * B));
        long long s = (long long)hop * (t0 + tl) + left - half + i;
        if (s < 0) s = -s;
        if (L_end >= 0 && s >= L_end) s = 2 * (L_end - 1) - s;
        const float v = s >= n_prev ? x[(size_t)b * ldx + (size_t)(s - n_prev)] : ring[(size_t)b * R + (size_t)(s % R)];
        frames[(size_t)i * Jp + (size_t)b * Tp + 1 + tl] = v;
    }
}

__global__ void stream_ring_kernel(float* __restrict__ ring, int R, const float* __restrict__ x, long long ldx, int n_new, long long n_prev,
                                   long long s0, int B) {
    const long long cnt = n_prev + n_new - s0;
    const long long n = cnt * B;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(e / cnt);
        const long long s = s0 + e % cnt;
        ring[(size_t)b * R + (size_t)(s % R)] = x[(size_t)b * ldx + (size_t)(s - n_prev)];
    }
}

// padded positions P in [p_start, p_end): carried partial sum (positions below p_start + cin_len) plus the frames t0 ..
// t0+k-1 in increasing t; P - half < e1 is final and goes to y (times 1 / envelope as idv_make_dft computes it), the rest
// becomes the carry for positions from half + e1 on
__global__ void stream_ola_kernel(const float* __restrict__ frames, int Tp, int Jp, const float* __restrict__ cin, int cin_len,
                                  float* __restrict__ cout_, int cap, int B, int n_fft, int win, int hop, long long t0, int k,
                                  long long T_total, long long e0, long long e1, long long p_end, float* __restrict__ y, int ldy,
                                  long long y_off) {
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long p_start = half + e0, p_new = half + e1;
    const long long span = p_end - p_start;
    const long long n = span * B;
    const double two_pi = 6.283185307179586476925286766559;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(e / span);
        const long long P = p_start + e % span;
        float v = (P - p_start < cin_len) ? cin[(size_t)b * cap + (size_t)(P - p_start)] : 0.f;
        for (int tl = 0; tl < k; ++tl) {
            const long long i = P - (long long)hop * (t0 + tl) - left;
            if (i >= 0 && i < win) v += frames[(size_t)i * Jp + (size_t)b * Tp + 1 + tl];
        }
        if (P < p_new) {
            // frames whose window covers P: P - win < hop*t + left <= P (at most ceil(win/hop) of them, wherever the stream is)
            double env = 0.0;
            long long t_hi = (P - left) / hop;
            if (T_total >= 0 && t_hi > T_total - 1) t_hi = T_total - 1;
            long long t_lo = P - left - win >= 0 ? (P - left - win) / hop + 1 : 0;
            for (long long t = t_lo; t <= t_hi; ++t) {
                const long long i = P - (long long)hop * t - left;
                if (i >= 0 && i < win) {
                    const double wn = 0.5 - 0.5 * cos(two_pi * i / win);
                    env += wn * wn;
                }
            }
            const float inv = env > 1e-11 ? (float)(1.0 / env) : 0.f;
            y[(size_t)b * ldy + (size_t)(y_off + P - p_start)] = v * inv;
        } else {
            cout_[(size_t)b * cap + (size_t)(P - p_new)] = v;
        }
    }
}

}  // namespace

extern "C" int idv_stream_frames(const float* ring, int R, const float* x, long long ldx, int n_new, long long n_prev, long long L_end,
                                 int B, int n_fft, int win, int hop, long long t0, int k, float* frames, int Tp, int Jp, void* stream) {
    if (!ring || R <= 0 || (n_new > 0 && (!x || ldx < n_new)) || n_new < 0 || n_prev < 0 || B <= 0 || n_fft <= 0 || win <= 0 || win > n_fft ||
        hop <= 0 || t0 < 0 || k <= 0 || !frames || Tp < k + 1 || Jp < B * Tp)
        return IDV_EINVAL;
    // every sample read must be in the ring or in x
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long first = (long long)hop * t0 + left - half, last = (long long)hop * (t0 + k - 1) + left - half + win - 1;
    const long long lo_read = first < 0 ? 0 : first;
    const long long hi_read = (L_end >= 0 && last >= L_end) ? L_end - 1 : last;
    if (hi_read >= n_prev + n_new || (lo_read < n_prev && n_prev - lo_read > R) || (first < 0 && -first >= n_prev + n_new) ||
        (first < 0 && n_prev > R))
        return IDV_EINVAL;
    hipLaunchKernelGGL(stream_frames_kernel, dim3(grid_of((long long)win * B * k)), dim3(256), 0, (hipStream_t)stream, ring, R, x,
                       ldx, n_prev, L_end, B, n_fft, win, hop, t0, k, frames, Tp, Jp);
    return idv_launch_status();
}

extern "C" int idv_stream_ring(float* ring, int R, const float* x, long long ldx, int n_new, long long n_prev, int B, void* stream) {
    if (!ring || R <= 0 || n_new < 0 || (n_new > 0 && (!x || ldx < n_new)) || n_prev < 0 || B <= 0) return IDV_EINVAL;
    if (n_new == 0) return IDV_OK;
    const long long s0 = (n_prev + n_new - R > n_prev) ? n_prev + n_new - R : n_prev;
    hipLaunchKernelGGL(stream_ring_kernel, dim3(grid_of((n_prev + n_new - s0) * B)), dim3(256), 0, (hipStream_t)stream, ring, R, x,
                       ldx, n_new, n_prev, s0, B);
    return idv_launch_status();
}

extern "C" int idv_stream_ola(const float* frames, int Tp, int Jp, const float* carry_in, int carry_in_len, float* carry_out, int cap,
                              int B, int n_fft, int win, int hop, long long t0, int k, long long T_total, long long e0, long long e1,
                              long long p_end, float* y, int ldy, long long y_off, void* stream) {
    if ((k > 0 && !frames) || k < 0 || !carry_in || !carry_out || cap <= 0 || carry_in_len < 0 || carry_in_len > cap || B <= 0 ||
        n_fft <= 0 || win <= 0 || win > n_fft || hop <= 0 || t0 < 0 || e1 < e0 || e0 < 0 || (e1 > e0 && !y) || y_off < 0 ||
        (k > 0 && (Tp < k + 1 || Jp < B * Tp)))
        return IDV_EINVAL;
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long p_start = half + e0;
    if (p_end < half + e1 || p_end - p_start < carry_in_len || p_end - (half + e1) > cap || y_off + (e1 - e0) > ldy ||
        (k > 0 && (long long)hop * (t0 + k - 1) + left + win > p_end))
        return IDV_EINVAL;
    if (p_end <= p_start) return IDV_OK;
    hipLaunchKernelGGL(stream_ola_kernel, dim3(grid_of((p_end - p_start) * B)), dim3(256), 0, (hipStream_t)stream, frames, Tp, Jp,
                       carry_in, carry_in_len, carry_out, cap, B, n_fft, win, hop, t0, k, T_total, e0, e1, p_end, y, ldy, y_off);
    return idv_launch_status();
}
