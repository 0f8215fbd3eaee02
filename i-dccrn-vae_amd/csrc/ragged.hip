// Signal ends of a batch of utterances of different lengths (inference.enhance_* with `lengths`): STFT framing with the end
// mirror at each utterance's own length, and the ISTFT overlap-add over each utterance's own frames with the envelope of those
// frames.  Utterance b has lens[b] samples, T_b = 1 + lens[b]/hop frames and hop*(T_b - 1) output samples; the batch is laid out
// for Tmax = max_b T_b frames (Tp >= Tmax + 1 columns per utterance).  In a causal network frame t depends on frames <= t only, so
// nothing between these two kernels needs the lengths: the columns past T_b are written as zeros here and never read back there.
//
// Index conventions as in elementwise.hip / stream_io.hip (torch.stft / torch.istft, center=True, reflect padding): half =
// n_fft/2, left = (n_fft - win)/2; frame t holds samples s = hop*t + left - half + k, k in [0, win); s < 0 reads x[-s], s >= L
// reads x[2(L-1) - s].
#include "bf16_common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int RG_TT = 32;         // frames per block (as stft_frames_kernel)

// One block per (b, 32 frames): the signal segment of the block's valid frames is staged in LDS with both mirrors applied (the
// end mirror at L = lens[b]; no sample at or past L is read), then written out coalesced along j.  KIMG = false: planar
// frames[win][Jp] (idv_stft_frames); KIMG = true: the split-bf16 K-major image (idv_stft_frames_kimage).  Frames t >= T_b and
// the guard column are zeros.  ZPAD (idv_stft_frames_ragged_pad, pad_mode 1): the samples before 0 and at or past L are zeros instead
// of the mirror images (librosa.stft's pad_mode="constant"); any L >= 0 is then valid.
template <bool KIMG, bool ZPAD = false>
__global__ __launch_bounds__(256) void stft_frames_ragged_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lens,
                                                                 int n_fft, int win, int hop, int Tmax, float* __restrict__ frames,
                                                                 unsigned short* __restrict__ img, long long lo_off, int KO, int Tp,
                                                                 int Jp) {
    extern __shared__ float seg[];
    const int b = blockIdx.y, t0 = blockIdx.x * RG_TT;
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    long long L = lens[b];
    if (L > ldx) L = ldx;                                         // never past the row, whatever lens holds
    if (L < 0) L = 0;
    const int Tb = (int)min((long long)Tmax, 1 + L / hop);
    const int nt = min(RG_TT, Tmax - t0);                         // columns this block writes
    const int nv = max(0, min(nt, Tb - t0));                      // of which valid frames
    const int seglen = nv > 0 ? hop * (nv - 1) + win : 0;
    const long long s0 = (long long)hop * t0 + left - half;       // original-signal index of seg[0]
    for (int e = threadIdx.x; e < seglen; e += blockDim.x) {
        long long s = s0 + e;
        if constexpr (!ZPAD) {
            if (s < 0) s = -s;
            if (s >= L) s = 2LL * (L - 1) - s;
        }
        seg[e] = (s >= 0 && s < L) ? x[(size_t)b * ldx + s] : 0.f;
    }
    __syncthreads();
    const int tl = threadIdx.x & 31, kq = threadIdx.x >> 5;       // 32 frames x 8 k-lanes (k octets for the image)
    const bool live = tl < nv;
    if constexpr (!KIMG) {
        if (tl < nt) {
            const size_t col = (size_t)b * Tp + t0 + tl + 1;
            for (int k = kq; k < win; k += 8) frames[(size_t)k * Jp + col] = live ? seg[hop * tl + k] : 0.f;
        }
        if (blockIdx.x == 0)
            for (int k = threadIdx.x; k < win; k += blockDim.x) frames[(size_t)k * Jp + (size_t)b * Tp] = 0.f;
    } else {
        // 33 columns per block: the 32 frames and, in the first block of an utterance, its guard column
        for (int o = kq; o < KO; o += 8) {
            for (int pass = 0; pass < 2; ++pass) {
                const bool guard = pass == 1;
                if (guard && (blockIdx.x != 0 || tl != 0)) continue;
                if (!guard && tl >= nt) continue;
                const bool val = !guard && live;
                const size_t col = (size_t)b * Tp + (guard ? 0 : t0 + tl + 1);
                unsigned hw[4], lw[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int k0 = 8 * o + 2 * w;
                    const float x0 = (val && k0 < win) ? seg[hop * tl + k0] : 0.f;
                    const float x1 = (val && k0 + 1 < win) ? seg[hop * tl + k0 + 1] : 0.f;
                    const unsigned u0 = __builtin_bit_cast(unsigned, x0) & 0xffff0000u;
                    const unsigned u1 = __builtin_bit_cast(unsigned, x1) & 0xffff0000u;
                    hw[w] = (u0 >> 16) | u1;
                    lw[w] = pack_bf16(x0 - __builtin_bit_cast(float, u0), x1 - __builtin_bit_cast(float, u1));
                }
                unsigned short* d = img + ((size_t)o * Jp + col) * 8;
                *(uint4*)d = make_uint4(hw[0], hw[1], hw[2], hw[3]);
                *(uint4*)(d + lo_off) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
            }
        }
    }
}

// y[b][s] = (sum_{t < T_b} frames[k = s + half - left - hop*t][b*Tp + t + 1]) / (sum_{t < T_b} w[k]^2) for s < hop*(T_b - 1), 0 for
// the rest of the row.  The squared window sits in LDS in double; the envelope is summed in increasing t in double and inverted
// once, as idv_make_dft computes the table idv_istft_ola reads -- so a row equals what that kernel writes for T = T_b.
__global__ __launch_bounds__(256) void istft_ola_ragged_kernel(const float* __restrict__ frames, const int* __restrict__ lens, int len_div,
                                                               int B, int n_fft, int win, int hop, int Tmax, int Tp, int Jp,
                                                               float* __restrict__ y, long long ldy) {
    extern __shared__ double w2[];
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = threadIdx.x; k < win; k += blockDim.x) {
        const double wn = 0.5 - 0.5 * cos(two_pi * k / win);      // hann, periodic
        w2[k] = wn * wn;
    }
    __syncthreads();
    const int Lmax = hop * (Tmax - 1);
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long n = (long long)B * Lmax;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(idx / Lmax), s = (int)(idx % Lmax);
        long long L = lens[b / len_div];
        if (L < 0) L = 0;
        const int T = (int)min((long long)Tmax, 1 + L / hop);
        float out = 0.f;
        if (s < hop * (T - 1)) {
            const int p = s + half - left;                 // position relative to the window start of frame 0
            int t_hi = p / hop;
            if (t_hi > T - 1) t_hi = T - 1;
            int t_lo = (p - win + hop) / hop;              // smallest t with p - hop*t < win
            if (p - win + 1 <= 0) t_lo = 0;
            if (t_lo < 0) t_lo = 0;
            float acc = 0.f;
            double env = 0.0;
            for (int t = t_lo; t <= t_hi; ++t) {
                const int k = p - hop * t;
                if (k >= 0 && k < win) {
                    acc += frames[(size_t)k * Jp + (size_t)b * Tp + t + 1];
                    env += w2[k];
                }
            }
            out = acc * (env > 1e-11 ? (float)(1.0 / env) : 0.f);
        }
        y[(size_t)b * ldy + s] = out;
    }
}

inline int grid_for(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

inline bool frames_args_ok(const float* x, long long ldx, const int* lens, int B, int n_fft, int win, int hop, int Tmax, int Tp, int Jp,
                           bool zpad = false) {
    return x && lens && B > 0 && B <= 65535 && n_fft > 0 && win > 0 && win <= n_fft && hop > 0 && Tmax >= 1 &&
           ldx > (zpad ? 0 : n_fft / 2) && Tp >= Tmax + 1 && (long long)Jp >= (long long)B * Tp;
}

}  // namespace

extern "C" int idv_stft_frames_ragged(const float* x, long long ldx, const int* lens, int B, int n_fft, int win, int hop, int Tmax,
                                      float* frames, int Tp, int Jp, void* stream) {
    if (!frames || !frames_args_ok(x, ldx, lens, B, n_fft, win, hop, Tmax, Tp, Jp)) return IDV_EINVAL;
    const size_t smem = (size_t)(hop * (RG_TT - 1) + win) * sizeof(float);
    hipLaunchKernelGGL(stft_frames_ragged_kernel<false>, dim3((Tmax + RG_TT - 1) / RG_TT, B), dim3(256), smem, (hipStream_t)stream, x,
                       ldx, lens, n_fft, win, hop, Tmax, frames, (unsigned short*)nullptr, 0LL, 0, Tp, Jp);
    return idv_launch_status();
}

extern "C" int idv_stft_frames_ragged_pad(const float* x, long long ldx, const int* lens, int B, int n_fft, int win, int hop, int Tmax,
                                          int pad_mode, float* frames, int Tp, int Jp, void* stream) {
    if (pad_mode == IDV_PAD_REFLECT) return idv_stft_frames_ragged(x, ldx, lens, B, n_fft, win, hop, Tmax, frames, Tp, Jp, stream);
    if (pad_mode != IDV_PAD_CONSTANT || !frames || !frames_args_ok(x, ldx, lens, B, n_fft, win, hop, Tmax, Tp, Jp, true)) return IDV_EINVAL;
    const size_t smem = (size_t)(hop * (RG_TT - 1) + win) * sizeof(float);
    hipLaunchKernelGGL((stft_frames_ragged_kernel<false, true>), dim3((Tmax + RG_TT - 1) / RG_TT, B), dim3(256), smem, (hipStream_t)stream,
                       x, ldx, lens, n_fft, win, hop, Tmax, frames, (unsigned short*)nullptr, 0LL, 0, Tp, Jp);
    return idv_launch_status();
}

extern "C" int idv_stft_frames_kimage_ragged(const float* x, long long ldx, const int* lens, int B, int n_fft, int win, int hop, int Tmax,
                                             void* img, long long lo_off, int Tp, int Jp, void* stream) {
    if (!img || (lo_off % 8) || (reinterpret_cast<uintptr_t>(img) & 15) || !frames_args_ok(x, ldx, lens, B, n_fft, win, hop, Tmax, Tp, Jp))
        return IDV_EINVAL;
    const int KO = (win + 63) / 64 * 8;
    const size_t smem = (size_t)(hop * (RG_TT - 1) + win) * sizeof(float);
    hipLaunchKernelGGL(stft_frames_ragged_kernel<true>, dim3((Tmax + RG_TT - 1) / RG_TT, B), dim3(256), smem, (hipStream_t)stream, x,
                       ldx, lens, n_fft, win, hop, Tmax, (float*)nullptr, (unsigned short*)img, lo_off, KO, Tp, Jp);
    return idv_launch_status();
}

extern "C" int idv_istft_ola_ragged(const float* frames, const int* lens, int len_div, int B, int n_fft, int win, int hop, int Tmax,
                                    int Tp, int Jp, float* y, long long ldy, void* stream) {
    if (!frames || !lens || !y || len_div < 1 || B <= 0 || n_fft <= 0 || win <= 0 || win > n_fft || hop <= 0 || Tmax < 2 ||
        Tp < Tmax + 1 || (long long)Jp < (long long)B * Tp || ldy < (long long)hop * (Tmax - 1))
        return IDV_EINVAL;
    hipLaunchKernelGGL(istft_ola_ragged_kernel, dim3(grid_for((long long)B * hop * (Tmax - 1))), dim3(256), (size_t)win * sizeof(double),
                       (hipStream_t)stream, frames, lens, len_div, B, n_fft, win, hop, Tmax, Tp, Jp, y, ldy);
    return idv_launch_status();
}
