// Reverberation: each row convolved with its own room impulse response, dataset/reverb.py reverb / reverb_draw.
// Row b has n = lens[b] samples x at x + x_off[b] (or x + b ldx), K = taps[b] taps h at h + h_off[b] (or h + b ldh) and H = hist[b]
// real samples in front of its start:
//
//   y[i] = float( sum_{k < K} (double)h[k] (double)x[i - k] ),  x[j] = 0 for j < -H,   0 <= i < n;     y[i] = 0,  n <= i < L
//
// the definition of tests/reverb_ref.py (scipy.signal.fftconvolve(x, h)[:n] within its own error).  Every product of two floats is
// exact in double, the sum is double, the result ONE float32 rounding of it.
//
// Block-Toeplitz form on v_mfma_f64_16x16x4_f64.  Output i = i0 + 256 g + 16 a + r (r, a in 0 .. 15) is element [r][a] of tile g:
//   D_g[r][a] = sum_c sum_j M_c[r][j] X_g[j][a - c],   M_c[r][j] = h[16 c + r - j] (0 outside [0, K)),
//                                                     X_g[j][beta] = x[i0 + 256 g + 16 beta + j] (0 below -H and from n on)
// so tap block c is four MFMAs (j = 4 s + k, s = 0 .. 3) per 256 outputs, and every M_c with c >= 1 is a full matrix: the upper
// triangle of tap block c - 1 and the lower one of c share it.  c runs over 0 .. (K + 14) / 16.
//   A operand, lane l, step s:  M_c[l & 15][4 s + (l >> 4)];   B operand:  X_g[4 s + (l >> 4)][(l & 15) - c]
//   C/D (the f64 map):          lane l, register q holds D[(l >> 4) + 4 q][l & 15]
//
// A workgroup of four waves owns RV_T = 4096 consecutive outputs of one row, a wave four tiles (1024 outputs, 4 x 4 accumulator
// registers of doubles), so one A fragment feeds four MFMAs.  The tap blocks are walked in chunks of RV_CB = 64 in increasing c; per
// chunk the workgroup stages, as float32, the 16 RV_CB + 30 taps the chunk's M_c hold and the x window under them, samples
// i0 - 16 (c0 + RV_CB - 1) .. i0 + RV_T - 1, with the zeros of the definition put in at staging (nothing at or past x[n], before
// x[-H] or at or past h[K] is read, by scalar loads at any alignment).  Operands are converted to double at the LDS read.  The x
// window lies in blocks of 16 samples at a pitch of 17 floats: the B read of lane (a, k) is float 17 (a + const) + 4 s + k, and
// 17 a + k mod 64 takes 64 different values over a in 0 .. 15, k in 0 .. 3, where the pitch 16 would put the 16 lanes of a k on
// one bank.  The A read is 19 neighbouring floats, the equal addresses broadcast.
//
// Skipped work: tile g takes tap block c only while 16 c - 15 <= (its last output below n) + H, so a short row under a long
// response costs the triangle; tiles at or past n take none and write zeros.  What is skipped would have added +0.
// Order: output i adds its terms in increasing c, then increasing s, then the instruction's own order of k; c, s, k follow from
// (i mod 4096, K, H) of the row alone.  B, the other rows, L, the pitches, the pool offsets and the alignment of the pointers have
// no part in it.  No atomics, no work buffer.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int RV_MAX_TAPS = 1 << 16;
constexpr int RV_MAX_HIST = 65535;
constexpr int RV_T = 4096;                               // outputs of a workgroup
constexpr int RV_WT = RV_T / 4;                          // outputs of a wave: four tiles of 256
constexpr int RV_CB = 64;                                // tap blocks of a chunk
constexpr int RV_NB = RV_T / 16 + RV_CB - 1;             // 16-sample blocks of the x window of a chunk
constexpr int RV_PITCH = 17;                             // floats per block in LDS
constexpr int RV_HS = 16 * RV_CB + 15;                   // taps of a chunk: h[16 c0 - 15 .. 16 (c0 + RV_CB) - 1]

#define RV_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (double)(b), (c), 0, 0, 0)

__global__ __launch_bounds__(256) void reverb_kernel(const float* __restrict__ x, const long long* __restrict__ x_off, long long ldx,
                                                     const float* __restrict__ h, const long long* __restrict__ h_off, long long ldh,
                                                     const int* __restrict__ lens, const int* __restrict__ taps,
                                                     const int* __restrict__ hist, int L, int Kmax, float* __restrict__ y, long long ldy) {
    __shared__ float xw[RV_NB * RV_PITCH];
    __shared__ float hs[RV_HS + 1];
    const int b = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int i0 = blockIdx.x * RV_T;
    const float* xr = row_base(x, x_off, ldx, b);
    const float* hr = row_base(h, h_off, ldh, b);
    const int n = row_len(lens, b, L);
    const int K = max(1, min(taps[b], Kmax));
    const int H = max(0, min(hist ? hist[b] : 0, RV_MAX_HIST));
    const int nC = (K + 14) / 16 + 1;                                   // tap blocks: 16 c - 15 <= K - 1
    // tap block c reaches output i while 16 c - 15 <= i + H
    const int wg_last = min(i0 + RV_T, n) - 1;
    const int nc_wg = wg_last >= i0 ? min(nC, (wg_last + 15 + H) / 16 + 1) : 0;
    int cend[4], cmin = nC, cmax = 0;                                   // tile g takes the tap blocks below cend[g]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int tb = i0 + w * RV_WT + 256 * g, last = min(tb + 256, n) - 1;
        cend[g] = last >= tb ? min(nC, (last + 15 + H) / 16 + 1) : 0;
        cmin = min(cmin, cend[g]);
        cmax = max(cmax, cend[g]);
    }
    const int a = lane & 15, kq = lane >> 4;
    f64x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f64x4{0, 0, 0, 0};

    for (int c0 = 0; c0 < nc_wg; c0 += RV_CB) {
        __syncthreads();                                                // the previous chunk's operands have been read
        for (int t = tid; t < RV_HS; t += 256) {
            const int k = 16 * c0 - 15 + t;
            hs[t] = (k >= 0 && k < K) ? hr[k] : 0.f;
        }
        const int xs = i0 - 16 * (c0 + RV_CB - 1);                      // the window's first sample, a multiple of 16
        for (int e = tid; e < 16 * RV_NB; e += 256) {
            const int j = xs + e;
            xw[(e >> 4) * RV_PITCH + (e & 15)] = (j >= -H && j < n) ? xr[j] : 0.f;
        }
        __syncthreads();
        // A: hs[16 cc + 15 + r - j], r = a (the lane's row of M), j = 4 s + kq;  B: block w 64 + 16 g + a + (RV_CB - 1 - cc), float j
        const float* ha = hs + 15 + a - kq;
        const float* xb = xw + (w * 64 + a + RV_CB - 1) * RV_PITCH + kq;
        const int full = min(RV_CB, cmin - c0), part = min(RV_CB, cmax - c0);
        int cc = 0;
        for (; cc < full; ++cc) {                                       // all four tiles
            const float* pa = ha + 16 * cc;
            const float* pb = xb - cc * RV_PITCH;
            const double a0 = (double)pa[0], a1 = (double)pa[-4], a2 = (double)pa[-8], a3 = (double)pa[-12];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = RV_MFMA(a0, pb[16 * RV_PITCH * g], acc[g]);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = RV_MFMA(a1, pb[16 * RV_PITCH * g + 4], acc[g]);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = RV_MFMA(a2, pb[16 * RV_PITCH * g + 8], acc[g]);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = RV_MFMA(a3, pb[16 * RV_PITCH * g + 12], acc[g]);
        }
        for (; cc < part; ++cc) {                       // the edge of the triangle and the row's last wave: tile by tile
            const float* pa = ha + 16 * cc;
            const float* pb = xb - cc * RV_PITCH;
            const double a0 = (double)pa[0], a1 = (double)pa[-4], a2 = (double)pa[-8], a3 = (double)pa[-12];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (c0 + cc < cend[g]) {                                // wave-uniform
                    const float* pg = pb + 16 * RV_PITCH * g;
                    acc[g] = RV_MFMA(a0, pg[0], acc[g]);
                    acc[g] = RV_MFMA(a1, pg[4], acc[g]);
                    acc[g] = RV_MFMA(a2, pg[8], acc[g]);
                    acc[g] = RV_MFMA(a3, pg[12], acc[g]);
                }
            }
        }
    }
    // lane l, register q: row (l >> 4) + 4 q, column l & 15 of the tile
    float* yr = y + (long long)b * ldy;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + w * RV_WT + 256 * g + 16 * a + kq + 4 * q;
            if (i < L) yr[i] = i < n ? (float)acc[g][q] : 0.f;
        }
    }
}

}  // namespace

extern "C" int idv_reverb(const float* x, const long long* x_off, long long ldx, const float* h, const long long* h_off, long long ldh,
                          const int* lens, const int* taps, const int* hist, int B, int L, int Kmax, float* y, long long ldy, void* stream) {
    if (!x || !h || !taps || !y || !row_limits_ok(B, L) || Kmax <= 0 || Kmax > RV_MAX_TAPS) return IDV_EINVAL;
    if ((!x_off && ldx < L) || (!h_off && ldh < Kmax) || ldy < L) return IDV_EINVAL;
    if (!aligned_to(4, {x, h, y, lens, taps, hist}) || !aligned_to(8, {x_off, h_off})) return IDV_EINVAL;
    const unsigned gx = (unsigned)(((long long)L + RV_T - 1) / RV_T);
    hipLaunchKernelGGL(reverb_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, x_off, ldx, h, h_off, ldh, lens, taps, hist, L, Kmax,
                       y, ldy);
    return idv_launch_status();
}
