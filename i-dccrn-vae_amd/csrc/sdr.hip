// BSS-eval SDR of a padded batch, one source, a K-tap distortion filter (inference.compute_sdr; tests/sdr_ref.py).
// Row b has n = lens[b] samples of the reference s and of the estimate e, both zero outside [0, n):
//
//   r[k] = sum_i s[i] s[i + k],  d[k] = sum_i s[i] e[i + k]    (0 <= k < K)
//   G c = d,  G[i][j] = r[|i - j|]
//   p[i] = sum_{k < K} c[k] s[i - k],  err[i] = e[i] - p[i]    (0 <= i < n + K - 1)
//   out = float( 10 log10( sum p^2 / sum err^2 ) )
//
// Three passes and a row-wise end, all in double (a product of two float32 is exact in double):
//
// 1. sdr_corr_kernel: r and d as a block-Toeplitz product on v_mfma_f64_16x16x4_f64.  Lag k = 16 a + t is element [t][a] of a tile of
//    256 lags, and with the samples cut into blocks of 16, i = 16 m + j - t:
//      D[t][a] = sum_m sum_j S_m[t][j] Y_m[j][a],   S_m[t][j] = s[16 m + j - t],   Y_m[j][a] = y[16 (m + a) + j]     (y = s for r, e for d)
//    so a sample block m is four MFMAs (j = 4 q + k) per 256 lags; m runs over 0 .. (n + 14) / 16.
//      A operand, lane l, step q:  S_m[l & 15][4 q + (l >> 4)];   B operand:  Y_m[4 q + (l >> 4)][l & 15]
//      C/D (the f64 map):          lane l, register v holds D[(l >> 4) + 4 v][l & 15]
//    A workgroup of four waves owns SD_MB = 256 sample blocks of one row; wave w takes y = (w & 1 ? e : s) and the lags
//    256 (w >> 1) .. 256 (w >> 1) + 255 (a wave whose lags start at or past K has no part).  The workgroup stages s flat (the A
//    operand: 19 neighbouring floats per read, equal addresses broadcast) and the windows of s and e under the tile in blocks of 16
//    at a pitch of 17 floats, as reverb.hip does, with the zeros of the definition put in at staging.  Step q has its own accumulator
//    (four independent MFMA chains), the four are added as (0 + 1) + (2 + 3), and the tile's 2 K sums go to `work`.
// 2. sdr_solve_kernel: one workgroup of 512 threads per row.  It adds the row's tiles in increasing order, then runs the Levinson
//    recursion for a symmetric Toeplitz matrix with a general right side: thread t holds a[t] (the prediction-error filter) and c[t];
//    step i is two dot products of i terms (wave butterfly, then the eight waves left to right), the reflection update of a through a
//    double-buffered copy in LDS, and the update of c: two barriers a step.  A prediction error that is not positive ends the row as
//    NaN (a numerically singular G, e.g. a pure tone without a noise floor), and so does r[0] == 0 (a silent reference).
// 3. sdr_proj_kernel: p = c * s over the n + K - 1 outputs in reverb.hip's block-Toeplitz form with double taps (output i = 16 a + t of a
//    tile of 256, tap block u: M_u[t][j] = c[16 u + t - j], X[j][a - u] = s[16 (a - u) + j]); a workgroup owns SD_T = 4096 outputs, a
//    wave four tiles.  p stays in the accumulators: each lane adds p^2 and (e - p)^2 of its outputs in increasing (tile, register), the
//    lanes meet in the butterfly, the waves left to right, and the two sums of the workgroup go to `work`.  The energies come from
//    the explicit residual, not from the quadratic forms c'd and sum e^2 - c'd, which cancel at high SDR.
// 4. sdr_final_kernel: a row's workgroup sums in increasing order, the dB value and the special rows.
//
// Order: every sum's order follows from the row's own (n, K).  B, the other rows, Lmax, the pitches and the padding have no part in it;
// nothing at or past lens[b] is read.  No atomics, every loop bounded.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

#include <math.h>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SD_KMAX = 512;
constexpr int SD_PITCH = 17;                             // floats per 16-sample block in LDS
constexpr int SD_MB = 256;                               // sample blocks of a workgroup of the correlation pass
constexpr int SD_NB = SD_MB + SD_KMAX / 16 - 1;          // blocks of its y windows
constexpr int SD_FLAT = 16 * SD_MB + 15;                 // floats of its flat s window: s[16 m0 - 15 .. 16 (m0 + SD_MB) - 1]
constexpr int SD_T = 4096;                               // outputs of a workgroup of the projection pass
constexpr int SD_CB = SD_KMAX / 16 + 1;                  // tap blocks at most: 16 u - 15 <= K - 1
constexpr int SD_XB = SD_T / 16 + SD_CB - 1;             // blocks of its s window
constexpr int SD_CS = 16 * SD_CB + 15;                   // taps staged: c[-15 .. 16 SD_CB - 1]

#define SD_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((double)(a), (double)(b), (c), 0, 0, 0)

__host__ __device__ inline int corr_blocks(int n) { return n > 0 ? (n + 14) / 16 + 1 : 0; }
__host__ __device__ inline int corr_tiles(int n) { return (corr_blocks(n) + SD_MB - 1) / SD_MB; }
__host__ __device__ inline int proj_tiles(int n, int K) { return n > 0 ? (int)(((long long)n + K - 1 + SD_T - 1) / SD_T) : 0; }

__global__ __launch_bounds__(256) void sdr_corr_kernel(const float* __restrict__ ref, long long ref_ld, const float* __restrict__ est,
                                                       long long est_ld, const int* __restrict__ lens, int L, int K,
                                                       double* __restrict__ part, int tile_pitch) {
    __shared__ float yw[2][SD_NB * SD_PITCH];
    __shared__ float sf[SD_FLAT + 1];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int n = row_len(lens, b, L);
    const int nM = corr_blocks(n), m0 = tile * SD_MB;
    if (m0 >= nM) return;                                               // the row ends before this tile: the solve pass does not read it
    const float* sr = ref + (long long)b * ref_ld;
    const float* er = est + (long long)b * est_ld;
    const int base = 16 * m0;
    for (int e = tid; e < 16 * SD_NB; e += 256) {
        const int j = base + e, at = (e >> 4) * SD_PITCH + (e & 15);
        const bool in = j < n;
        yw[0][at] = in ? sr[j] : 0.f;
        yw[1][at] = in ? er[j] : 0.f;
    }
    for (int t = tid; t < SD_FLAT; t += 256) {
        const int j = base - 15 + t;
        sf[t] = (j >= 0 && j < n) ? sr[j] : 0.f;
    }
    __syncthreads();
    const int sig = w & 1, half = w >> 1;
    if (256 * half >= K) return;                                        // wave-uniform, behind the last barrier
    const int a = lane & 15, kq = lane >> 4;
    const int mend = min(SD_MB, nM - m0);
    // A: sf[16 mm + 15 + j - t], t = a (the lane's row of S), j = 4 q + kq;  B: block mm + a + 16 half, float j
    const float* pa = sf + 15 + kq - a;
    const float* pb = yw[sig] + (a + 16 * half) * SD_PITCH + kq;
    f64x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0}, acc2 = {0, 0, 0, 0}, acc3 = {0, 0, 0, 0};
    for (int mm = 0; mm < mend; ++mm) {
        const float* qa = pa + 16 * mm;
        const float* qb = pb + SD_PITCH * mm;
        acc0 = SD_MFMA(qa[0], qb[0], acc0);
        acc1 = SD_MFMA(qa[4], qb[4], acc1);
        acc2 = SD_MFMA(qa[8], qb[8], acc2);
        acc3 = SD_MFMA(qa[12], qb[12], acc3);
    }
    const f64x4 acc = (acc0 + acc1) + (acc2 + acc3);
    // lane l, register v: row (l >> 4) + 4 v, column l & 15 of the tile: lag 16 column + row
    double* out = part + (((long long)b * tile_pitch + tile) * 2 + sig) * K;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int k = 16 * (a + 16 * half) + kq + 4 * v;
        if (k < K) out[k] = acc[v];
    }
}

__global__ __launch_bounds__(512) void sdr_solve_kernel(const double* __restrict__ part, int tile_pitch, const int* __restrict__ lens, int L,
                                                        int K, double* __restrict__ cw, double* __restrict__ status,
                                                        double* __restrict__ filt) {
    __shared__ double rs[SD_KMAX], ds[SD_KMAX], ab[2][SD_KMAX], sh[2][16];
    const int b = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int nT = corr_tiles(row_len(lens, b, L));
    for (int idx = t; idx < 2 * K; idx += 512) {
        const int sig = idx >= K, k = idx - sig * K;
        const double* src = part + ((long long)b * tile_pitch * 2 + sig) * K + k;
        double s = 0.0;
        for (int tile = 0; tile < nT; ++tile) s += src[(long long)tile * 2 * K];
        (sig ? ds : rs)[k] = s;
    }
    ab[0][t] = t == 0 ? 1.0 : 0.0;
    ab[1][t] = 0.0;
    __syncthreads();
    const double r0 = rs[0];
    int bad = r0 > 0.0 ? 0 : 1;                                         // 1: a silent reference (or one that is not finite)
    double E = r0, a = t == 0 ? 1.0 : 0.0, x = (t == 0 && !bad) ? ds[0] / r0 : 0.0;
    if (!bad) {
        for (int i = 1; i < K; ++i) {
            const double rv = t < i ? rs[i - t] : 0.0;
            const double v1 = wave_sum_d(a * rv), v2 = wave_sum_d(x * rv);
            double* shp = sh[i & 1];
            if (lane == 0) {
                shp[w] = v1;
                shp[8 + w] = v2;
            }
            __syncthreads();
            double s1 = shp[0], s2 = shp[8];
#pragma unroll
            for (int q = 1; q < 8; ++q) {
                s1 += shp[q];
                s2 += shp[8 + q];
            }
            const double lam = -s1 / E;
            a = t <= i ? a + lam * ab[(i - 1) & 1][i - t] : 0.0;
            ab[i & 1][t] = a;
            E = E * (1.0 - lam * lam);
            if (!(E > 0.0)) {                                           // the same value in every thread
                bad = 2;
                break;
            }
            __syncthreads();
            const double mu = (ds[i] - s2) / E;
            if (t <= i) x += mu * ab[i & 1][i - t];
        }
    }
    if (t < K) {
        const double c = bad ? (double)NAN : x;
        cw[(long long)b * K + t] = c;
        if (filt) filt[(long long)b * K + t] = c;
    }
    if (t == 0) status[b] = (double)bad;
}

__global__ __launch_bounds__(256) void sdr_proj_kernel(const float* __restrict__ ref, long long ref_ld, const float* __restrict__ est,
                                                       long long est_ld, const int* __restrict__ lens, int L, int K,
                                                       const double* __restrict__ cw, double* __restrict__ part, int tile_pitch) {
    __shared__ float xw[SD_XB * SD_PITCH];
    __shared__ double cs[SD_CS + 1];
    __shared__ double shw[4];
    const int b = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int n = row_len(lens, b, L);
    const long long i0l = (long long)blockIdx.x * SD_T;
    if (n < 1 || i0l >= (long long)n + K - 1) return;                   // the row ends before this tile: the end pass does not read it
    const int i0 = (int)i0l, nout = n + K - 1;                          // n <= 2^27: an int with room to spare
    const float* sr = ref + (long long)b * ref_ld;
    const float* er = est + (long long)b * est_ld;
    const double* cr = cw + (long long)b * K;
    const int nC = K / 16 + 1;                                          // tap blocks: 16 u - 15 <= K - 1
    for (int t = tid; t < 16 * nC + 15; t += 256) {
        const int k = t - 15;
        cs[t] = (k >= 0 && k < K) ? cr[k] : 0.0;
    }
    const int xs = i0 - 16 * (nC - 1);                                  // the window's first sample, a multiple of 16
    for (int e = tid; e < 16 * (SD_T / 16 + nC - 1); e += 256) {
        const int j = xs + e;
        xw[(e >> 4) * SD_PITCH + (e & 15)] = (j >= 0 && j < n) ? sr[j] : 0.f;
    }
    __syncthreads();
    const int a = lane & 15, kq = lane >> 4;
    bool on[4];                                                         // tile g has outputs of the row
#pragma unroll
    for (int g = 0; g < 4; ++g) on[g] = i0 + w * 1024 + 256 * g < nout;
    f64x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f64x4{0, 0, 0, 0};
    // A: cs[16 u + 15 + t - j], t = a (the lane's row of M), j = 4 q + kq;  B: block w 64 + 16 g + a + (nC - 1 - u), float j
    const double* ca = cs + 15 + a - kq;
    const float* xb = xw + (w * 64 + a + nC - 1) * SD_PITCH + kq;
    for (int u = 0; u < nC; ++u) {
        const double* pa = ca + 16 * u;
        const float* pb = xb - u * SD_PITCH;
        const double a0 = pa[0], a1 = pa[-4], a2 = pa[-8], a3 = pa[-12];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (on[g]) {                                                // wave-uniform
                const float* pg = pb + 16 * SD_PITCH * g;
                acc[g] = SD_MFMA(a0, pg[0], acc[g]);
                acc[g] = SD_MFMA(a1, pg[4], acc[g]);
                acc[g] = SD_MFMA(a2, pg[8], acc[g]);
                acc[g] = SD_MFMA(a3, pg[12], acc[g]);
            }
        }
    }
    // lane l, register v: row (l >> 4) + 4 v, column l & 15 of the tile
    double sp = 0.0, se = 0.0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + w * 1024 + 256 * g + 16 * a + kq + 4 * v;
            if (i < nout) {
                const double pv = acc[g][v];
                const double ev = (i < n ? (double)er[i] : 0.0) - pv;
                sp += pv * pv;
                se += ev * ev;
            }
        }
    }
    sp = waves_sum<4>(sp, shw);
    se = waves_sum<4>(se, shw);
    if (tid == 0) {
        double* out = part + ((long long)b * tile_pitch + blockIdx.x) * 2;
        out[0] = sp;
        out[1] = se;
    }
}

__global__ __launch_bounds__(64) void sdr_final_kernel(const double* __restrict__ part, int tile_pitch, const double* __restrict__ status,
                                                       const int* __restrict__ lens, int L, int K, int B, float* __restrict__ out,
                                                       double* __restrict__ details) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int nT = proj_tiles(row_len(lens, b, L), K);
    const double* src = part + (long long)b * tile_pitch * 2;
    double sp = 0.0, se = 0.0;
    for (int tile = 0; tile < nT; ++tile) {
        sp += src[2 * tile];
        se += src[2 * tile + 1];
    }
    float v;
    if (nT == 0 || status[b] != 0.0) {                                  // a silent reference, a solve that met a non-positive pivot
        v = NAN;
        sp = se = (double)NAN;
    } else if (sp == 0.0) {
        v = -INFINITY;                                                  // a silent estimate
    } else if (se == 0.0) {
        v = INFINITY;
    } else {
        v = (float)(10.0 * log10(sp / se));
    }
    out[b] = v;
    if (details) {
        details[2 * b] = sp;
        details[2 * b + 1] = se;
    }
}

struct Layout {
    long long t1, t3;                                                   // tiles per row of the two tiled passes
    long long off_c, off_status, off_part3, doubles;                    // in doubles; the correlation partials lie at 0
};

inline Layout layout(int B, int Lmax, int K) {
    Layout l;
    l.t1 = corr_tiles(Lmax);
    l.t3 = proj_tiles(Lmax, K);
    l.off_c = (long long)B * l.t1 * 2 * K;
    l.off_status = l.off_c + (long long)B * K;
    l.off_part3 = l.off_status + B;
    l.doubles = l.off_part3 + (long long)B * l.t3 * 2;
    return l;
}

inline bool filt_len_ok(int K) { return K >= 16 && K <= SD_KMAX && K % 16 == 0; }

}  // namespace

extern "C" long long idv_sdr_work_bytes(int B, int Lmax, int K) {
    if (!row_limits_ok(B, Lmax) || !filt_len_ok(K)) return -1;
    return layout(B, Lmax, K).doubles * (long long)sizeof(double);
}

extern "C" int idv_sdr(const float* ref, long long ref_ld, const float* est, long long est_ld, const int* lens, int B, int Lmax, int K,
                       void* work, long long work_bytes, float* out, double* details, double* filt, void* stream) {
    if (!ref || !est || !work || !out || !row_limits_ok(B, Lmax) || !filt_len_ok(K)) return IDV_EINVAL;
    if (ref_ld < Lmax || est_ld < Lmax) return IDV_EINVAL;
    if (!aligned_to(16, {work}) || !aligned_to(8, {details, filt}) || !aligned_to(4, {ref, est, lens, out})) return IDV_EINVAL;
    const Layout l = layout(B, Lmax, K);
    if (work_bytes < l.doubles * (long long)sizeof(double)) return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double* wk = (double*)work;
    double* cw = wk + l.off_c;
    double* status = wk + l.off_status;
    double* part3 = wk + l.off_part3;
    hipLaunchKernelGGL(sdr_corr_kernel, dim3((unsigned)l.t1, B), dim3(256), 0, st, ref, ref_ld, est, est_ld, lens, Lmax, K, wk, (int)l.t1);
    hipLaunchKernelGGL(sdr_solve_kernel, dim3(B), dim3(512), 0, st, wk, (int)l.t1, lens, Lmax, K, cw, status, filt);
    hipLaunchKernelGGL(sdr_proj_kernel, dim3((unsigned)l.t3, B), dim3(256), 0, st, ref, ref_ld, est, est_ld, lens, Lmax, K, cw, part3,
                       (int)l.t3);
    hipLaunchKernelGGL(sdr_final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, part3, (int)l.t3, status, lens, Lmax, K, B, out, details);
    return idv_launch_status();
}
