// BSS-eval SDR, SIR and SAR of a padded batch with TWO sources: the target and one interferer, K-tap distortion filters
// (inference.compute_bss; tests/bss_ref.py).  Row b has n = lens[b] samples of the target reference s, of the
// interferer reference v and of the estimate y, all zero outside [0, n):
//
//   x_ab[k] = sum_i a[i] b[i + k]   (a, b in {s, v}),   d_a[k] = sum_i a[i] y[i + k]                     (0 <= k < K; x_ab[-k] = x_ba[k])
//   G_ss c = d_s                                        (K x K: the system of sdr.hip)
//   [G_ss G_sv; G_vs G_vv] [C_s; C_v] = [d_s; d_v],     G_ab[i][j] = x_ab[i - j]                          (2K x 2K)
//   p1 = c * s,  pall = C_s * s + C_v * v                                                                (0 <= i < n + K - 1)
//   SDR = 10 log10( sum p1^2 / sum (y - p1)^2 ),  SIR = 10 log10( sum p1^2 / sum (pall - p1)^2 ),  SAR = 10 log10( sum pall^2 / sum (y - pall)^2 )
//
// The SDR column, c, sum p1^2 and sum (y - p1)^2 are idv_sdr's own (its four launches run first, on a slice of `work`), so they are
// the bits compute_sdr returns.  Then, all in double (a product of two float32 is exact in double):
//
// 1. bss_corr_kernel: the six lag sets as block-Toeplitz products on v_mfma_f64_16x16x4_f64, in the form of sdr_corr_kernel (lag
//    k = 16 a + t is element [t][a] of a tile of 256 lags; sample block m is four MFMAs per tile and pair).  A workgroup of four waves
//    owns BS_MB = 256 sample blocks of one row and stages s, v and y once, in blocks of 16 at a pitch of 17 floats with one block in
//    front (the A operand reaches 15 samples back; it is read from the same pitched image, so the three windows are all the LDS there
//    is: 58.75 KB).  Wave w takes the A operand of (w & 1 ? v : s) and the lags 256 (w >> 1) .. 256 (w >> 1) + 255: one A fragment
//    feeds three MFMAs, against s, v and y.  Step q of each pair has its own accumulator (twelve independent chains), the four are
//    added as (0 + 1) + (2 + 3), and the tile's 6 K sums go to `work` in the order x_ss, x_sv, d_s, x_vs, x_vv, d_v.
// 2. bss_solve_kernel: one workgroup of 512 threads per row.  It adds the row's tiles in increasing order, then runs the block
//    Levinson recursion (Whittle; Wiggins and Robinson) on G reordered by interleaving the two sources, a symmetric block-Toeplitz
//    matrix of 2 x 2 blocks R_k = [x_ss[k] x_sv[k]; x_vs[k] x_vv[k]], R_-k = R_k'.  Thread t holds block t of the forward predictor F,
//    of the backward predictor B (stored reversed) and of the solution X: ten doubles.  Step n: D = sum_j R_{n-j} F_j and
//    sum_j R_{n-j} X_j (six sums: wave butterfly, then the eight waves left to right; the backward sum is D', G being symmetric),
//    F_t -= B_{n-t} Eb^-1 D, B_t -= F_{n-t} Ef^-1 D' through one copy of F and B in LDS (32 KB; with the lags 56 KB), the two 2 x 2
//    error matrices, then X_t += B_{n-t} Eb^-1 (d_n - sum): three barriers a step.  An error matrix that is not positive definite
//    ends the row as NaN (a numerically singular G, e.g. v = 2 s), and so do n <= K (2 K unknowns, n + K - 1 equations), a silent
//    reference and a silent interferer.
// 3. bss_proj_kernel: p1 and pall over the n + K - 1 outputs in the block-Toeplitz form of sdr_proj_kernel with three tap sets and two
//    sample windows; a workgroup owns BS_T = 4096 outputs, a wave four tiles.  p1 and pall stay in the accumulators; each lane adds
//    (pall - p1)^2, pall^2 and (y - pall)^2 of its outputs in increasing (tile, register), the lanes meet in the butterfly, the waves
//    left to right, and the three sums of the workgroup go to `work`.
// 4. bss_final_kernel: a row's workgroup sums in increasing order, the three dB values and the special rows.
//
// Order: every sum's order follows from the row's own (n, K).  B, the other rows, Lmax, the pitches and the padding have no part in it;
// nothing at or past lens[b] is read.  No atomics, every loop bounded.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

#include <math.h>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BS_KMAX = 512;
constexpr int BS_PITCH = 17;                             // floats per 16-sample block in LDS
constexpr int BS_MB = 256;                               // sample blocks of a workgroup of the correlation pass
constexpr int BS_NB = 1 + BS_MB + BS_KMAX / 16 - 1;      // blocks of its windows: one in front for the A operand
constexpr int BS_T = 4096;                               // outputs of a workgroup of the projection pass
constexpr int BS_CB = BS_KMAX / 16 + 1;                  // tap blocks at most: 16 u - 15 <= K - 1
constexpr int BS_XB = BS_T / 16 + BS_CB - 1;             // blocks of its sample windows
constexpr int BS_CS = 16 * BS_CB + 15;                   // taps staged: c[-15 .. 16 BS_CB - 1]

#define BS_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((double)(a), (double)(b), (c), 0, 0, 0)

__host__ __device__ inline int corr_blocks(int n) { return n > 0 ? (n + 14) / 16 + 1 : 0; }
__host__ __device__ inline int corr_tiles(int n) { return (corr_blocks(n) + BS_MB - 1) / BS_MB; }
__host__ __device__ inline int proj_tiles(int n, int K) { return n > 0 ? (int)(((long long)n + K - 1 + BS_T - 1) / BS_T) : 0; }

__global__ __launch_bounds__(256) void bss_corr_kernel(const float* __restrict__ ref, long long ref_ld, const float* __restrict__ itf,
                                                       long long itf_ld, const float* __restrict__ est, long long est_ld,
                                                       const int* __restrict__ lens, int L, int K, double* __restrict__ part,
                                                       int tile_pitch) {
    __shared__ float yw[3][BS_NB * BS_PITCH];                           // s, v, y from sample 16 m0 - 16 on
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int n = row_len(lens, b, L);
    const int nM = corr_blocks(n), m0 = tile * BS_MB;
    if (m0 >= nM) return;                                               // the row ends before this tile: the solve pass does not read it
    const float* sr = ref + (long long)b * ref_ld;
    const float* vr = itf + (long long)b * itf_ld;
    const float* er = est + (long long)b * est_ld;
    const int base = 16 * m0 - 16;
    for (int e = tid; e < 16 * BS_NB; e += 256) {
        const int j = base + e, at = (e >> 4) * BS_PITCH + (e & 15);
        const bool in = j >= 0 && j < n;
        yw[0][at] = in ? sr[j] : 0.f;
        yw[1][at] = in ? vr[j] : 0.f;
        yw[2][at] = in ? er[j] : 0.f;
    }
    __syncthreads();
    const int asig = w & 1, half = w >> 1;
    if (256 * half >= K) return;                                        // wave-uniform, behind the last barrier
    const int a = lane & 15, kq = lane >> 4;
    const int mend = min(BS_MB, nM - m0);
    // A: sample 16 (m0 + mm) + j - t of the A signal, t = a (the lane's row of S), j = 4 q + kq: 16 + j - t = 1 .. 31 floats into block mm
    // B: block 1 + mm + a + 16 half, float j
    int offa[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int o = 16 + 4 * q + kq - a;
        offa[q] = (o >> 4) * BS_PITCH + (o & 15);
    }
    const float* pa = yw[asig];
    const int offb = (1 + a + 16 * half) * BS_PITCH + kq;
    f64x4 acc[3][4];
#pragma unroll
    for (int y = 0; y < 3; ++y)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[y][q] = f64x4{0, 0, 0, 0};
    for (int mm = 0; mm < mend; ++mm) {
        const float* qa = pa + BS_PITCH * mm;
        const float a0 = qa[offa[0]], a1 = qa[offa[1]], a2 = qa[offa[2]], a3 = qa[offa[3]];
#pragma unroll
        for (int y = 0; y < 3; ++y) {
            const float* qb = yw[y] + offb + BS_PITCH * mm;
            acc[y][0] = BS_MFMA(a0, qb[0], acc[y][0]);
            acc[y][1] = BS_MFMA(a1, qb[4], acc[y][1]);
            acc[y][2] = BS_MFMA(a2, qb[8], acc[y][2]);
            acc[y][3] = BS_MFMA(a3, qb[12], acc[y][3]);
        }
    }
    // lane l, register r: row (l >> 4) + 4 r, column l & 15 of the tile: lag 16 column + row
    double* out = part + (((long long)b * tile_pitch + tile) * 6 + 3 * asig) * K;
#pragma unroll
    for (int y = 0; y < 3; ++y) {
        const f64x4 s4 = (acc[y][0] + acc[y][1]) + (acc[y][2] + acc[y][3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * (a + 16 * half) + kq + 4 * r;
            if (k < K) out[(long long)y * K + k] = s4[r];
        }
    }
}

// 2 x 2 matrices, row-major in four doubles
struct M2 {
    double a, b, c, d;
};
__device__ __forceinline__ M2 mul(const M2& x, const M2& y) {
    return M2{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}
__device__ __forceinline__ M2 sub(const M2& x, const M2& y) { return M2{x.a - y.a, x.b - y.b, x.c - y.c, x.d - y.d}; }
__device__ __forceinline__ M2 tr(const M2& x) { return M2{x.a, x.c, x.b, x.d}; }
// two rounded products: fused, x.a x.d - round(x.b x.c) of an exactly singular block (v = 2 s) is the rounding error of the second
// product, of either sign, where the definition has 0
__device__ __forceinline__ double det(const M2& x) {
#pragma clang fp contract(off)
    const double ad = x.a * x.d, bc = x.b * x.c;
    return ad - bc;
}
__device__ __forceinline__ M2 inv(const M2& x) {
    const double q = 1.0 / det(x);
    return M2{x.d * q, -x.b * q, -x.c * q, x.a * q};
}
// positive definite as far as the recursion needs it (false for NaN)
__device__ __forceinline__ bool posdef(const M2& x) { return x.a > 0.0 && x.d > 0.0 && det(x) > 0.0; }

__global__ __launch_bounds__(512) void bss_solve_kernel(const double* __restrict__ part, int tile_pitch, const int* __restrict__ lens, int L,
                                                        int K, double* __restrict__ cw, double* __restrict__ status,
                                                        double* __restrict__ filt) {
    __shared__ double Rl[4][BS_KMAX], dl[2][BS_KMAX], fb[8][BS_KMAX], sh[2][6][8];
    const int b = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int n = row_len(lens, b, L);
    const int nT = corr_tiles(n);
    // the sets of a tile: x_ss, x_sv, d_s, x_vs, x_vv, d_v
    for (int idx = t; idx < 6 * K; idx += 512) {
        const int set = idx / K, k = idx - set * K;
        const double* src = part + ((long long)b * tile_pitch * 6 + set) * K + k;
        double s = 0.0;
        for (int tile = 0; tile < nT; ++tile) s += src[(long long)tile * 6 * K];
        if (set == 2) dl[0][k] = s;
        else if (set == 5) dl[1][k] = s;
        else Rl[set < 2 ? set : set - 1][k] = s;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) fb[q][t] = (t == 0 && (q == 0 || q == 3 || q == 4 || q == 7)) ? 1.0 : 0.0;
    __syncthreads();
    const M2 R0{Rl[0][0], Rl[1][0], Rl[2][0], Rl[3][0]};
    // 1: too short for the joint system, a silent reference or interferer (or one that is not finite); 2: a pivot that is not positive
    int bad = (n > K && R0.a > 0.0 && R0.d > 0.0) ? 0 : 1;
    if (!bad && !posdef(R0)) bad = 2;
    M2 F{t == 0 ? 1.0 : 0.0, 0.0, 0.0, t == 0 ? 1.0 : 0.0}, Bk = F, Ef = R0, Eb = R0;
    double x0 = 0.0, x1 = 0.0;
    if (!bad) {
        if (t == 0) {
            const M2 Ri = inv(R0);
            x0 = Ri.a * dl[0][0] + Ri.b * dl[1][0];
            x1 = Ri.c * dl[0][0] + Ri.d * dl[1][0];
        }
        for (int i = 1; i < K; ++i) {
            M2 P{0, 0, 0, 0};
            double p0 = 0.0, p1 = 0.0;
            if (t < i) {
                const M2 Rm{Rl[0][i - t], Rl[1][i - t], Rl[2][i - t], Rl[3][i - t]};
                P = mul(Rm, F);
                p0 = Rm.a * x0 + Rm.b * x1;
                p1 = Rm.c * x0 + Rm.d * x1;
            }
            const double v0 = wave_sum_d(P.a), v1 = wave_sum_d(P.b), v2 = wave_sum_d(P.c), v3 = wave_sum_d(P.d), v4 = wave_sum_d(p0),
                         v5 = wave_sum_d(p1);
            double(*shp)[8] = sh[i & 1];
            if (lane == 0) {
                shp[0][w] = v0;
                shp[1][w] = v1;
                shp[2][w] = v2;
                shp[3][w] = v3;
                shp[4][w] = v4;
                shp[5][w] = v5;
            }
            __syncthreads();
            double s[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                s[q] = shp[q][0];
#pragma unroll
                for (int u = 1; u < 8; ++u) s[q] += shp[q][u];
            }
            const M2 D{s[0], s[1], s[2], s[3]};
            const M2 Kf = mul(inv(Eb), D), Kb = mul(inv(Ef), tr(D));
            M2 Fo{0, 0, 0, 0}, Bo{0, 0, 0, 0};                          // F and B of the step before at block i - t
            if (t >= 1 && t <= i) {
                Fo = M2{fb[0][i - t], fb[1][i - t], fb[2][i - t], fb[3][i - t]};
                Bo = M2{fb[4][i - t], fb[5][i - t], fb[6][i - t], fb[7][i - t]};
            }
            F = sub(F, mul(Bo, Kf));
            Bk = sub(Bk, mul(Fo, Kb));
            Ef = sub(Ef, mul(tr(D), Kf));
            Eb = sub(Eb, mul(D, Kb));
            if (!posdef(Ef) || !posdef(Eb)) {                           // the same values in every thread
                bad = 2;
                break;
            }
            __syncthreads();
            fb[0][t] = F.a;
            fb[1][t] = F.b;
            fb[2][t] = F.c;
            fb[3][t] = F.d;
            fb[4][t] = Bk.a;
            fb[5][t] = Bk.b;
            fb[6][t] = Bk.c;
            fb[7][t] = Bk.d;
            __syncthreads();
            const M2 Ei = inv(Eb);
            const double g0 = dl[0][i] - s[4], g1 = dl[1][i] - s[5];
            const double mu0 = Ei.a * g0 + Ei.b * g1, mu1 = Ei.c * g0 + Ei.d * g1;
            if (t <= i) {
                x0 += fb[4][i - t] * mu0 + fb[5][i - t] * mu1;
                x1 += fb[6][i - t] * mu0 + fb[7][i - t] * mu1;
            }
        }
    }
    if (t < K) {
        const double cs = bad ? (double)NAN : x0, cv = bad ? (double)NAN : x1;
        double* o = cw + (long long)b * 2 * K;
        o[t] = cs;
        o[K + t] = cv;
        if (filt) {
            filt[(long long)b * 2 * K + t] = cs;
            filt[(long long)b * 2 * K + K + t] = cv;
        }
    }
    if (t == 0) status[b] = (double)bad;
}

__global__ __launch_bounds__(256) void bss_proj_kernel(const float* __restrict__ ref, long long ref_ld, const float* __restrict__ itf,
                                                       long long itf_ld, const float* __restrict__ est, long long est_ld,
                                                       const int* __restrict__ lens, int L, int K, const double* __restrict__ c1,
                                                       const double* __restrict__ cw, const double* __restrict__ status,
                                                       double* __restrict__ part, int tile_pitch) {
    __shared__ float xw[2][BS_XB * BS_PITCH];                           // s, v
    __shared__ double cs[3][BS_CS + 1];                                 // c, C_s, C_v
    __shared__ double shw[4];
    const int b = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int n = row_len(lens, b, L);
    const long long i0l = (long long)blockIdx.x * BS_T;
    if (n < 1 || i0l >= (long long)n + K - 1) return;                   // the row ends before this tile: the end pass does not read it
    if (status[b] != 0.0) return;                                       // a NaN row: the end pass does not read its sums
    const int i0 = (int)i0l, nout = n + K - 1;                          // n <= 2^27: an int with room to spare
    const float* sr = ref + (long long)b * ref_ld;
    const float* vr = itf + (long long)b * itf_ld;
    const float* er = est + (long long)b * est_ld;
    const double* c1r = c1 + (long long)b * K;
    const double* cr = cw + (long long)b * 2 * K;
    const int nC = K / 16 + 1;                                          // tap blocks: 16 u - 15 <= K - 1
    for (int t = tid; t < 16 * nC + 15; t += 256) {
        const int k = t - 15;
        const bool in = k >= 0 && k < K;
        cs[0][t] = in ? c1r[k] : 0.0;
        cs[1][t] = in ? cr[k] : 0.0;
        cs[2][t] = in ? cr[K + k] : 0.0;
    }
    const int xs = i0 - 16 * (nC - 1);                                  // the windows' first sample, a multiple of 16
    for (int e = tid; e < 16 * (BS_T / 16 + nC - 1); e += 256) {
        const int j = xs + e, at = (e >> 4) * BS_PITCH + (e & 15);
        const bool in = j >= 0 && j < n;
        xw[0][at] = in ? sr[j] : 0.f;
        xw[1][at] = in ? vr[j] : 0.f;
    }
    __syncthreads();
    const int a = lane & 15, kq = lane >> 4;
    bool on[4];                                                         // tile g has outputs of the row
#pragma unroll
    for (int g = 0; g < 4; ++g) on[g] = i0 + w * 1024 + 256 * g < nout;
    f64x4 acc1[4], acca[4];                                             // p1, pall
#pragma unroll
    for (int g = 0; g < 4; ++g) acc1[g] = acca[g] = f64x4{0, 0, 0, 0};
    // A: cs[.][16 u + 15 + t - j], t = a (the lane's row of M), j = 4 q + kq;  B: block w 64 + 16 g + a + (nC - 1 - u), float j
    const int ca = 15 + a - kq;
    const int xb = (w * 64 + a + nC - 1) * BS_PITCH + kq;
    for (int u = 0; u < nC; ++u) {
        const int pa = ca + 16 * u;
        const int pb = xb - u * BS_PITCH;
        double t1[4], ts[4], tv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t1[q] = cs[0][pa - 4 * q];
            ts[q] = cs[1][pa - 4 * q];
            tv[q] = cs[2][pa - 4 * q];
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (on[g]) {                                                // wave-uniform
                const float* ps = xw[0] + pb + 16 * BS_PITCH * g;
                const float* pv = xw[1] + pb + 16 * BS_PITCH * g;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float sv = ps[4 * q];
                    acc1[g] = BS_MFMA(t1[q], sv, acc1[g]);
                    acca[g] = BS_MFMA(ts[q], sv, acca[g]);
                    acca[g] = BS_MFMA(tv[q], pv[4 * q], acca[g]);
                }
            }
        }
    }
    // lane l, register r: row (l >> 4) + 4 r, column l & 15 of the tile
    double si = 0.0, sp = 0.0, sa = 0.0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + w * 1024 + 256 * g + 16 * a + kq + 4 * r;
            if (i < nout) {
                const double pall = acca[g][r];
                const double ei = pall - acc1[g][r];
                const double ea = (i < n ? (double)er[i] : 0.0) - pall;
                si += ei * ei;
                sp += pall * pall;
                sa += ea * ea;
            }
        }
    }
    si = waves_sum<4>(si, shw);
    sp = waves_sum<4>(sp, shw);
    sa = waves_sum<4>(sa, shw);
    if (tid == 0) {
        double* out = part + ((long long)b * tile_pitch + blockIdx.x) * 3;
        out[0] = si;
        out[1] = sp;
        out[2] = sa;
    }
}

// a zero numerator gives -inf, otherwise a zero denominator +inf
__device__ __forceinline__ float ratio_db(double num, double den) {
    if (num == 0.0) return -INFINITY;
    if (den == 0.0) return INFINITY;
    return (float)(10.0 * log10(num / den));
}

__global__ __launch_bounds__(64) void bss_final_kernel(const double* __restrict__ part, int tile_pitch, const double* __restrict__ status,
                                                       const float* __restrict__ sdr, const double* __restrict__ sdr_det,
                                                       const int* __restrict__ lens, int L, int K, int B, float* __restrict__ out,
                                                       double* __restrict__ details) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float v = sdr[b];
    const double tp = sdr_det[2 * b], te = sdr_det[2 * b + 1];
    double si = (double)NAN, sp = si, sa = si;
    float sir = NAN, sar = NAN;
    if (status[b] == 0.0 && !isnan(v)) {
        const int nT = proj_tiles(row_len(lens, b, L), K);
        const double* src = part + (long long)b * tile_pitch * 3;
        si = sp = sa = 0.0;
        for (int tile = 0; tile < nT; ++tile) {
            si += src[3 * tile];
            sp += src[3 * tile + 1];
            sa += src[3 * tile + 2];
        }
        sir = ratio_db(tp, si);
        sar = ratio_db(sp, sa);
    }
    out[3 * b] = v;
    out[3 * b + 1] = sir;
    out[3 * b + 2] = sar;
    if (details) {
        double* o = details + 5 * (long long)b;
        o[0] = tp;
        o[1] = te;
        o[2] = si;
        o[3] = sp;
        o[4] = sa;
    }
}

struct Layout {
    long long t1, t3;                                                   // tiles per row of the two tiled passes
    // in doubles; idv_sdr's own work lies at 0
    long long off_sdr_out, off_sdr_det, off_c1, off_part1, off_cw, off_status, off_part3, doubles;
};

inline Layout layout(int B, int Lmax, int K, long long sdr_bytes) {
    Layout l;
    l.t1 = corr_tiles(Lmax);
    l.t3 = proj_tiles(Lmax, K);
    l.off_sdr_out = sdr_bytes / (long long)sizeof(double);
    l.off_sdr_det = l.off_sdr_out + (B + 1) / 2;                        // B floats
    l.off_c1 = l.off_sdr_det + 2LL * B;
    l.off_part1 = l.off_c1 + (long long)B * K;
    l.off_cw = l.off_part1 + (long long)B * l.t1 * 6 * K;
    l.off_status = l.off_cw + 2LL * B * K;
    l.off_part3 = l.off_status + B;
    l.doubles = l.off_part3 + (long long)B * l.t3 * 3;
    return l;
}

}  // namespace

extern "C" long long idv_bss_work_bytes(int B, int Lmax, int K) {
    const long long sdr_bytes = idv_sdr_work_bytes(B, Lmax, K);
    if (sdr_bytes < 0) return -1;
    return layout(B, Lmax, K, sdr_bytes).doubles * (long long)sizeof(double);
}

extern "C" int idv_bss(const float* ref, long long ref_ld, const float* interf, long long interf_ld, const float* est, long long est_ld,
                       const int* lens, int B, int Lmax, int K, void* work, long long work_bytes, float* out, double* details, double* filt,
                       void* stream) {
    if (!ref || !interf || !est || !work || !out) return IDV_EINVAL;
    const long long sdr_bytes = idv_sdr_work_bytes(B, Lmax, K);
    if (sdr_bytes < 0) return IDV_EINVAL;                               // B, Lmax or K outside their ranges
    if (ref_ld < Lmax || interf_ld < Lmax || est_ld < Lmax) return IDV_EINVAL;
    if (!aligned_to(16, {work}) || !aligned_to(8, {details, filt}) || !aligned_to(4, {ref, interf, est, lens, out})) return IDV_EINVAL;
    const Layout l = layout(B, Lmax, K, sdr_bytes);
    if (work_bytes < l.doubles * (long long)sizeof(double)) return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double* wk = (double*)work;
    float* sdr_out = (float*)(wk + l.off_sdr_out);
    double* sdr_det = wk + l.off_sdr_det;
    double* c1 = wk + l.off_c1;
    double* part1 = wk + l.off_part1;
    double* cw = wk + l.off_cw;
    double* status = wk + l.off_status;
    double* part3 = wk + l.off_part3;
    const int rc = idv_sdr(ref, ref_ld, est, est_ld, lens, B, Lmax, K, work, sdr_bytes, sdr_out, sdr_det, c1, stream);
    if (rc != IDV_OK) return rc;
    hipLaunchKernelGGL(bss_corr_kernel, dim3((unsigned)l.t1, B), dim3(256), 0, st, ref, ref_ld, interf, interf_ld, est, est_ld, lens, Lmax,
                       K, part1, (int)l.t1);
    hipLaunchKernelGGL(bss_solve_kernel, dim3(B), dim3(512), 0, st, part1, (int)l.t1, lens, Lmax, K, cw, status, filt);
    hipLaunchKernelGGL(bss_proj_kernel, dim3((unsigned)l.t3, B), dim3(256), 0, st, ref, ref_ld, interf, interf_ld, est, est_ld, lens, Lmax,
                       K, c1, cw, status, part3, (int)l.t3);
    hipLaunchKernelGGL(bss_final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, part3, (int)l.t3, status, sdr_out, sdr_det, lens, Lmax, K, B,
                       out, details);
    return idv_launch_status();
}
