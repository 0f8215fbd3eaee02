// Latent-space report on the device (latent.py): what the reference's two evaluation scripts compute per utterance on
// the host -- pretrained_vaes/test_prevae.py (posterior covariance entries, its KL form, the covariance of miu over the test set) and
// nsvae_dccrn/test_nsvae_se.py (posterior distances, the simplified silhouette score) -- for padded batches of any lengths.
//
// A latent is read in place from the planar LSTM output q[2][H][Jp] (F = 1): channel off + h, frame t of row b at
// q[(ri H + off + h) Jp + b Tp + t + 1].  Only frames t < frames[b] are read; guard columns never.
//
//   (a) row_stats_kernel / pair_dist_kernel   one wave per (row, channel); its lanes take the frames t = lane, lane + 64, ... (unit
//       stride in memory).  Elementwise values are fp32 with the reference's operations in the reference's order (no contraction into
//       fma), every sum is double: lane partials in increasing t, then the xor butterfly.  The *_final_kernel, one wave per row, adds
//       the channels h = lane, lane + 64 and runs the butterfly again.  The order depends on frames[b] and zdim alone: a row's bits do
//       not depend on the batch around it.
//   (b) miu moments: the frames are numbered g = b T + t and cut into chunks of MM_CH numbers (independent of Tp / Jp, so a copy of the
//       latent in another planar buffer gives the same bits).  mean_kernel: count and mean of every row of a chunk.  prod_kernel: the
//       32 x 32 blocks on and above the block diagonal of X X^T, X = the chunk's values centred on the chunk's mean with the invalid
//       columns zeroed, staged through LDS as double and multiplied on v_mfma_f64_16x16x4_f64 (one 16 x 16 tile per wave).
//       fold kernels: chunks in increasing order, then the state, by Chan's formula for co-moments.
//   (c) set_moments_kernel / sil_kernel / sil_final_kernel: column means and variances of a set of sampled latent vectors, the score
//       of every vector, and their mean.
// No atomics anywhere: the same sequence of calls gives the same bits.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct Lat {
    const float* q;
    int H, Jp, Tp, o_miu, o_ls, o_dl;
    __device__ __forceinline__ const float* re(int off, int h, int b) const { return q + (size_t)(off + h) * Jp + (size_t)b * Tp + 1; }
    __device__ __forceinline__ const float* im(int off, int h, int b) const { return q + (size_t)(H + off + h) * Jp + (size_t)b * Tp + 1; }
};

__device__ __forceinline__ int row_frames(const int* frames, int b, int T) { return frames ? min(max(frames[b], 1), T) : T; }

// test_prevae.py:25-43 and :45-69 for one (t, h), fp32 step by step
struct Elem {
    float vrr, vri, vii, kl_miu, kl_sig;
};
__device__ __forceinline__ Elem elem_stats(float mr, float mi, float ls, float dr, float di) {
#pragma clang fp contract(off)
    const float sg = expf(ls);
    const float a = sqrtf(dr * dr + di * di + 1e-6f);
    const float sc = sg * 0.99f / (a + 1e-6f);
    if (a >= sg - 1e-3f) {
        dr = dr * sc;
        di = di * sc;
    }
    Elem e;
    e.vrr = 0.5f * (sg + dr);
    e.vri = 0.5f * di;
    e.vii = 0.5f * (sg - dr);
    const float a2 = dr * dr + di * di;
    const float lg = logf(sg * sg - a2 + 1e-6f);
    e.kl_miu = mr * mr + mi * mi;
    e.kl_sig = fabsf(sg - 1.0f - 0.5f * lg);
    return e;
}

constexpr int RS_W = 10;            // per (row, channel): mean_t |vrr|, |vri|, |vii|, the channel's KL sum, then min / max of the three
constexpr int PD_W = 3;             // per (row, channel): the channel's share of dis_mean^2, dis_sigma^2, dis_delta^2

// grid (zdim / 4, B): one wave per channel of a row
__global__ __launch_bounds__(256) void row_stats_kernel(Lat q, int zdim, const int* __restrict__ frames, int T, double* __restrict__ work) {
    const int b = blockIdx.y, h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n = row_frames(frames, b, T);
    const float* mr = q.re(q.o_miu, h, b);
    const float* mi = q.im(q.o_miu, h, b);
    const float* ls = q.re(q.o_ls, h, b);
    const float* dr = q.re(q.o_dl, h, b);
    const float* di = q.im(q.o_dl, h, b);
    double kl = 0, a[3] = {0, 0, 0};
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = lane; t < n; t += 64) {
        const Elem e = elem_stats(mr[t], mi[t], ls[t], dr[t], di[t]);
        const float v[3] = {e.vrr, e.vri, e.vii};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] += (double)fabsf(v[k]);
            mn[k] = fminf(mn[k], v[k]);
            mx[k] = fmaxf(mx[k], v[k]);
        }
        kl += (double)e.kl_miu + (double)e.kl_sig;
    }
    kl = wave_sum_d(kl);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = wave_sum_d(a[k]) / (double)n;                        // mean_t |v| of this channel
        mn[k] = wave_min(mn[k]);
        mx[k] = wave_max(mx[k]);
    }
    if (lane == 0) {
        double* o = work + ((size_t)b * zdim + h) * RS_W;
        for (int k = 0; k < 3; ++k) {
            o[k] = a[k];
            o[4 + 2 * k] = (double)mn[k];
            o[5 + 2 * k] = (double)mx[k];
        }
        o[3] = kl;
    }
}

// grid (B), one wave: the channels h = lane, lane + 64 in this order, then the butterfly
__global__ __launch_bounds__(64) void row_stats_final_kernel(const double* __restrict__ work, int zdim, const int* __restrict__ frames,
                                                             int T, double* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = row_frames(frames, b, T);
    double kl = 0, s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0}, mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int h = lane; h < zdim; h += 64) {
        const double* o = work + ((size_t)b * zdim + h) * RS_W;
        kl += o[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s1[k] += o[k];
            s2[k] += o[k] * o[k];
            mn[k] = fmin(mn[k], o[4 + 2 * k]);
            mx[k] = fmax(mx[k], o[5 + 2 * k]);
        }
    }
    kl = wave_sum_d(kl);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s1[k] = wave_sum_d(s1[k]);
        s2[k] = wave_sum_d(s2[k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[k] = fmin(mn[k], __shfl_xor(mn[k], o, 64));
            mx[k] = fmax(mx[k], __shfl_xor(mx[k], o, 64));
        }
    }
    if (lane == 0) {
        double* o = out + (size_t)b * 13;
        o[0] = kl / (double)n;
        for (int k = 0; k < 3; ++k) {
            o[1 + 4 * k] = mn[k];
            o[2 + 4 * k] = mx[k];
            o[3 + 4 * k] = s1[k] / (double)zdim;
            o[4 + 4 * k] = sqrt(s2[k]);
        }
    }
}

__device__ __forceinline__ float sqdiff(float a, float b) {
#pragma clang fp contract(off)
    const float d = a - b;
    return d * d;
}

// grid (zdim / 4, B): one wave per channel of a row
__global__ __launch_bounds__(256) void pair_dist_kernel(Lat qa, Lat qb, int zdim, const int* __restrict__ frames, int T,
                                                        double* __restrict__ work) {
    const int b = blockIdx.y, h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n = row_frames(frames, b, T);
    const float* amr = qa.re(qa.o_miu, h, b); const float* ami = qa.im(qa.o_miu, h, b);
    const float* bmr = qb.re(qb.o_miu, h, b); const float* bmi = qb.im(qb.o_miu, h, b);
    const float* als = qa.re(qa.o_ls, h, b);  const float* bls = qb.re(qb.o_ls, h, b);
    const float* adr = qa.re(qa.o_dl, h, b);  const float* adi = qa.im(qa.o_dl, h, b);
    const float* bdr = qb.re(qb.o_dl, h, b);  const float* bdi = qb.im(qb.o_dl, h, b);
    double s[5] = {0, 0, 0, 0, 0};
    for (int t = lane; t < n; t += 64) {
        s[0] += (double)sqdiff(amr[t], bmr[t]);
        s[1] += (double)sqdiff(ami[t], bmi[t]);
        s[2] += (double)sqdiff(expf(als[t]), expf(bls[t]));
        s[3] += (double)sqdiff(adr[t], bdr[t]);
        s[4] += (double)sqdiff(adi[t], bdi[t]);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = wave_sum_d(s[k]) / (double)n;
    if (lane == 0) {
        double* o = work + ((size_t)b * zdim + h) * PD_W;
        o[0] = s[0] + s[1];
        o[1] = s[2];
        o[2] = s[3] + s[4];
    }
}

// grid (B), one wave: the channels h = lane, lane + 64 in this order, then the butterfly
__global__ __launch_bounds__(64) void pair_dist_final_kernel(const double* __restrict__ work, int zdim, double* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double acc[3] = {0, 0, 0};
    for (int h = lane; h < zdim; h += 64)
        for (int k = 0; k < 3; ++k) acc[k] += work[((size_t)b * zdim + h) * PD_W + k];
    for (int k = 0; k < 3; ++k) {
        const double v = wave_sum_d(acc[k]);
        if (lane == 0) out[(size_t)b * 3 + k] = sqrt(v);
    }
}

// ---------------------------------------------------------------------------------------------------------------- miu moments
constexpr int MM_CH = 512;          // frame numbers per chunk
constexpr int MM_KS = 64;           // columns staged per step
constexpr int MM_LD = MM_KS + 1;    // LDS row pitch in doubles (odd: the 16 rows of an operand fall into different banks)

struct Src {
    const float* q;
    int H, Jp, Tp, off, zdim;
    // row r of the 2 zdim rows: real channels, then imaginary channels
    __device__ __forceinline__ const float* row(int r) const {
        const int ri = r >= zdim, h = r - ri * zdim;
        return q + (size_t)(ri * H + off + h) * Jp;
    }
};

// frame number g = b T + t -> its column in the planar buffer, or -1 when it is not a valid frame
__device__ __forceinline__ long long frame_col(long long g, long long G, int T, int Tp, const int* frames) {
    if (g >= G) return -1;
    const int b = (int)(g / T), t = (int)(g - (long long)b * T);
    return t < row_frames(frames, b, T) ? (long long)b * Tp + t + 1 : -1;
}

// layout of a partial and of the state: n, mean[R], C[R][R]  (R = 2 zdim)
__device__ __forceinline__ size_t mm_stride(int R) { return 1 + (size_t)R + (size_t)R * R; }

// grid (nch, R / 16): count and mean of 16 rows (four per wave) over the chunk's valid frames
__global__ __launch_bounds__(256) void mm_mean_kernel(Src x, const int* __restrict__ frames, int B, int T, double* __restrict__ part) {
    const int ch = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, R = 2 * x.zdim;
    const long long G = (long long)B * T;
    long long col[MM_CH / 64];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < MM_CH / 64; ++k) {
        col[k] = frame_col((long long)ch * MM_CH + k * 64 + lane, G, T, x.Tp, frames);
        cnt += col[k] >= 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    double* o = part + (size_t)ch * mm_stride(R);
    if (threadIdx.x == 0 && blockIdx.y == 0) o[0] = (double)cnt;
    for (int r = blockIdx.y * 16 + w; r < blockIdx.y * 16 + 16; r += 4) {
        const float* p = x.row(r);
        double s = 0;
#pragma unroll
        for (int k = 0; k < MM_CH / 64; ++k)
            if (col[k] >= 0) s += (double)p[col[k]];
        s = wave_sum_d(s);
        if (lane == 0) o[1 + r] = cnt > 0 ? s / (double)cnt : 0.0;
    }
}

// grid (block pairs bi <= bj, nch): C[bi 32 .. +32][bj 32 .. +32] of the chunk
__global__ __launch_bounds__(256) void mm_prod_kernel(Src x, const int* __restrict__ frames, int B, int T, double* __restrict__ part) {
    __shared__ double sA[32 * MM_LD], sB[32 * MM_LD];
    const int R = 2 * x.zdim, nb = R / 32, ch = blockIdx.y;
    int bi = 0, rest = blockIdx.x;                                  // blockIdx.x enumerates (bi, bj >= bi) row by row
    while (rest >= nb - bi) {
        rest -= nb - bi;
        ++bi;
    }
    const int bj = bi + rest;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long G = (long long)B * T;
    double* o = part + (size_t)ch * mm_stride(R);
    const double* mean = o + 1;
    const int kc = threadIdx.x & 63, r0 = threadIdx.x >> 6;         // staging: column kc of the step, rows r0, r0 + 4, ...
    const int wr = w >> 1, wc = w & 1;                              // the wave's 16 x 16 tile of the 32 x 32 block
    f64x4 acc = {0, 0, 0, 0};
    for (int k0 = 0; k0 < MM_CH; k0 += MM_KS) {
        const long long col = frame_col((long long)ch * MM_CH + k0 + kc, G, T, x.Tp, frames);
        __syncthreads();                                            // the previous step's operands have been read
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = r0 + 4 * q, ra = bi * 32 + r, rb = bj * 32 + r;
            sA[r * MM_LD + kc] = col >= 0 ? (double)x.row(ra)[col] - mean[ra] : 0.0;
            sB[r * MM_LD + kc] = col >= 0 ? (double)x.row(rb)[col] - mean[rb] : 0.0;
        }
        __syncthreads();
        // A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15] = X_bj[j][k]: D = X_bi X_bj^T
        const double* pa = sA + (wr * 16 + (lane & 15)) * MM_LD + (lane >> 4);
        const double* pb = sB + (wc * 16 + (lane & 15)) * MM_LD + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < MM_KS; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], pb[kk], acc, 0, 0, 0);
    }
    // f64 C/D layout: column lane & 15, row (lane >> 4) + 4 reg
    double* C = o + 1 + R;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int i = bi * 32 + wr * 16 + (lane >> 4) + 4 * reg, j = bj * 32 + wc * 16 + (lane & 15);
        C[(size_t)i * R + j] = acc[reg];
    }
}

// One thread per element (i, j) of the blocks on and above the block diagonal: fold the nch partials (or another state) into the state's
// C[i][j].  Every thread carries the running n, mean[i], mean[j] itself; the state's n and mean are written by mm_fold_mean_kernel,
// launched behind this one.
__global__ __launch_bounds__(256) void mm_fold_cov_kernel(const double* __restrict__ part, int nch, int R, double* __restrict__ state) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= R * R) return;
    const int i = e / R, j = e - i * R;
    if ((i >> 5) > (j >> 5)) return;
    double na = state[0], mi = state[1 + i], mj = state[1 + j], Ca = state[1 + R + e];
    const size_t st = 1 + (size_t)R + (size_t)R * R;
    for (int c = 0; c < nch; ++c) {
        const double* o = part + (size_t)c * st;
        const double nb = o[0];
        if (nb == 0) continue;
        if (na == 0) {
            na = nb;
            mi = o[1 + i];
            mj = o[1 + j];
            Ca = o[1 + R + e];
            continue;
        }
        const double n = na + nb, di = o[1 + i] - mi, dj = o[1 + j] - mj;
        Ca += o[1 + R + e] + di * dj * (na * (nb / n));
        mi += di * (nb / n);
        mj += dj * (nb / n);
        na = n;
    }
    state[1 + R + e] = Ca;
}

__global__ __launch_bounds__(256) void mm_fold_mean_kernel(const double* __restrict__ part, int nch, int R, double* __restrict__ state) {
    const int r = threadIdx.x;
    const double n0 = state[0];
    double na = n0, m = r < R ? state[1 + r] : 0.0;
    const size_t st = 1 + (size_t)R + (size_t)R * R;
    for (int c = 0; c < nch; ++c) {
        const double* o = part + (size_t)c * st;
        const double nb = o[0];
        if (nb == 0) continue;
        if (na == 0) {
            na = nb;
            m = r < R ? o[1 + r] : 0.0;
            continue;
        }
        const double n = na + nb;
        if (r < R) m += (o[1 + r] - m) * (nb / n);
        na = n;
    }
    __syncthreads();                                                // every thread has read state[0]
    if (r < R) state[1 + r] = m;
    if (r == 0) state[0] = na;
}

// ---------------------------------------------------------------------------------------------------------------- sampled sets
// grid (D / 16), 1024 threads: thread (g, c) sums the rows n = g, g + 64, ... of column 16 blockIdx + c; the 64 groups are added in order
__global__ __launch_bounds__(1024) void set_moments_kernel(const float* __restrict__ x, int N, int D, double* __restrict__ mom) {
    __shared__ double sh[64][17];
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4, d = blockIdx.x * 16 + c;
    double s = 0;
    for (int n = g; n < N; n += 64) s += (double)x[(size_t)n * D + d];
    sh[g][c] = s;
    __syncthreads();
    double mean = 0;
    for (int k = 0; k < 64; ++k) mean += sh[k][c];
    mean /= (double)N;
    __syncthreads();
    double v = 0;
    for (int n = g; n < N; n += 64) {
        const double e = (double)x[(size_t)n * D + d] - mean;
        v += e * e;
    }
    sh[g][c] = v;
    __syncthreads();
    if (g == 0) {
        double var = 0;
        for (int k = 0; k < 64; ++k) var += sh[k][c];
        mom[d] = mean;
        mom[D + d] = var / (double)N;
    }
}

// one wave per vector: its distance to its own set's mean and to the other set's, and the score of test_nsvae_se.py:42-47
__global__ __launch_bounds__(256) void sil_kernel(const float* __restrict__ x1, int N1, const float* __restrict__ x2, int N2, int D,
                                                  const double* __restrict__ mom1, const double* __restrict__ mom2,
                                                  double* __restrict__ score) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= N1 + N2) return;
    const bool first = v < N1;
    const float* x = first ? x1 + (size_t)v * D : x2 + (size_t)(v - N1) * D;
    const double* own = first ? mom1 : mom2;
    const double* oth = first ? mom2 : mom1;
    double a = 0, e = 0;
    for (int d = lane; d < D; d += 64) {
        const double xv = (double)x[d], da = xv - own[d], de = xv - oth[d];
        a += da * da;
        e += de * de;
    }
    const double intra = sqrt(wave_sum_d(a)), inter = sqrt(wave_sum_d(e));
    if (lane == 0) score[v] = (inter - intra) / fmax(intra, inter);
}

__global__ __launch_bounds__(256) void sil_final_kernel(const double* __restrict__ score, int N, int D, const double* __restrict__ mom1,
                                                        const double* __restrict__ mom2, double* __restrict__ out) {
    __shared__ double sh[4];
    double s = 0;
    for (int n = threadIdx.x; n < N; n += 256) s += score[n];
    s = waves_sum<4>(s, sh);
    if (threadIdx.x != 0) return;
    out[0] = s / (double)N;
    double md = 0, var[4] = {0, 0, 0, 0};
    for (int d = 0; d < D; ++d) {
        const double c = mom1[d] - mom2[d];
        md += c * c;
        var[d & 1] += mom1[D + d];
        var[2 + (d & 1)] += mom2[D + d];
    }
    out[1] = md;
    for (int k = 0; k < 4; ++k) out[2 + k] = var[k] / (double)(D / 2);
}

bool zdim_ok(int zdim) { return zdim >= 16 && zdim <= 128 && zdim % 16 == 0; }

// frame t < T of row b < B sits in column b Tp + t + 1 < B Tp <= Jp of its plane: every read stays inside the 2 H Jp floats
bool lat_ok(const float* q, int H, int Jp, int Tp, int B, int T) {
    return q && H > 0 && T >= 1 && Tp >= T + 1 && B >= 1 && B <= 65535 && (long long)B * Tp <= (long long)Jp;
}
bool f64_ok(const void* a, const void* b) { return a && b && !((uintptr_t)a & 7) && !((uintptr_t)b & 7); }
bool off_ok(int off, int zdim, int H) { return off >= 0 && off + zdim <= H; }

}  // namespace

extern "C" int idv_latent_row_stats(const float* q, int H, int Jp, int Tp, int off_miu, int off_ls, int off_dl, int zdim,
                                    const int* frames, int B, int T, double* work, double* out, void* stream) {
    if (!f64_ok(work, out) || !zdim_ok(zdim) || !lat_ok(q, H, Jp, Tp, B, T) || !off_ok(off_miu, zdim, H) || !off_ok(off_ls, zdim, H) ||
        !off_ok(off_dl, zdim, H))
        return IDV_EINVAL;
    const Lat l{q, H, Jp, Tp, off_miu, off_ls, off_dl};
    hipLaunchKernelGGL(row_stats_kernel, dim3(zdim / 4, B), dim3(256), 0, (hipStream_t)stream, l, zdim, frames, T, work);
    hipLaunchKernelGGL(row_stats_final_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)work, zdim, frames, T, out);
    return idv_launch_status();
}

extern "C" int idv_latent_pair_dist(const float* qa, int Ha, int Jpa, int Tpa, int oa_miu, int oa_ls, int oa_dl, const float* qb, int Hb,
                                    int Jpb, int Tpb, int ob_miu, int ob_ls, int ob_dl, int zdim, const int* frames, int B, int T,
                                    double* work, double* out, void* stream) {
    if (!f64_ok(work, out) || !zdim_ok(zdim) || !lat_ok(qa, Ha, Jpa, Tpa, B, T) || !lat_ok(qb, Hb, Jpb, Tpb, B, T) ||
        !off_ok(oa_miu, zdim, Ha) || !off_ok(oa_ls, zdim, Ha) || !off_ok(oa_dl, zdim, Ha) || !off_ok(ob_miu, zdim, Hb) ||
        !off_ok(ob_ls, zdim, Hb) || !off_ok(ob_dl, zdim, Hb))
        return IDV_EINVAL;
    const Lat a{qa, Ha, Jpa, Tpa, oa_miu, oa_ls, oa_dl}, b{qb, Hb, Jpb, Tpb, ob_miu, ob_ls, ob_dl};
    hipLaunchKernelGGL(pair_dist_kernel, dim3(zdim / 4, B), dim3(256), 0, (hipStream_t)stream, a, b, zdim, frames, T, work);
    hipLaunchKernelGGL(pair_dist_final_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)work, zdim, out);
    return idv_launch_status();
}

extern "C" int idv_miu_moments_chunk(void) { return MM_CH; }

extern "C" long long idv_miu_moments_work_bytes(int zdim, int B, int T) {
    if (!zdim_ok(zdim) || B < 1 || B > 65535 || T < 1 || (long long)B * T > 2147483647LL - MM_CH) return -1;
    const long long nch = ((long long)B * T + MM_CH - 1) / MM_CH, R = 2 * zdim;
    if (nch > 65535) return -1;
    return nch * (1 + R + R * R) * (long long)sizeof(double);
}

extern "C" int idv_miu_moments_update(const float* q, int H, int Jp, int Tp, int off_miu, int zdim, const int* frames, int B, int T,
                                      double* state, void* work, long long work_bytes, void* stream) {
    const long long need = idv_miu_moments_work_bytes(zdim, B, T);
    if (need < 0 || work_bytes < need || !f64_ok(work, state) || !lat_ok(q, H, Jp, Tp, B, T) || !off_ok(off_miu, zdim, H))
        return IDV_EINVAL;
    const int nch = (int)(((long long)B * T + MM_CH - 1) / MM_CH), R = 2 * zdim, nb = R / 32;
    const Src x{q, H, Jp, Tp, off_miu, zdim};
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)work;
    hipLaunchKernelGGL(mm_mean_kernel, dim3(nch, R / 16), dim3(256), 0, st, x, frames, B, T, part);
    hipLaunchKernelGGL(mm_prod_kernel, dim3(nb * (nb + 1) / 2, nch), dim3(256), 0, st, x, frames, B, T, part);
    hipLaunchKernelGGL(mm_fold_cov_kernel, dim3((R * R + 255) / 256), dim3(256), 0, st, (const double*)part, nch, R, state);
    hipLaunchKernelGGL(mm_fold_mean_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nch, R, state);
    return idv_launch_status();
}

extern "C" int idv_miu_moments_merge(double* state, const double* other, int zdim, void* stream) {
    if (!state || !other || state == other || !zdim_ok(zdim) || ((uintptr_t)state & 7) || ((uintptr_t)other & 7)) return IDV_EINVAL;
    const int R = 2 * zdim;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mm_fold_cov_kernel, dim3((R * R + 255) / 256), dim3(256), 0, st, other, 1, R, state);
    hipLaunchKernelGGL(mm_fold_mean_kernel, dim3(1), dim3(256), 0, st, other, 1, R, state);
    return idv_launch_status();
}

extern "C" int idv_latent_set_moments(const float* x, int N, int D, double* mom, void* stream) {
    if (!x || !mom || ((uintptr_t)mom & 7) || N < 1 || D < 32 || D > 256 || D % 32 || (long long)N * D > 2147483647LL) return IDV_EINVAL;
    hipLaunchKernelGGL(set_moments_kernel, dim3(D / 16), dim3(1024), 0, (hipStream_t)stream, x, N, D, mom);
    return idv_launch_status();
}

extern "C" int idv_latent_silhouette(const float* x1, int N1, const float* x2, int N2, int D, const double* mom1, const double* mom2,
                                     double* work, double* out, void* stream) {
    if (!x1 || !x2 || !mom1 || !mom2 || !work || !out || ((uintptr_t)work & 7) || ((uintptr_t)out & 7) || ((uintptr_t)mom1 & 7) ||
        ((uintptr_t)mom2 & 7) || N1 < 1 || N2 < 1 || D < 32 || D > 256 || D % 32 || ((long long)N1 + N2) * D > 2147483647LL)
        return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int N = N1 + N2;
    hipLaunchKernelGGL(sil_kernel, dim3((N + 3) / 4), dim3(256), 0, st, x1, N1, x2, N2, D, mom1, mom2, work);
    hipLaunchKernelGGL(sil_final_kernel, dim3(1), dim3(256), 0, st, (const double*)work, N, D, mom1, mom2, out);
    return idv_launch_status();
}
