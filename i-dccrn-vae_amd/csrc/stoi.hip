// STOI / ESTOI (Taal et al. 2011, Jensen & Taal 2016, with the constants and the framing of the pystoi package) and the scaled RMSE
// of utils/eval_metrics.py:33-41 for a padded batch of utterances of different lengths: inference.compute_stoi / compute_rmse.
//
//   (a) resample_kernel      16 kHz -> 10 kHz, out[n] = 5 sum_j x[j] h[290 + 8n - 5j] (scipy.signal.resample_poly(x, 5, 8, window=h)),
//                            both signals in one launch, fp32 taps and samples, double accumulator
//   (b) energy_kernel        e_i = 20 log10(|w x_i| + EPS) of the clean signal's frames, one wave per frame
//       mask_kernel          per row: max, keep mask, in-kernel prefix sum -> list of kept frame indices, K_b, counts
//   (c) spec_band_kernel     32 second-stage frames per workgroup rebuilt in LDS from the kept windowed frames (frame j = w * (kept j +
//                            tail half of kept j-1 + head half of kept j+1): the overlap-added signal is never written), the
//                            256 -> bins 7..230 DFT on v_mfma_f32_32x32x2_f32 (7 bin tiles x re/im, K = 256), and in the epilogue
//                            |X|^2 -> LDS -> third-octave band sums -> sqrt: 15 floats per frame reach memory
//   (d) segment_kernel       one workgroup per (row, run of 32 segments): the 15 x 61 band tile in LDS, eight segments at a time (one
//                            per half wave) in double; per-run partials, folded per row in a fixed order by final_kernel
//
// Row b reads nothing at or past lens[b] and nothing of another row, every sum has a fixed order and there is no atomic: a row's
// result does not depend on B, on the other rows or on the padding.  Tables (taps, window, DFT matrix, band edges) are formed in
// double by table_kernel once per device, on the stream of the first call; later calls wait for that launch's event until it has
// been seen complete.  No allocation, no host synchronisation.
#include <mutex>
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int NTAP = 581, HALF = 290, NW = 256, HOP = 128, NBAND = 15, NSEG = 30;
constexpr int BIN0 = 7, NTILE = 7, KSTEPS = NW / 2;       // bins 7 .. 230 in 7 tiles of 32 (219 .. 230 are computed and unused)
constexpr int FPW = 32;                                   // frames per spec_band workgroup
constexpr int YLD = NW + 1;                               // LDS pitch of a staged frame
constexpr int RUN = 32, SLOTS = 8, TCOLS = RUN + NSEG - 1; // segments per segment workgroup, at a time, band-tile columns
constexpr double EPS = 2.220446049250313e-16;

struct Tables {
    float h[NTAP + 3];
    float w[NW];
    int lo[NBAND], hi[NBAND];
    float dft[NTILE * 2 * KSTEPS * 64];                   // [tile][re | im][k step][lane]: the A operand as the lanes read it
};
__device__ Tables g_tab;

__device__ double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((double)k * k);
        sum += term;
    }
    return sum;
}

__global__ __launch_bounds__(256) void table_kernel() {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
    for (int idx = gid; idx < NTILE * 2 * KSTEPS * 64; idx += gsz) {
        const int lane = idx & 63, ks = (idx >> 6) % KSTEPS, part = (idx / (64 * KSTEPS)) & 1, tile = idx / (64 * KSTEPS * 2);
        const int bin = BIN0 + 32 * tile + (lane & 31), n = 2 * ks + (lane >> 5);
        const double ph = (double)((bin * n) & 511) / 256.0;               // exact phase reduction
        g_tab.dft[idx] = (float)(part == 0 ? cospi(ph) : sinpi(ph));
    }
    if (blockIdx.x != 0) return;
    __shared__ double hraw[NTAP];
    __shared__ double hsum;
    const double beta = 0.1102 * (60 - 8.7), fc = 1.0 / 16;
    for (int k = threadIdx.x; k < NTAP; k += blockDim.x) {
        const double t = k - HALF, r = t / HALF;
        const double kais = bessel_i0(beta * sqrt(fmax(0.0, 1.0 - r * r))) / bessel_i0(beta);
        const double a = 2 * fc * t;
        const double sinc = k == HALF ? 1.0 : sinpi(a) / (3.14159265358979323846 * a);
        hraw[k] = kais * (2 * 5 * fc * sinc);
    }
    if (threadIdx.x < NW) g_tab.w[threadIdx.x] = (float)(0.5 - 0.5 * cospi(2.0 * (threadIdx.x + 1) / (NW + 1)));   // hanning(258)[1:-1]
    if (threadIdx.x < NBAND) {                            // the bins nearest to 150 * 2^((2i -+ 1) / 6) Hz
        for (int side = 0; side < 2; ++side) {
            const double f = 150.0 * pow(2.0, (2 * (int)threadIdx.x + (side ? 1 : -1)) / 6.0);
            int best = 0;
            double bd = f * f;
            for (int k = 1; k <= 256; ++k) {
                const double d = k * (10000.0 / 512) - f;
                if (d * d < bd) { bd = d * d; best = k; }
            }
            best = min(max(best, BIN0), BIN0 + 32 * NTILE);
            (side ? g_tab.hi : g_tab.lo)[threadIdx.x] = best;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0;
        for (int k = 0; k < NTAP; ++k) s += hraw[k];
        hsum = s;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NTAP + 3; k += blockDim.x) g_tab.h[k] = k < NTAP ? (float)(hraw[k] / hsum) : 0.f;
}

// ---- row geometry
__host__ __device__ __forceinline__ int n10_of(int L, int fs16) { return fs16 ? (int)((5LL * L + 7) / 8) : L; }
__host__ __device__ __forceinline__ int frames_of(int n) { return n > NW ? (n - NW + HOP - 1) / HOP : 0; }   // len(range(0, n - 256, 128))
__device__ __forceinline__ int floor_div(int a, int d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }

// (a) grid (ceil(N10max / 256), B, 2): z = 0 the clean signal, 1 the estimate
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ ref, long long ref_ld, const float* __restrict__ est,
                                                       long long est_ld, const int* __restrict__ lens, int Lmax, float* __restrict__ rs,
                                                       long long rs_ld, int B) {
    __shared__ float hs[NTAP + 3];
    __shared__ float xs[528];
    const int b = blockIdx.y, s = blockIdx.z;
    const int L = row_len(lens, b, Lmax), n10 = n10_of(L, 1), n0 = blockIdx.x * 256;
    if (n0 >= n10) return;
    const float* x = s ? est + (size_t)b * est_ld : ref + (size_t)b * ref_ld;
    const int jbase = floor_div(8 * n0 - HALF, 5);
    for (int k = threadIdx.x; k < NTAP + 3; k += 256) hs[k] = g_tab.h[k];
    for (int k = threadIdx.x; k < 528; k += 256) {
        const int j = jbase + k;
        xs[k] = (j >= 0 && j < L) ? x[j] : 0.f;
    }
    __syncthreads();
    const int n = n0 + threadIdx.x;
    if (n >= n10) return;
    const int jlo = -floor_div(HALF - 8 * n, 5), jhi = floor_div(8 * n + HALF, 5);     // 0 <= 290 + 8n - 5j <= 580
    double acc = 0;
    for (int j = jlo; j <= jhi; ++j) acc += (double)xs[j - jbase] * (double)hs[HALF + 8 * n - 5 * j];
    rs[((size_t)s * B + b) * rs_ld + n] = (float)(5.0 * acc);
}

// (b) grid (ceil(Fmax / 4), B): one wave per frame of the clean signal
__global__ __launch_bounds__(256) void energy_kernel(const float* __restrict__ x, long long ld, const int* __restrict__ lens, int Lmax,
                                                     int fs16, double* __restrict__ en, int Fp) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int F = frames_of(n10_of(row_len(lens, b, Lmax), fs16));
    if (i >= F) return;
    const float* r = x + (size_t)b * ld + (size_t)i * HOP;
    double s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float p = g_tab.w[lane + 64 * q] * r[lane + 64 * q];
        s += (double)p * p;
    }
    s = wave_sum_d(s);
    if (lane == 0) en[(size_t)b * Fp + i] = 20.0 * log10(sqrt(s) + EPS);
}

// grid B: keep frame i iff max(e) - 40 - e_i < 0; kept[b][0 .. K_b - 1] = the kept i in increasing order
__global__ __launch_bounds__(256) void mask_kernel(const double* __restrict__ en, const int* __restrict__ lens, int Lmax, int fs16, int Fp,
                                                   int* __restrict__ kept, int* __restrict__ Kc, int* __restrict__ counts) {
    __shared__ double shm[4];
    __shared__ int shc[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int F = frames_of(n10_of(row_len(lens, b, Lmax), fs16));
    const double* e = en + (size_t)b * Fp;
    double m = -INFINITY;
    for (int i = threadIdx.x; i < F; i += 256) m = fmax(m, e[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) shm[wv] = m;
    __syncthreads();
    m = fmax(fmax(shm[0], shm[1]), fmax(shm[2], shm[3]));
    int base = 0;
    for (int i0 = 0; i0 < F; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < F && (m - 40.0 - e[i]) < 0;
        const unsigned long long bal = __ballot(keep);
        const int below = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();                                   // shc of the previous chunk has been read
        if (lane == 0) shc[wv] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int q = 0; q < wv; ++q) off += shc[q];
        if (keep) kept[(size_t)b * Fp + off + below] = i;
        base += shc[0] + shc[1] + shc[2] + shc[3];
    }
    if (threadIdx.x == 0) {
        Kc[b] = base;
        if (counts) {
            counts[b * 3] = F;
            counts[b * 3 + 1] = base;
            counts[b * 3 + 2] = base - 1 >= NSEG ? base - NSEG : 0;
        }
    }
}

// (c) grid (ceil((Fmax - 1) / 32), B, 2): second-stage frames j0 .. j0 + 31 of signal z of row b -> tob[z][b][15][Fp]
__global__ __launch_bounds__(256) void spec_band_kernel(const float* __restrict__ x0, long long ld0, const float* __restrict__ x1,
                                                        long long ld1, const int* __restrict__ kept, const int* __restrict__ Kc, int Fp,
                                                        int B, float* __restrict__ tob) {
    __shared__ float sh[FPW * YLD];                        // the staged frames [frame][n], then |X|^2 [bin - 7][frame]
    __shared__ int sidx[FPW + 2];
    const int b = blockIdx.y, s = blockIdx.z, j0 = blockIdx.x * FPW;
    const int nfr = Kc[b] - 1;
    if (j0 >= nfr) return;
    const float* r = s ? x1 + (size_t)b * ld1 : x0 + (size_t)b * ld0;
    if (threadIdx.x < FPW + 2) {
        const int j = j0 - 1 + (int)threadIdx.x;
        sidx[threadIdx.x] = (j >= 0 && j <= nfr) ? kept[(size_t)b * Fp + j] : -1;
    }
    __syncthreads();
    {
        const int n = threadIdx.x;
        const float wn = g_tab.w[n], wo = g_tab.w[n ^ HOP];
        for (int c = 0; c < FPW; ++c) {
            float y = 0.f;
            if (j0 + c < nfr) {
                const int other = n < HOP ? sidx[c] : sidx[c + 2];              // kept j - 1 (its tail half) / kept j + 1 (its head half)
                float v = wn * r[(size_t)sidx[c + 1] * HOP + n];
                if (other >= 0) v += wo * r[(size_t)other * HOP + (n ^ HOP)];
                y = wn * v;
            }
            sh[c * YLD + n] = y;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ntile = wv + 4 < NTILE ? 2 : 1;               // wave wv: bin tiles wv and wv + 4
    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][p][q] = 0.f;
    const float* yb = sh + (lane & 31) * YLD + (lane >> 5);
    const float* a0 = g_tab.dft + (size_t)(wv * 2) * KSTEPS * 64 + lane;
    const float* a1 = g_tab.dft + (size_t)((wv + 4) * 2) * KSTEPS * 64 + lane;
#pragma unroll 4
    for (int ks = 0; ks < KSTEPS; ++ks) {
        const float bv = yb[2 * ks];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[ks * 64], bv, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[(KSTEPS + ks) * 64], bv, acc[0][1], 0, 0, 0);
        if (ntile == 2) {
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[ks * 64], bv, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[(KSTEPS + ks) * 64], bv, acc[1][1], 0, 0, 0);
        }
    }
    __syncthreads();                                       // every wave has read its frames: sh becomes |X|^2
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (t < ntile) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = 32 * (wv + 4 * t) + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                const float re = acc[t][0][q], im = acc[t][1][q];
                sh[row * FPW + (lane & 31)] = re * re + im * im;
            }
        }
    }
    __syncthreads();
    for (int item = threadIdx.x; item < NBAND * FPW; item += 256) {
        const int band = item >> 5, c = item & 31;
        if (j0 + c >= nfr) continue;
        double sum = 0;
        for (int k = g_tab.lo[band]; k < g_tab.hi[band]; ++k) sum += (double)sh[(k - BIN0) * FPW + c];
        tob[(((size_t)s * B + b) * NBAND + band) * Fp + j0 + c] = (float)sqrt(sum);
    }
}

// (d) grid (ceil((Fmax - 30) / 32), B): segments blockIdx.x * 32 .. + 31 of row b (segment g = band columns g .. g + 29)
__global__ __launch_bounds__(256) void segment_kernel(const float* __restrict__ tob, const int* __restrict__ Kc, int Fp, int B, int extended,
                                                      double* __restrict__ part, int nblk) {
    __shared__ float tile[2][NBAND][TCOLS + 3];
    __shared__ double mu[SLOTS][2][NBAND], nrm[SLOTS][2][NBAND];
    __shared__ double dsh[SLOTS][32];
    __shared__ double segv[RUN];
    const int b = blockIdx.y, g0 = blockIdx.x * RUN;
    const int nfr = Kc[b] - 1;
    const int M = nfr >= NSEG ? nfr - NSEG + 1 : 0;
    if (g0 >= M) return;
    for (int k = threadIdx.x; k < 2 * NBAND * TCOLS; k += 256) {
        const int c = k % TCOLS, band = (k / TCOLS) % NBAND, s = k / (TCOLS * NBAND);
        tile[s][band][c] = g0 + c < nfr ? tob[(((size_t)s * B + b) * NBAND + band) * Fp + g0 + c] : 0.f;
    }
    __syncthreads();
    const int slot = threadIdx.x >> 5, sub = threadIdx.x & 31;
    for (int pass = 0; pass < RUN / SLOTS; ++pass) {
        const int c0 = pass * SLOTS + slot;                // first band column of this half wave's segment, relative to g0
        if (extended) {
            if (sub < 2 * NBAND) {                         // rows: mean and norm over the 30 frames
                const int s = sub / NBAND, band = sub % NBAND;
                const float* v = &tile[s][band][c0];
                double m = 0, ss = 0;
                for (int t = 0; t < NSEG; ++t) m += (double)v[t];
                m /= NSEG;
                for (int t = 0; t < NSEG; ++t) { const double d = (double)v[t] - m; ss += d * d; }
                mu[slot][s][band] = m;
                nrm[slot][s][band] = sqrt(ss) + EPS;
            }
            __syncthreads();
            if (sub < NSEG) {                              // columns: the row-normalised values, mean and norm over the 15 bands
                double xv[NBAND], yv[NBAND], mx = 0, my = 0, sx = 0, sy = 0, dot = 0;
#pragma unroll
                for (int k = 0; k < NBAND; ++k) {
                    xv[k] = ((double)tile[0][k][c0 + sub] - mu[slot][0][k]) / nrm[slot][0][k];
                    yv[k] = ((double)tile[1][k][c0 + sub] - mu[slot][1][k]) / nrm[slot][1][k];
                    mx += xv[k];
                    my += yv[k];
                }
                mx /= NBAND;
                my /= NBAND;
#pragma unroll
                for (int k = 0; k < NBAND; ++k) {
                    xv[k] -= mx;
                    yv[k] -= my;
                    sx += xv[k] * xv[k];
                    sy += yv[k] * yv[k];
                }
                const double nx = sqrt(sx) + EPS, ny = sqrt(sy) + EPS;
#pragma unroll
                for (int k = 0; k < NBAND; ++k) dot += (xv[k] / nx) * (yv[k] / ny);
                dsh[slot][sub] = dot;
            }
        } else {
            if (sub < NBAND) {                             // one band row: scale, clip, normalise, correlate
                const float* xr = &tile[0][sub][c0];
                const float* yr = &tile[1][sub][c0];
                const double clip = 1.0 + 5.623413251903491;     // 1 + 10^(15/20)
                double sxx = 0, syy = 0;
                for (int t = 0; t < NSEG; ++t) { sxx += (double)xr[t] * xr[t]; syy += (double)yr[t] * yr[t]; }
                const double c = sqrt(sxx) / (sqrt(syy) + EPS);
                double mx = 0, my = 0;
                for (int t = 0; t < NSEG; ++t) {
                    mx += (double)xr[t];
                    my += fmin(c * (double)yr[t], (double)xr[t] * clip);
                }
                mx /= NSEG;
                my /= NSEG;
                double vx = 0, vy = 0;
                for (int t = 0; t < NSEG; ++t) {
                    const double dx = (double)xr[t] - mx, dy = fmin(c * (double)yr[t], (double)xr[t] * clip) - my;
                    vx += dx * dx;
                    vy += dy * dy;
                }
                const double nx = sqrt(vx) + EPS, ny = sqrt(vy) + EPS;
                double dot = 0;
                for (int t = 0; t < NSEG; ++t) {
                    const double dx = (double)xr[t] - mx, dy = fmin(c * (double)yr[t], (double)xr[t] * clip) - my;
                    dot += (dx / nx) * (dy / ny);
                }
                dsh[slot][sub] = dot;
            }
        }
        __syncthreads();
        if (sub == 0) {
            double sum = 0;
            const int cnt = extended ? NSEG : NBAND;
            for (int k = 0; k < cnt; ++k) sum += dsh[slot][k];
            segv[c0] = g0 + c0 < M ? (extended ? sum / NSEG : sum) : 0.0;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double sum = 0;
        for (int k = 0; k < RUN; ++k) sum += segv[k];
        part[(size_t)b * nblk + blockIdx.x] = sum;
    }
}

__global__ void final_kernel(const double* __restrict__ part, const int* __restrict__ Kc, int nblk, int B, int extended,
                             float* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int nfr = Kc[b] - 1;
    if (nfr < NSEG) {
        out[b] = 1e-5f;
        return;
    }
    const int M = nfr - NSEG + 1, nb = (M + RUN - 1) / RUN;
    double sum = 0;
    for (int k = 0; k < nb; ++k) sum += part[(size_t)b * nblk + k];
    out[b] = (float)(extended ? sum / M : sum / ((double)NBAND * M));
}

// grid B: alpha = <e, r> / <e, e>; sqrt(mean((alpha e - r)^2)) over the first lens[b] samples, both passes in double
__global__ __launch_bounds__(1024) void rmse_kernel(const float* __restrict__ ref, long long ref_ld, const float* __restrict__ est,
                                                    long long est_ld, const int* __restrict__ lens, int Lmax, double* __restrict__ work,
                                                    float* __restrict__ out) {
    __shared__ double sh[16];
    const int b = blockIdx.x;
    const float* r = ref + (size_t)b * ref_ld;
    const float* e = est + (size_t)b * est_ld;
    const int L = max(0, min(lens[b], Lmax));
    double D = 0, Q = 0;
    for (int n = threadIdx.x; n < L; n += 1024) {
        const double ev = e[n];
        D += ev * (double)r[n];
        Q += ev * ev;
    }
    D = waves_sum<16, true>(D, sh);
    Q = waves_sum<16, true>(Q, sh);
    const double alpha = D / Q;
    double S = 0;
    for (int n = threadIdx.x; n < L; n += 1024) {
        const double d = alpha * (double)e[n] - (double)r[n];
        S += d * d;
    }
    S = waves_sum<16, true>(S, sh);
    if (threadIdx.x == 0) {
        work[b * 3] = D;
        work[b * 3 + 1] = Q;
        work[b * 3 + 2] = S;
        out[b] = (float)sqrt(S / L);
    }
}

// ---- host side
struct Layout {
    long long rs_ld, Fp, nblk;
    long long off_rs, off_en, off_kept, off_K, off_tob, off_part, bytes;
};

long long up(long long v, long long a) { return (v + a - 1) / a * a; }

Layout layout(int B, int Lmax, int fs) {
    Layout l;
    const int fs16 = fs == 16000;
    const int n10 = n10_of(Lmax, fs16), F = frames_of(n10);
    l.rs_ld = up(n10, 64);
    l.Fp = up(F > 0 ? F : 1, 32);
    l.nblk = F - NSEG > 0 ? (F - NSEG + RUN - 1) / RUN : 1;
    long long o = 0;
    l.off_rs = o;   o += up(fs16 ? 2LL * B * l.rs_ld * 4 : 0, 256);
    l.off_en = o;   o += up((long long)B * l.Fp * 8, 256);
    l.off_kept = o; o += up((long long)B * l.Fp * 4, 256);
    l.off_K = o;    o += up((long long)B * 4, 256);
    l.off_tob = o;  o += up(2LL * B * NBAND * l.Fp * 4, 256);
    l.off_part = o; o += up((long long)B * l.nblk * 8, 256);
    l.bytes = o;
    return l;
}

struct DevTables {
    int state = 0;                                         // 0: not launched, 1: launched, 2: seen complete
    hipEvent_t ev;
};
DevTables g_dev[64];
std::mutex g_mu;

int ensure_tables(hipStream_t st) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return IDV_EINVAL;
    std::lock_guard<std::mutex> lock(g_mu);
    DevTables& d = g_dev[dev];
    if (d.state == 2) return IDV_OK;
    if (d.state == 0) {
        if (hipEventCreateWithFlags(&d.ev, hipEventDisableTiming) != hipSuccess) return IDV_ELAUNCH;
        hipLaunchKernelGGL(table_kernel, dim3(112), dim3(256), 0, st);
        if (hipEventRecord(d.ev, st) != hipSuccess) return IDV_ELAUNCH;
        d.state = 1;
        return IDV_OK;
    }
    if (hipEventQuery(d.ev) == hipSuccess) {
        d.state = 2;
        return IDV_OK;
    }
    (void)hipGetLastError();                               // hipErrorNotReady is not a launch failure
    return hipStreamWaitEvent(st, d.ev, 0) == hipSuccess ? IDV_OK : IDV_ELAUNCH;
}

}  // namespace

extern "C" long long idv_stoi_work_bytes(int B, int Lmax, int fs) {
    if (B <= 0 || Lmax <= 0 || Lmax > ROWS_MAX_LEN || (fs != 10000 && fs != 16000)) return -1;
    return layout(B, Lmax, fs).bytes;
}

extern "C" int idv_stoi(const float* ref, long long ref_ld, const float* est, long long est_ld, const int* lens, int B, int Lmax, int fs,
                        int extended, void* work, long long work_bytes, float* out, int* counts, void* stream) {
    if (!ref || !est || !work || !out || !row_limits_ok(B, Lmax) || (fs != 10000 && fs != 16000)) return IDV_EINVAL;   // 8 n stays an int
    if (ref_ld < Lmax || est_ld < Lmax || !aligned_to(16, {work})) return IDV_EINVAL;
    const Layout l = layout(B, Lmax, fs);
    if (work_bytes < l.bytes) return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int rc = ensure_tables(st);
    if (rc != IDV_OK) return rc;
    const int fs16 = fs == 16000;
    char* wk = (char*)work;
    float* rs = (float*)(wk + l.off_rs);
    double* en = (double*)(wk + l.off_en);
    int* kept = (int*)(wk + l.off_kept);
    int* Kc = (int*)(wk + l.off_K);
    float* tob = (float*)(wk + l.off_tob);
    double* part = (double*)(wk + l.off_part);
    const int n10 = n10_of(Lmax, fs16), F = frames_of(n10), Fp = (int)l.Fp;
    const float* x0 = ref;
    const float* x1 = est;
    long long ld0 = ref_ld, ld1 = est_ld;
    if (fs16) {
        hipLaunchKernelGGL(resample_kernel, dim3((n10 + 255) / 256, B, 2), dim3(256), 0, st, ref, ref_ld, est, est_ld, lens, Lmax, rs,
                           l.rs_ld, B);
        x0 = rs;
        x1 = rs + (size_t)B * l.rs_ld;
        ld0 = ld1 = l.rs_ld;
    }
    if (F > 0)
        hipLaunchKernelGGL(energy_kernel, dim3((F + 3) / 4, B), dim3(256), 0, st, x0, ld0, lens, Lmax, fs16, en, Fp);
    hipLaunchKernelGGL(mask_kernel, dim3(B), dim3(256), 0, st, en, lens, Lmax, fs16, Fp, kept, Kc, counts);
    if (F - 1 >= NSEG) {
        hipLaunchKernelGGL(spec_band_kernel, dim3((F - 1 + FPW - 1) / FPW, B, 2), dim3(256), 0, st, x0, ld0, x1, ld1, kept, Kc, Fp, B, tob);
        hipLaunchKernelGGL(segment_kernel, dim3((int)l.nblk, B), dim3(256), 0, st, tob, Kc, Fp, B, extended ? 1 : 0, part, (int)l.nblk);
    }
    hipLaunchKernelGGL(final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, part, Kc, (int)l.nblk, B, extended ? 1 : 0, out);
    return idv_launch_status();
}

extern "C" int idv_rmse_ragged(const float* ref, long long ref_ld, const float* est, long long est_ld, const int* lens, int B, double* work,
                               float* out, void* stream) {
    if (!ref || !est || !lens || !work || !out || B <= 0 || ref_ld <= 0 || est_ld <= 0) return IDV_EINVAL;
    const long long m = ref_ld < est_ld ? ref_ld : est_ld;
    const int Lmax = m > 2147483647LL ? 2147483647 : (int)m;
    hipLaunchKernelGGL(rmse_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, ref, ref_ld, est, est_ld, lens, Lmax, work, out);
    return idv_launch_status();
}
