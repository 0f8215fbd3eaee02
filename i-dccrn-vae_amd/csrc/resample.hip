// Rational polyphase resampler for a padded batch of signals of different lengths: inference.resample / resample_list.
//
//   y[b][n] = up * sum_j x[b][j] h[half + n*down - j*up],   0 <= j < L_b,  0 <= half + n*down - j*up <= 2*half,   n < ceil(L_b*up/down)
//
// which is scipy.signal.resample_poly(x, up, down) with its default filter when h is that filter (up/down reduced by their gcd, m =
// max(up, down), half = 10*m, h = kaiser(2*half + 1, 5.0) * sinc(t/m)/m normalised to sum 1; the caller forms h in double and passes it
// as fp32).  Numerics as resample_kernel of stoi.hip: fp32 samples and taps, one double accumulator per output, j increasing, no atomics.
//
// One workgroup per (256 outputs, row).  The taps sit in LDS at a skewed index k + (k >> 5): neighbouring outputs read taps `down`
// apart, and an even `down` (160: 44.1 kHz from 16 kHz) would otherwise put the 64 lanes on two banks.  The input span of the 256 outputs
// is staged in LDS too where it fits XCAP samples (every ratio between the common rates and 16 kHz); a longer span (decimation by more
// than 9 with up = 1) is read from memory with the same indices in the same order, so both forms give the same bits.  Row b reads
// nothing at or past lens[b] and nothing of another row; columns n_out(lens[b]) .. ncols - 1 are written as zeros.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int RS_MAXM = 640;                  // max(up, down) after reduction
constexpr int RS_NO = 256;                    // outputs per workgroup
constexpr int XCAP = 2560;                    // staged input samples per workgroup

__host__ __device__ __forceinline__ int skew(int k) { return k + (k >> 5); }
__host__ __device__ __forceinline__ long long fdiv(long long a, long long d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }
__host__ __device__ __forceinline__ long long n_out_of(long long L, int up, int down) { return (L * up + down - 1) / down; }

template <bool STAGED>
__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lens, int Lmax,
                                                            int up, int down, int half, const float* __restrict__ taps,
                                                            float* __restrict__ y, long long ldy, long long ncols) {
    extern __shared__ float sh[];
    const int ntap = 2 * half + 1;
    float* hs = sh;                                        // skew(ntap - 1) + 1 floats
    float* xs = sh + skew(ntap - 1) + 1;                   // XCAP floats (STAGED)
    const int b = blockIdx.y;
    const int L = row_len(lens, b, Lmax);
    const long long nout = n_out_of(L, up, down);
    const long long n0 = (long long)blockIdx.x * RS_NO, n = n0 + threadIdx.x;
    float* yr = y + (size_t)b * ldy;
    if (n0 >= nout) {                                      // a workgroup past this row's end: zeros only
        if (n < ncols) yr[n] = 0.f;
        return;
    }
    const float* xr = x + (size_t)b * ldx;
    for (int k = threadIdx.x; k < ntap; k += 256) hs[skew(k)] = taps[k];
    // smallest j any output of this workgroup reads: ceil((n0*down - half) / up), not below 0
    const long long jbase = max(0LL, -fdiv(half - n0 * down, up));
    if (STAGED) {
        const long long nl = min(n0 + RS_NO, nout) - 1;
        const long long jtop = min((long long)L - 1, fdiv(nl * down + half, up));
        const int cnt = (int)(jtop - jbase + 1);           // <= XCAP: the host chose STAGED for this (up, down)
        for (int k = threadIdx.x; k < cnt; k += 256) xs[k] = xr[jbase + k];
    }
    __syncthreads();
    if (n >= ncols) return;
    if (n >= nout) {
        yr[n] = 0.f;
        return;
    }
    const long long c = n * down + half;                   // tap index of j = 0
    const long long jlo = max(0LL, -fdiv(half - n * down, up)), jhi = min((long long)L - 1, fdiv(c, up));
    double acc = 0;
    int k = (int)(c - jlo * up);                           // in [0, 2*half] for jlo <= j <= jhi
    if (STAGED) {
        const float* xp = xs + (jlo - jbase);
        for (long long j = jlo; j <= jhi; ++j, k -= up) acc += (double)(*xp++) * (double)hs[skew(k)];
    } else {
        for (long long j = jlo; j <= jhi; ++j, k -= up) acc += (double)xr[j] * (double)hs[skew(k)];
    }
    yr[n] = (float)((double)up * acc);
}

int gcd_of(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

extern "C" int idv_resample_ntaps(int up, int down) {
    if (up <= 0 || down <= 0) return IDV_EINVAL;
    const int g = gcd_of(up, down);
    const int m = up > down ? up / g : down / g;
    if (m > RS_MAXM) return IDV_EINVAL;
    return 20 * m + 1;
}

extern "C" long long idv_resample_len(long long L, int up, int down) {
    if (L < 0 || L > ROWS_MAX_LEN || idv_resample_ntaps(up, down) < 0) return IDV_EINVAL;
    const int g = gcd_of(up, down);
    return n_out_of(L, up / g, down / g);
}

extern "C" int idv_resample(const float* x, long long ldx, const int* lens, int B, int L, int up, int down, const float* taps, float* y,
                            long long ldy, void* stream) {
    if (!x || !taps || !y || !row_limits_ok(B, L) || ldx < L) return IDV_EINVAL;
    if (idv_resample_ntaps(up, down) < 0) return IDV_EINVAL;
    const int g = gcd_of(up, down);
    up /= g;
    down /= g;
    const int half = 10 * (up > down ? up : down);
    const long long ncols = n_out_of(L, up, down);
    if (ldy < ncols || ncols > 2147483647LL - RS_NO) return IDV_EINVAL;
    // the widest input span of one workgroup: j from ceil((n0*down - half)/up) to floor(((n0 + 255)*down + half)/up)
    const long long span = ((long long)(RS_NO - 1) * down + 2LL * half) / up + 2;
    const size_t ntap_sk = (size_t)skew(2 * half) + 1;
    const dim3 grid((unsigned)((ncols + RS_NO - 1) / RS_NO), B);
    hipStream_t st = (hipStream_t)stream;
    if (span <= XCAP)
        hipLaunchKernelGGL(resample_poly_kernel<true>, grid, dim3(256), (ntap_sk + XCAP) * sizeof(float), st, x, ldx, lens, L, up, down,
                           half, taps, y, ldy, ncols);
    else
        hipLaunchKernelGGL(resample_poly_kernel<false>, grid, dim3(256), ntap_sk * sizeof(float), st, x, ldx, lens, L, up, down, half,
                           taps, y, ldy, ncols);
    return idv_launch_status();
}
