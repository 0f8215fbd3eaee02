// Mixture synthesis at a given SNR and level for rows of different lengths: dataset/mix.py snr_mix / DynamicMixtures.
// The definition is normalize / snr_mixer / segmental_snr_mixer of the DNS-Challenge synthesizer restated (tests/mix_ref.py; parity with
// the package itself is unpinned), with a window's level the true dB of its mean square.  EPS = 2^-52, T = 10^(target_db / 20); row b has
// n = lens[b] clean samples c[i] and the noise v[i] = noise_b[(o + i) mod m], m = noise_lens[b], o = noise_phase[b]:
//
//   kc = T / (rms(c) / (max|c| + EPS) + EPS) / (max|c| + EPS), kv alike:  c2 = kc c, v2 = kv v
//   plain: rc = rms(c2), rv = rms(v2);  segmental: the same over the samples of the win-sample windows whose 10 log10(mean(v2^2) + EPS)
//   exceeds thresh_db (EPS and EPS when there is none)
//   a = kc, b = kv rc / 10^(snr_db / 20) / (rv + EPS):  y0 = a c + b v;   s = 10^(level_db / 20) / (rms(y0) + EPS);
//   s max|y0| > clip: s is divided by s max|y0| / (clip - EPS);   g_clean = a s, g_noise = b s
//
//   (a) window_stats_kernel  one wave per win-sample window k of a row: W[b][k] = max|c|, sum c^2, max|v|, sum v^2 in double (the square of
//                            a float32 is exact in double).  Every sample is read once, 16 bytes per lane.
//   (b) row_gains_kernel     one workgroup per row: the windows' partials -> row statistics, the active windows, a and b.
//   (c) window_level_kernel  one wave per window: sum y0^2 and max|y0| from the samples themselves (sum c v would cancel where c = -v).
//   (d) row_final_kernel     one workgroup per row: s, the clip rule, g_clean, g_noise, the realised level.
//   (e) write_kernel         noisy = float(g_clean c + g_noise v), clean_out = float(g_clean c), noise_out = float(g_noise v): one fp32
//                            rounding of a double expression of the INPUT samples each; zeros from n to the width.
//
// A row is base + off[b] (device int64 sample offsets: rows read in place in a packed pool) or base + b ld (off == NULL: a padded
// batch), at any alignment: a lane loads the 16 bytes of ITS quad wherever they lie (4-byte aligned vector loads); a quad that
// straddles the row's end or the noise's wrap is read sample by sample.  Every sum is taken in the fixed order of rows.hpp, so a row's
// result does not depend on B, on the other rows, on what lies at or past n (it is never read), on the row pitch or on the base
// alignment.  No atomics; pow, log10 and sqrt run in double on the device, nothing returns to the host.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

#include <cmath>

namespace {

constexpr int MX_WF = IDV_MIX_WIN_FIELDS;     // doubles per window: max|c|, sum c^2, max|v|, sum v^2, max|y0|, sum y0^2
constexpr int MX_RF = IDV_MIX_ROW_FIELDS;     // doubles per row, the IDV_MIX_* indices of the header
constexpr double MX_EPS = 2.220446049250313e-16;

struct Row {
    const float* c;       // n samples
    const float* v;       // m samples, read cyclically from o
    int n, m, o;
};

__device__ __forceinline__ Row row_of(const float* __restrict__ clean, const long long* __restrict__ clean_off, long long ldc,
                                      const float* __restrict__ noise, const long long* __restrict__ noise_off, long long ldn,
                                      const int* __restrict__ lens, const int* __restrict__ noise_lens, const int* __restrict__ phase, int L,
                                      int Ln, int b) {
    Row r;
    r.c = row_base(clean, clean_off, ldc, b);
    r.v = row_base(noise, noise_off, ldn, b);
    r.n = row_len(lens, b, L);
    r.m = max(1, min(noise_lens ? noise_lens[b] : Ln, Ln));
    const int o = phase ? phase[b] : 0;
    r.o = o > 0 ? o % r.m : 0;
    return r;
}

// the noise under samples p .. p + 3 of the row: j = (o + p) mod m is passed in; one load where the four are contiguous in the noise row
__device__ __forceinline__ float4 load_noise(const float* __restrict__ v, int j, int m, int p, int cnt) {
    float4 r;
    if (p + 3 < cnt && j + 3 < m) {
        const quad_t q = *reinterpret_cast<const quad_t*>(v + j);
        return make_float4(q.x, q.y, q.z, q.w);
    }
    float t[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        t[e] = p + e < cnt ? v[j] : 0.f;
        j = j + 1 < m ? j + 1 : 0;
    }
    r.x = t[0], r.y = t[1], r.z = t[2], r.w = t[3];
    return r;
}

// (j0 + d) mod m for 0 <= j0 < m and d >= 0, without a division where the noise row is at least as long as d
__device__ __forceinline__ int wrap(int j0, int d, int m) {
    unsigned j = (unsigned)j0 + (unsigned)d;
    if (j >= (unsigned)m) {
        j -= (unsigned)m;
        if (j >= (unsigned)m) j %= (unsigned)m;
    }
    return (int)j;
}

#define MIX_ROW_PARAMS                                                                                                                   \
    const float *__restrict__ clean, const long long *__restrict__ clean_off, long long ldc, const float *__restrict__ noise,           \
        const long long *__restrict__ noise_off, long long ldn, const int *__restrict__ lens, const int *__restrict__ noise_lens,       \
        const int *__restrict__ phase, int L, int Ln
#define MIX_ROW_ARGS clean, clean_off, ldc, noise, noise_off, ldn, lens, noise_lens, phase, L, Ln

__global__ __launch_bounds__(256) void window_stats_kernel(MIX_ROW_PARAMS, int win, int nwin, double* __restrict__ W) {
    const int b = blockIdx.y;
    Window w = wave_window();
    if (w.k >= nwin) return;
    const Row r = row_of(MIX_ROW_ARGS, b);
    double sc = 0, mc = 0, sv = 0, mv = 0;
    if (w.cut(win, r.n)) {                                 // wave-uniform
        const int jw = wrap(r.o, w.w0, r.m);
        for (int q = w.lane; q < w.nquad; q += 64) {
            const float4 a = load4(r.c + w.w0, 4 * q, w.cnt);
            const float4 u = load_noise(r.v, wrap(jw, 4 * q, r.m), r.m, 4 * q, w.cnt);
            acc_sq(sc, mc, a.x), acc_sq(sc, mc, a.y), acc_sq(sc, mc, a.z), acc_sq(sc, mc, a.w);
            acc_sq(sv, mv, u.x), acc_sq(sv, mv, u.y), acc_sq(sv, mv, u.z), acc_sq(sv, mv, u.w);
        }
        sc = wave_sum_d(sc), sv = wave_sum_d(sv);
        mc = wave_max_d(mc), mv = wave_max_d(mv);
    }
    if (w.lane == 0) {
        double* o = W + ((size_t)b * nwin + w.k) * MX_WF;
        o[0] = mc, o[1] = sc, o[2] = mv, o[3] = sv;
    }
}

__global__ __launch_bounds__(256) void window_level_kernel(MIX_ROW_PARAMS, int win, int nwin, const double* __restrict__ R,
                                                           double* __restrict__ W) {
    const int b = blockIdx.y;
    Window w = wave_window();
    if (w.k >= nwin) return;
    const Row r = row_of(MIX_ROW_ARGS, b);
    const double ga = R[(size_t)b * MX_RF + IDV_MIX_A], gb = R[(size_t)b * MX_RF + IDV_MIX_B];
    double sy = 0, my = 0;
    if (w.cut(win, r.n)) {
        const int jw = wrap(r.o, w.w0, r.m);
        for (int q = w.lane; q < w.nquad; q += 64) {
            const float4 a = load4(r.c + w.w0, 4 * q, w.cnt);
            const float4 u = load_noise(r.v, wrap(jw, 4 * q, r.m), r.m, 4 * q, w.cnt);
            const double y0 = fma(ga, (double)a.x, gb * (double)u.x), y1 = fma(ga, (double)a.y, gb * (double)u.y);
            const double y2 = fma(ga, (double)a.z, gb * (double)u.z), y3 = fma(ga, (double)a.w, gb * (double)u.w);
            sy += y0 * y0, sy += y1 * y1, sy += y2 * y2, sy += y3 * y3;
            my = fmax(fmax(my, fabs(y0)), fmax(fabs(y1), fmax(fabs(y2), fabs(y3))));
        }
        sy = wave_sum_d(sy);
        my = wave_max_d(my);
    }
    if (w.lane == 0) {
        double* o = W + ((size_t)b * nwin + w.k) * MX_WF;
        o[4] = my, o[5] = sy;
    }
}

__global__ __launch_bounds__(256) void row_gains_kernel(const int* __restrict__ lens, int L, int win, int nwin, const double* __restrict__ W,
                                                        const double* __restrict__ par, int segmental, double target_db, double thresh_db,
                                                        double* __restrict__ R) {
    __shared__ double sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = row_len(lens, b, L);
    const int nw = (int)(((long long)n + win - 1) / win);
    const double* Wr = W + (size_t)b * nwin * MX_WF;
    double mc = 0, sc = 0, mv = 0, sv = 0;
    for (int k = tid; k < nw; k += 256) {
        mc = fmax(mc, Wr[k * (size_t)MX_WF]), sc += Wr[k * (size_t)MX_WF + 1];
        mv = fmax(mv, Wr[k * (size_t)MX_WF + 2]), sv += Wr[k * (size_t)MX_WF + 3];
    }
    mc = block_max(mc, sh, tid), mv = block_max(mv, sh, tid);
    sc = block_sum(sc, sh, tid), sv = block_sum(sv, sh, tid);
    const double nn = (double)max(n, 1);
    const double T = pow(10.0, target_db / 20.0);
    const double kc = T / (sqrt(sc / nn) / (mc + MX_EPS) + MX_EPS) / (mc + MX_EPS);
    const double kv = T / (sqrt(sv / nn) / (mv + MX_EPS) + MX_EPS) / (mv + MX_EPS);
    double ac = sc, av = sv, cnt = (double)n;
    if (segmental) {
        ac = av = cnt = 0;
        for (int k = tid; k < nw; k += 256) {
            const int len = min(win, n - k * win);
            const double e = Wr[k * (size_t)MX_WF + 3];
            if (10.0 * log10(kv * kv * e / (double)len + MX_EPS) > thresh_db) ac += Wr[k * (size_t)MX_WF + 1], av += e, cnt += (double)len;
        }
        ac = block_sum(ac, sh, tid), av = block_sum(av, sh, tid), cnt = block_sum(cnt, sh, tid);
    }
    if (tid == 0) {
        const bool some = cnt > 0;
        const double rc = some ? kc * sqrt(ac / cnt) : MX_EPS, rv = some ? kv * sqrt(av / cnt) : MX_EPS;
        double* r = R + (size_t)b * MX_RF;
        r[IDV_MIX_MAX_C] = mc, r[IDV_MIX_SUM_C2] = sc, r[IDV_MIX_MAX_V] = mv, r[IDV_MIX_SUM_V2] = sv;
        r[IDV_MIX_ACT_C2] = ac, r[IDV_MIX_ACT_V2] = av, r[IDV_MIX_ACTIVE] = cnt;
        r[IDV_MIX_A] = kc;
        r[IDV_MIX_B] = kv * rc / pow(10.0, par[2 * b] / 20.0) / (rv + MX_EPS);
    }
}

__global__ __launch_bounds__(256) void row_final_kernel(const int* __restrict__ lens, int L, int win, int nwin, const double* __restrict__ W,
                                                        const double* __restrict__ par, double clip, double* __restrict__ R) {
    __shared__ double sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = row_len(lens, b, L);
    const int nw = (int)(((long long)n + win - 1) / win);
    const double* Wr = W + (size_t)b * nwin * MX_WF;
    double my = 0, sy = 0;
    for (int k = tid; k < nw; k += 256) my = fmax(my, Wr[k * (size_t)MX_WF + 4]), sy += Wr[k * (size_t)MX_WF + 5];
    my = block_max(my, sh, tid);
    sy = block_sum(sy, sh, tid);
    if (tid == 0) {
        double* r = R + (size_t)b * MX_RF;
        const double ry = sqrt(sy / (double)max(n, 1));
        double s = pow(10.0, par[2 * b + 1] / 20.0) / (ry + MX_EPS);
        const double peak = s * my;
        const bool clipped = peak > clip;
        if (clipped) s = s / (peak / (clip - MX_EPS));
        r[IDV_MIX_SUM_Y2] = sy, r[IDV_MIX_MAX_Y] = my;
        r[IDV_MIX_G_CLEAN] = r[IDV_MIX_A] * s;
        r[IDV_MIX_G_NOISE] = r[IDV_MIX_B] * s;
        r[IDV_MIX_LEVEL_DB] = 20.0 * log10(s * ry + MX_EPS);
        r[IDV_MIX_CLIPPED] = clipped ? 1.0 : 0.0;
        r[IDV_MIX_LEN] = (double)n;
    }
}

__global__ __launch_bounds__(256) void write_kernel(MIX_ROW_PARAMS, const double* __restrict__ R, float* __restrict__ noisy,
                                                    float* __restrict__ clean_out, float* __restrict__ noise_out, long long ldy) {
    const int b = blockIdx.y;
    const long long i0 = 4LL * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= L) return;
    const Row r = row_of(MIX_ROW_ARGS, b);
    const double gc = R[(size_t)b * MX_RF + IDV_MIX_G_CLEAN], gv = R[(size_t)b * MX_RF + IDV_MIX_G_NOISE];
    const int p = (int)i0;
    float y[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    if (p < r.n) {
        const float4 a = load4(r.c, p, r.n);
        const float4 u = load_noise(r.v, (int)(((unsigned)r.o + (unsigned)p) % (unsigned)r.m), r.m, p, r.n);
        const float ca[4] = {a.x, a.y, a.z, a.w}, ua[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p + e < r.n) {
                const double dc = gc * (double)ca[e], dv = gv * (double)ua[e];
                c[e] = (float)dc;
                v[e] = (float)dv;
                y[e] = (float)fma(gc, (double)ca[e], dv);
            }
        }
    }
    const size_t at = (size_t)b * ldy;
    store4(noisy + at, p, L, make_float4(y[0], y[1], y[2], y[3]));
    store4(clean_out + at, p, L, make_float4(c[0], c[1], c[2], c[3]));
    store4(noise_out + at, p, L, make_float4(v[0], v[1], v[2], v[3]));
}

bool rows_ok(const float* clean, const long long* clean_off, long long ldc, const float* noise, const long long* noise_off, long long ldn,
             int B, int L, int Ln) {
    if (!clean || !noise || !row_limits_ok(B, L) || !row_limits_ok(B, Ln)) return false;
    if (!clean_off && ldc < L) return false;
    if (!noise_off && ldn < Ln) return false;
    return aligned_to(4, {clean, noise}) && aligned_to(8, {clean_off, noise_off});
}

}  // namespace

extern "C" long long idv_mix_work_bytes(int B, int L, int win) { return window_work_bytes(B, L, win, MX_WF); }

extern "C" int idv_mix_gains(const float* clean, const long long* clean_off, long long ldc, const float* noise, const long long* noise_off,
                             long long ldn, const int* lens, const int* noise_lens, const int* phase, int B, int L, int Ln,
                             const double* par, int segmental, double target_db, double clip, int win, double thresh_db, void* work,
                             long long work_bytes, double* rows, void* stream) {
    const long long need = idv_mix_work_bytes(B, L, win);
    if (need < 0 || !rows_ok(clean, clean_off, ldc, noise, noise_off, ldn, B, L, Ln)) return IDV_EINVAL;
    if (!par || !work || !rows || work_bytes < need || !aligned_to(8, {work, rows, par})) return IDV_EINVAL;
    if (!std::isfinite(target_db) || !std::isfinite(thresh_db) || !std::isfinite(clip) || !(clip > 2 * MX_EPS)) return IDV_EINVAL;
    if (segmental != 0 && segmental != 1) return IDV_EINVAL;
    const int nwin = (int)(((long long)L + win - 1) / win);
    const dim3 gw((nwin + 3) / 4, B), gr(B), blk(256);
    hipStream_t st = (hipStream_t)stream;
    double* W = (double*)work;
    hipLaunchKernelGGL(window_stats_kernel, gw, blk, 0, st, MIX_ROW_ARGS, win, nwin, W);
    hipLaunchKernelGGL(row_gains_kernel, gr, blk, 0, st, lens, L, win, nwin, (const double*)W, par, segmental, target_db, thresh_db, rows);
    hipLaunchKernelGGL(window_level_kernel, gw, blk, 0, st, MIX_ROW_ARGS, win, nwin, (const double*)rows, W);
    hipLaunchKernelGGL(row_final_kernel, gr, blk, 0, st, lens, L, win, nwin, (const double*)W, par, clip, rows);
    return idv_launch_status();
}

extern "C" int idv_mix_write(const float* clean, const long long* clean_off, long long ldc, const float* noise, const long long* noise_off,
                             long long ldn, const int* lens, const int* noise_lens, const int* phase, int B, int L, int Ln,
                             const double* rows, float* noisy, float* clean_out, float* noise_out, long long ldy, void* stream) {
    if (!rows_ok(clean, clean_off, ldc, noise, noise_off, ldn, B, L, Ln)) return IDV_EINVAL;
    if (!rows || !noisy || !clean_out || !noise_out || ldy < L) return IDV_EINVAL;
    if (!aligned_to(8, {rows}) || !aligned_to(4, {noisy, clean_out, noise_out})) return IDV_EINVAL;
    const unsigned gx = (unsigned)(((long long)L + 1023) / 1024);
    hipLaunchKernelGGL(write_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, MIX_ROW_ARGS, rows, noisy, clean_out, noise_out, ldy);
    return idv_launch_status();
}
