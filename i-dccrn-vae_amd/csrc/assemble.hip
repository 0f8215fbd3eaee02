// Clip assembly: rows joined from several recordings with pauses between them, the share of active 50 ms windows of every candidate
// row, the choice among the candidates and the written rows: dataset/assemble.py assemble / activity / SignalPool.stats.
// The definition is build_audio / activitydetector of the DNS-Challenge synthesizer restated (tests/assemble_ref.py; parity with the
// package itself is unpinned).  EPS = 2^-52.
//
// A candidate row r = b tries + t is a list of at most 64 pieces (src, len, dst): len samples at pool + src go to positions dst .. of the
// row; the pieces are sorted by dst and disjoint, what no piece covers is +0.
//
//   (a) asm_window_kernel  one wave per win-sample window k of a candidate: W[r][k] = max|x|, sum x^2 in double (the square of a float32
//                          is exact in double).  Every sample is read once, 16 bytes per lane.
//   (b) asm_choose_kernel  one workgroup per row b; per candidate: the row's sum, k = T / (rms + EPS), per window db = 20 log10(k^2 sum
//                          + EPS), p = 1 / (1 + exp(-(a + b db))), the one-window smoothing, the count of windows with s > thresh;
//                          then the first candidate whose activity exceeds min_activity, or the most active one.
//   (c) asm_write_kernel   row b of the output = the pieces of candidate chosen[b] (read on the device), +0 elsewhere.
//
// The 64 pieces of a row sit in LDS; a lane finds the piece under the first sample of ITS quad by a 7-step search and loads the 16
// bytes wherever they lie (4-byte aligned vector loads); a quad that straddles a piece's end, a pause or the row's end is read sample
// by sample.  Every sum is taken in the fixed order of rows.hpp, so a candidate's numbers do not depend on B, on tries, on the other
// rows or on where its pieces lie in the pool.  A piece that is not inside the pool and inside its row is dropped whole, so no table
// can make a kernel read outside the pool.  No atomics, no spin, every loop bounded.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

#include <cmath>

namespace {

constexpr int AS_MAXP = IDV_ASM_MAX_PIECES;
constexpr int AS_WF = IDV_ASM_WIN_FIELDS;     // doubles per window: max|x|, sum x^2
constexpr double AS_EPS = 2.220446049250313e-16;
constexpr double AS_A = -1.0, AS_B = 0.2;     // the logistic of activitydetector
constexpr double AS_ATT = 0.8, AS_REL = 0.05; // its attack and release

struct Piece {
    long long src;
    int len, dst;
};

struct Tables {
    const float* pool;
    long long pool_n;
    const long long* src;
    const int* len;
    const int* dst;
    const int* first;
    const int* count;
    int npieces;
};

// the pieces of candidate r -> sh[0 .. 64) (threads 0 .. 63; the caller synchronises) and their number
__device__ __forceinline__ int load_pieces(const Tables& T, int r, int n, Piece* sh, int tid) {
    const int f = T.first[r];
    int c = T.count[r];
    c = (f < 0 || f > T.npieces) ? 0 : max(0, min(c, min(AS_MAXP, T.npieces - f)));
    if (tid < AS_MAXP) {
        Piece pc{0, 0, 0};
        if (tid < c) {
            const long long s = T.src[f + tid];
            const int l = T.len[f + tid], d = T.dst[f + tid];
            const bool ok = l > 0 && d >= 0 && d <= n - l && s >= 0 && s <= T.pool_n - l;
            pc = Piece{s, ok ? l : 0, d};
        }
        sh[tid] = pc;
    }
    return c;
}

// the last piece j < c with dst <= p, -1 where there is none
__device__ __forceinline__ int find_piece(const Piece* sh, int c, int p) {
    int lo = -1;
#pragma unroll
    for (int step = 64; step > 0; step >>= 1) {
        const int j = lo + step;
        if (j < c && sh[j].dst <= p) lo = j;
    }
    return lo;
}

// positions p .. p + 3 of the row; +0 where no piece lies (every piece ends inside the row, so neither does one past the row's end)
__device__ __forceinline__ float4 load_row4(const float* __restrict__ pool, const Piece* sh, int c, int p) {
    int j = find_piece(sh, c, p);
    if (j >= 0) {
        const Piece pc = sh[j];
        const int o = p - pc.dst;
        if (o + 3 < pc.len) {
            const quad_t q = *reinterpret_cast<const quad_t*>(pool + pc.src + o);
            return make_float4(q.x, q.y, q.z, q.w);
        }
    }
    float t[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int pos = p + e;
        if (j + 1 < c && sh[j + 1].dst <= pos) ++j;        // dst grows by at least 1 from piece to piece: one step per sample
        float v = 0.f;
        if (j >= 0) {
            const Piece pc = sh[j];
            const int o = pos - pc.dst;
            if (o < pc.len) v = pool[pc.src + o];
        }
        t[e] = v;
    }
    return make_float4(t[0], t[1], t[2], t[3]);
}

__global__ __launch_bounds__(256) void asm_window_kernel(Tables T, const int* __restrict__ rowlen, int samples, int win, int nwin,
                                                         double* __restrict__ W) {
    __shared__ Piece sh[AS_MAXP];
    const int r = blockIdx.y;
    Window w = wave_window();
    const int n = row_len(rowlen, r, samples);
    const int c = load_pieces(T, r, n, sh, threadIdx.x);
    __syncthreads();
    if (w.k >= nwin) return;
    double s = 0, m = 0;
    if (w.cut(win, n)) {                                   // wave-uniform
        for (int q = w.lane; q < w.nquad; q += 64) {
            const float4 a = load_row4(T.pool, sh, c, w.w0 + 4 * q);
            acc_sq(s, m, a.x), acc_sq(s, m, a.y), acc_sq(s, m, a.z), acc_sq(s, m, a.w);
        }
        s = wave_sum_d(s);
        m = wave_max_d(m);
    }
    if (w.lane == 0) {
        double* o = W + ((size_t)r * nwin + w.k) * AS_WF;
        o[0] = m, o[1] = s;
    }
}

__device__ __forceinline__ double energy_prob(double k2, double sum) {
    const double db = 20.0 * log10(k2 * sum + AS_EPS);
    return 1.0 / (1.0 + exp(-(AS_A + AS_B * db)));
}

__global__ __launch_bounds__(256) void asm_choose_kernel(const int* __restrict__ rowlen, int tries, int samples, int win, int nwin,
                                                         const double* __restrict__ W, double target_db, double energy_thresh,
                                                         double min_activity, double* __restrict__ rowstat, int* __restrict__ active,
                                                         int* __restrict__ windows, double* __restrict__ activity, int* __restrict__ chosen,
                                                         int* __restrict__ accepted) {
    __shared__ double sh[256];
    __shared__ int s_act[IDV_ASM_MAX_TRIES], s_nw[IDV_ASM_MAX_TRIES];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int t = 0; t < tries; ++t) {
        const int r = b * tries + t;
        const int n = row_len(rowlen, r, samples);
        const int nw = (int)(((long long)n + win - 1) / win);
        const double* Wr = W + (size_t)r * nwin * AS_WF;
        double mx = 0, sm = 0;
        for (int k = tid; k < nw; k += 256) mx = fmax(mx, Wr[k * (size_t)AS_WF]), sm += Wr[k * (size_t)AS_WF + 1];
        mx = block_max(mx, sh, tid);
        sm = block_sum(sm, sh, tid);
        const double kk = pow(10.0, target_db / 20.0) / (sqrt(sm / (double)max(n, 1)) + AS_EPS);
        const double k2 = kk * kk;
        double cnt = 0;
        for (int k = tid; k < nw; k += 256) {              // the smoothing looks back one window: the windows are independent
            const double p = energy_prob(k2, Wr[k * (size_t)AS_WF + 1]);
            const double pp = k > 0 ? energy_prob(k2, Wr[(k - 1) * (size_t)AS_WF + 1]) : 0.0;
            const double sj = p > pp ? AS_ATT * p + (1.0 - AS_ATT) * pp : AS_REL * p + (1.0 - AS_REL) * pp;
            cnt += sj > energy_thresh ? 1.0 : 0.0;
        }
        cnt = block_sum(cnt, sh, tid);                     // whole numbers: exact
        if (tid == 0) {
            s_act[t] = (int)cnt, s_nw[t] = nw;
            active[r] = (int)cnt, windows[r] = nw;
            activity[r] = nw > 0 ? cnt / (double)nw : 0.0;
            rowstat[2 * (size_t)r] = mx, rowstat[2 * (size_t)r + 1] = sm;
        }
    }
    if (tid == 0) {
        int pick = -1, best = 0;
        for (int t = 0; t < tries && pick < 0; ++t)
            if (s_nw[t] > 0 && (double)s_act[t] / (double)s_nw[t] > min_activity) pick = t;
        accepted[b] = pick >= 0 ? 1 : 0;
        if (pick < 0) {
            for (int t = 1; t < tries; ++t)
                if (s_act[t] > s_act[best]) best = t;
            pick = best;
        }
        chosen[b] = pick;
    }
}

__global__ __launch_bounds__(256) void asm_write_kernel(Tables T, const int* __restrict__ chosen, int tries, int samples,
                                                        float* __restrict__ out, long long ldo) {
    __shared__ Piece sh[AS_MAXP];
    const int b = blockIdx.y;
    const int t = max(0, min(chosen[b], tries - 1));
    const int c = load_pieces(T, b * tries + t, samples, sh, threadIdx.x);
    __syncthreads();
    const long long i0 = 4LL * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= samples) return;
    const int p = (int)i0;
    store4(out + (size_t)b * ldo, p, samples, load_row4(T.pool, sh, c, p));
}

bool tables_ok(const float* pool, long long pool_n, const long long* src, const int* len, const int* dst, const int* first,
               const int* count, int npieces, int B, int tries, int samples) {
    if (!pool || !src || !len || !dst || !first || !count) return false;
    if (pool_n <= 0 || npieces <= 0 || npieces > (1 << 30)) return false;
    if (B <= 0 || tries < 1 || tries > IDV_ASM_MAX_TRIES || !row_limits_ok((long long)B * tries, samples)) return false;
    return aligned_to(4, {pool, len, dst, first, count}) && aligned_to(8, {src});
}

}  // namespace

extern "C" long long idv_asm_work_bytes(int R, int samples, int win) { return window_work_bytes(R, samples, win, AS_WF); }

extern "C" int idv_asm_activity(const float* pool, long long pool_n, const long long* src, const int* len, const int* dst, const int* first,
                                const int* count, int npieces, const int* rowlen, int B, int tries, int samples, int win, double target_db,
                                double energy_thresh, double min_activity, void* work, long long work_bytes, double* rowstat, int* active,
                                int* windows, double* activity, int* chosen, int* accepted, void* stream) {
    if (!tables_ok(pool, pool_n, src, len, dst, first, count, npieces, B, tries, samples)) return IDV_EINVAL;
    const long long need = idv_asm_work_bytes(B * tries, samples, win);
    if (need < 0 || !work || work_bytes < need) return IDV_EINVAL;
    if (!rowstat || !active || !windows || !activity || !chosen || !accepted) return IDV_EINVAL;
    if (!aligned_to(8, {work, rowstat, activity}) || !aligned_to(4, {active, windows, chosen, accepted, rowlen})) return IDV_EINVAL;
    if (!std::isfinite(target_db) || !std::isfinite(energy_thresh) || !std::isfinite(min_activity)) return IDV_EINVAL;
    const int nwin = (int)(((long long)samples + win - 1) / win);
    const Tables T{pool, pool_n, src, len, dst, first, count, npieces};
    hipStream_t st = (hipStream_t)stream;
    double* W = (double*)work;
    hipLaunchKernelGGL(asm_window_kernel, dim3((nwin + 3) / 4, B * tries), dim3(256), 0, st, T, rowlen, samples, win, nwin, W);
    hipLaunchKernelGGL(asm_choose_kernel, dim3(B), dim3(256), 0, st, rowlen, tries, samples, win, nwin, (const double*)W, target_db,
                       energy_thresh, min_activity, rowstat, active, windows, activity, chosen, accepted);
    return idv_launch_status();
}

extern "C" int idv_asm_write(const float* pool, long long pool_n, const long long* src, const int* len, const int* dst, const int* first,
                             const int* count, int npieces, const int* chosen, int B, int tries, int samples, float* out, long long ldo,
                             void* stream) {
    if (!tables_ok(pool, pool_n, src, len, dst, first, count, npieces, B, tries, samples)) return IDV_EINVAL;
    if (!chosen || !out || ldo < samples || !aligned_to(4, {chosen, out})) return IDV_EINVAL;
    const Tables T{pool, pool_n, src, len, dst, first, count, npieces};
    const unsigned gx = (unsigned)(((long long)samples + 1023) / 1024);
    hipLaunchKernelGGL(asm_write_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, T, chosen, tries, samples, out, ldo);
    return idv_launch_status();
}
