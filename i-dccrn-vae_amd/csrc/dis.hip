// Distinguisher of the adversarial decoder fine-tune (model/pvae_module.py:2295-2351, model/nsvae_loss.py:953-986):
// the REAL two-layer nn.LSTM with hidden size 1 behind the six dis_Encoder blocks, forward and back-propagation through
// time, and the two LSGAN reductions with their gradients.  fp32 in and out, every sum in double, no atomics, no
// cooperative launch: nothing here needs a grid-wide barrier.
//
// The LSTM input is the last block's planar activation read IN PLACE: feature k = (c F + f) 2 + d of the reference's
// [T, B, 2 C F] tensor is plane p = d C F + (c F + f), frame t of row b is column j = b Tp + 1 + t.  Only those columns
// are read; the guard column in front of a row, anything past its T frames and the tail up to Jp are never looked at
// (quads of four columns are loaded with one 16-byte load where all four are frames, one by one otherwise).
//
//   projection      part[chunk][g][j] = sum over the chunk's RL_KC planes (ascending p) of W_ih0[g][k(p)] x[p][j]
//   gate sum        G0[g][j] = ((b_ih0[g] + b_hh0[g]) + part[0]) + part[1] + ...            (ascending chunk)
//   scan            one lane per row, both layers inside one step loop; saves the activated gates, the cell states
//                   and tanh(c) of both layers as save[t][12][B] doubles
//   reverse scan    one lane per row; dG0[g][j] and 20 per-row partial sums of the small parameter gradients
//   small reduce    the partials added over the rows b = 0, 1, ... by one thread each
//   back-projection dx[p][j] = sum_g W_ih0[g][k(p)] dG0[g][j]  (zeros in every non-frame column: the planar
//                   invariant) and wpart[tile][g][p] = sum over the tile's 1024 columns of dG0[g][j] x[p][j]
//   dW sum          dW_ih0[g][k] = wpart[0] + wpart[1] + ...                                 (ascending tile)
// Chunk and tile sizes are constants, so the place of a term in a sum of row b follows from (k, t) alone: y and dx of a
// row do not depend on the other rows or on B.
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int RL_KC = 128;      // planes per projection chunk (K = 2560: 20 chunks)
constexpr int RL_PC = 64;       // planes per back-projection workgroup
constexpr int RL_COLS = 1024;   // columns per workgroup: 256 threads x 4
constexpr int RL_NSAVE = 12;    // i, f, g, o, c, tanh(c) of layer 0, then of layer 1
constexpr int RL_NPART = 20;    // dW_hh0[4], db0[4], dW_ih1[4], dW_hh1[4], db1[4]

struct Quad {
    bool v[4];
    bool all, any;
};

// which of the columns j0 .. j0 + 3 are frames of a row
__device__ __forceinline__ Quad quad_mask(int j0, int J, int Tp, int T) {
    Quad q;
    q.all = true; q.any = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = j0 + c, tp = j % Tp;
        q.v[c] = j < J && tp >= 1 && tp <= T;
        q.all = q.all && q.v[c];
        q.any = q.any || q.v[c];
    }
    return q;
}

__device__ __forceinline__ f32x4 quad_load(const float* __restrict__ row, int j0, const Quad& q) {
    if (q.all) return *reinterpret_cast<const f32x4*>(row + j0);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (q.v[c]) r[c] = row[j0 + c];
    return r;
}

__device__ __forceinline__ int feature_of_plane(int p, int CF) { return (p % CF) * 2 + p / CF; }
__device__ __forceinline__ int plane_of_feature(int k, int CF) { return (k & 1) * CF + (k >> 1); }

__global__ __launch_bounds__(256) void rl_proj_kernel(const float* __restrict__ x, const float* __restrict__ wih0, int CF, int K,
                                                      int J, int Jp, int Tp, int T, double* __restrict__ part) {
    __shared__ float w[4][RL_KC];
    const int chunk = blockIdx.y, p0 = chunk * RL_KC;
    const int np = min(RL_KC, K - p0);
    for (int idx = threadIdx.x; idx < 4 * np; idx += 256) {
        const int g = idx / np, pp = idx % np;
        w[g][pp] = wih0[(size_t)g * K + feature_of_plane(p0 + pp, CF)];
    }
    __syncthreads();
    const int j0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (j0 >= Jp) return;
    const Quad q = quad_mask(j0, J, Tp, T);
    double acc[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[g][c] = 0.0;
    if (q.any) {
        const float* row = x + (size_t)p0 * Jp;
#pragma unroll 4
        for (int pp = 0; pp < np; ++pp, row += Jp) {
            const f32x4 v = quad_load(row, j0, q);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double wd = (double)w[g][pp];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[g][c] = fma(wd, (double)v[c], acc[g][c]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        double* dst = part + ((size_t)chunk * 4 + g) * Jp + j0;
#pragma unroll
        for (int c = 0; c < 4; ++c) dst[c] = acc[g][c];
    }
}

__global__ __launch_bounds__(256) void rl_gsum_kernel(const double* __restrict__ part, int nchunk, const float* __restrict__ bih0,
                                                      const float* __restrict__ bhh0, int Jp, double* __restrict__ G0) {
    const int j = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (j >= Jp) return;
    double s = (double)bih0[g] + (double)bhh0[g];
    for (int c = 0; c < nchunk; ++c) s += part[((size_t)c * 4 + g) * Jp + j];
    G0[(size_t)g * Jp + j] = s;
}

__device__ __forceinline__ double sigmoid_d(double v) { return 1.0 / (1.0 + exp(-v)); }

// one LSTM cell with hidden size 1: pre[4] = gate pre-activations (i, f, g, o); c is updated, h returned; the activated gates,
// c and tanh(c) go to s[0 .. 5] (stride B doubles) when s != nullptr
__device__ __forceinline__ double cell_d(const double pre[4], double& c, double* __restrict__ s, int B) {
    const double gi = sigmoid_d(pre[0]), gf = sigmoid_d(pre[1]), gg = tanh(pre[2]), go = sigmoid_d(pre[3]);
    c = fma(gf, c, gi * gg);
    const double tc = tanh(c);
    if (s) {
        s[0] = gi; s[(size_t)B] = gf; s[(size_t)2 * B] = gg; s[(size_t)3 * B] = go; s[(size_t)4 * B] = c; s[(size_t)5 * B] = tc;
    }
    return go * tc;
}

// Lanes run along the rows: the recurrence of a row is strictly sequential and 8 gates wide, so a row is one lane's work and
// T steps is the critical path whatever the mapping.  The four gate inputs of the next four steps are loaded into registers
// while the current four steps compute (the loads do not depend on the recurrence), which hides the strided reads of G0.
__global__ __launch_bounds__(64) void rl_scan_kernel(const double* __restrict__ G0, int B, int T, int Tp, int Jp,
                                                     const float* __restrict__ whh0, const float* __restrict__ wih1,
                                                     const float* __restrict__ whh1, const float* __restrict__ bih1,
                                                     const float* __restrict__ bhh1, double* __restrict__ save, float* __restrict__ y) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double u0[4], v1[4], u1[4], b1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        u0[g] = (double)whh0[g]; v1[g] = (double)wih1[g]; u1[g] = (double)whh1[g];
        b1[g] = (double)bih1[g] + (double)bhh1[g];
    }
    const double* gp = G0 + (size_t)b * Tp + 1;
    double cur[4][4], nxt[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) cur[u][g] = u < T ? gp[(size_t)g * Jp + u] : 0.0;
    double h0 = 0.0, c0 = 0.0, h1 = 0.0, c1 = 0.0;
    for (int t0 = 0; t0 < T; t0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) nxt[u][g] = t0 + 4 + u < T ? gp[(size_t)g * Jp + t0 + 4 + u] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u;
            if (t < T) {
                double* s = save ? save + ((size_t)t * RL_NSAVE) * B + b : nullptr;
                double pre[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) pre[g] = fma(u0[g], h0, cur[u][g]);
                h0 = cell_d(pre, c0, s, B);
#pragma unroll
                for (int g = 0; g < 4; ++g) pre[g] = fma(u1[g], h1, fma(v1[g], h0, b1[g]));
                h1 = cell_d(pre, c1, s ? s + (size_t)6 * B : nullptr, B);
                y[(size_t)b * T + t] = (float)h1;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) cur[u][g] = nxt[u][g];
    }
}

struct Step {
    double v[RL_NSAVE];
};

__device__ __forceinline__ Step step_load(const double* __restrict__ save, int t, int B, int b) {
    Step s;
    if (t >= 0) {
        const double* src = save + ((size_t)t * RL_NSAVE) * B + b;
#pragma unroll
        for (int q = 0; q < RL_NSAVE; ++q) s.v[q] = src[(size_t)q * B];
    } else {
#pragma unroll
        for (int q = 0; q < RL_NSAVE; ++q) s.v[q] = 0.0;
    }
    return s;
}

// gate gradients of one cell: s = (i, f, g, o, c, tanh c) of this step, cprev = c of the step before, dh = gradient arriving
// at h, dcn = gradient arriving at c from the step after (replaced by the one handed to the step before)
__device__ __forceinline__ void cell_bwd_d(const double* s, double cprev, double dh, double& dcn, double dG[4]) {
    const double gi = s[0], gf = s[1], gg = s[2], go = s[3], tc = s[5];
    const double dc = fma(dh * go, 1.0 - tc * tc, dcn);
    dG[0] = dc * gg * gi * (1.0 - gi);
    dG[1] = dc * cprev * gf * (1.0 - gf);
    dG[2] = dc * gi * (1.0 - gg * gg);
    dG[3] = dh * tc * go * (1.0 - go);
    dcn = dc * gf;
}

__global__ __launch_bounds__(64) void rl_bptt_kernel(const double* __restrict__ save, const float* __restrict__ dy, int B, int T, int Tp,
                                                     int Jp, const float* __restrict__ whh0, const float* __restrict__ wih1,
                                                     const float* __restrict__ whh1, double* __restrict__ dG0, double* __restrict__ part) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double u0[4], v1[4], u1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { u0[g] = (double)whh0[g]; v1[g] = (double)wih1[g]; u1[g] = (double)whh1[g]; }
    double acc[RL_NPART];
#pragma unroll
    for (int q = 0; q < RL_NPART; ++q) acc[q] = 0.0;
    double dG0n[4] = {0.0, 0.0, 0.0, 0.0}, dG1n[4] = {0.0, 0.0, 0.0, 0.0};
    double dc0n = 0.0, dc1n = 0.0;
    Step cur = step_load(save, T - 1, B, b), prv = step_load(save, T - 2, B, b);
    const float* dyr = dy + (size_t)b * T;
    float dyc = dyr[T - 1];
    double* out = dG0 + (size_t)b * Tp + 1;
    for (int t = T - 1; t >= 0; --t) {
        const Step pp = step_load(save, t - 2, B, b);              // needed two iterations from now
        const float dyn = t > 0 ? dyr[t - 1] : 0.f;
        const double h0 = cur.v[3] * cur.v[5];
        const double h0p = prv.v[3] * prv.v[5], h1p = prv.v[9] * prv.v[11];
        // layer 1
        double dh1 = (double)dyc;
#pragma unroll
        for (int g = 0; g < 4; ++g) dh1 = fma(u1[g], dG1n[g], dh1);
        double dG1[4];
        cell_bwd_d(cur.v + 6, prv.v[10], dh1, dc1n, dG1);
        // layer 0
        double dh0 = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g) dh0 = fma(v1[g], dG1[g], dh0);
#pragma unroll
        for (int g = 0; g < 4; ++g) dh0 = fma(u0[g], dG0n[g], dh0);
        double dG0c[4];
        cell_bwd_d(cur.v, prv.v[4], dh0, dc0n, dG0c);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            acc[g] = fma(dG0c[g], h0p, acc[g]);
            acc[4 + g] += dG0c[g];
            acc[8 + g] = fma(dG1[g], h0, acc[8 + g]);
            acc[12 + g] = fma(dG1[g], h1p, acc[12 + g]);
            acc[16 + g] += dG1[g];
            out[(size_t)g * Jp + t] = dG0c[g];
            dG0n[g] = dG0c[g];
            dG1n[g] = dG1[g];
        }
        cur = prv; prv = pp; dyc = dyn;
    }
#pragma unroll
    for (int q = 0; q < RL_NPART; ++q) part[(size_t)q * B + b] = acc[q];
}

// out[28] = dW_hh0[4], db_ih0[4], db_hh0[4], dW_ih1[4], dW_hh1[4], db_ih1[4], db_hh1[4]
__global__ __launch_bounds__(64) void rl_small_kernel(const double* __restrict__ part, int B, float* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= RL_NPART) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += part[(size_t)q * B + b];
    const int grp = q >> 2, g = q & 3;
    const float v = (float)s;
    if (grp == 0) out[g] = v;
    else if (grp == 1) { out[4 + g] = v; out[8 + g] = v; }
    else if (grp == 2) out[12 + g] = v;
    else if (grp == 3) out[16 + g] = v;
    else { out[20 + g] = v; out[24 + g] = v; }
}

template <bool DX, bool DW>
__global__ __launch_bounds__(256) void rl_back_kernel(const float* __restrict__ x, const double* __restrict__ dG0,
                                                      const float* __restrict__ wih0, int CF, int K, int J, int Jp, int Tp, int T,
                                                      float* __restrict__ dx, double* __restrict__ wpart) {
    __shared__ float w[4][RL_PC];
    __shared__ double red[RL_PC][4][4];           // [plane][wave][gate]
    const int tile = blockIdx.x, p0 = blockIdx.y * RL_PC;
    const int np = min(RL_PC, K - p0);
    if (DX) {
        for (int idx = threadIdx.x; idx < 4 * np; idx += 256) {
            const int g = idx / np, pp = idx % np;
            w[g][pp] = wih0[(size_t)g * K + feature_of_plane(p0 + pp, CF)];
        }
        __syncthreads();
    }
    const int j0 = (tile * 256 + threadIdx.x) * 4;
    const bool inr = j0 < Jp;
    Quad q;
    if (inr) q = quad_mask(j0, J, Tp, T);
    else { q.all = q.any = false; q.v[0] = q.v[1] = q.v[2] = q.v[3] = false; }
    double dg[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) dg[g][c] = q.v[c] ? dG0[(size_t)g * Jp + j0 + c] : 0.0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int pp = 0; pp < np; ++pp) {
        const size_t off = (size_t)(p0 + pp) * Jp;
        if (DW) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q.any) v = quad_load(x + off, j0, q);
            double s[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                s[g] = 0.0;
#pragma unroll
                for (int c = 0; c < 4; ++c) s[g] = fma(dg[g][c], (double)v[c], s[g]);
                s[g] = wave_sum_d(s[g]);
            }
            if (lane == 0) {
#pragma unroll
                for (int g = 0; g < 4; ++g) red[pp][wave][g] = s[g];
            }
        }
        if (DX && inr) {
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double a = 0.0;
#pragma unroll
                for (int g = 0; g < 4; ++g) a = fma((double)w[g][pp], dg[g][c], a);
                o[c] = (float)a;
            }
            *reinterpret_cast<f32x4*>(dx + off + j0) = o;
        }
    }
    if (DW) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < 4 * np; idx += 256) {
            const int g = idx / np, pp = idx % np;
            const double s = ((red[pp][0][g] + red[pp][1][g]) + red[pp][2][g]) + red[pp][3][g];
            wpart[((size_t)tile * 4 + g) * K + p0 + pp] = s;
        }
    }
}

__global__ __launch_bounds__(256) void rl_dw_kernel(const double* __restrict__ wpart, int ntile, int CF, int K, float* __restrict__ dw) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 4 * K) return;
    const int g = idx / K, k = idx % K;
    const int p = plane_of_feature(k, CF);
    double s = 0.0;
    for (int tl = 0; tl < ntile; ++tl) s += wpart[((size_t)tl * 4 + g) * K + p];
    dw[idx] = (float)s;
}

// ---- LSGAN: out[0] = (sum (a - 1)^2 + sum b^2) / n, b may be absent.  One workgroup: thread i takes elements i, i + 256, ...,
// lanes are added by the butterfly, the four waves in order.
__global__ __launch_bounds__(256) void lsgan_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                    float* __restrict__ out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (long long idx = threadIdx.x; idx < n; idx += 256) {
        const double da = (double)a[idx] - 1.0;
        double e = da * da;
        if (b) { const double vb = (double)b[idx]; e = fma(vb, vb, e); }
        acc += e;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (float)((((sh[0] + sh[1]) + sh[2]) + sh[3]) / (double)n);
}

__global__ __launch_bounds__(256) void lsgan_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                        const float* __restrict__ gout, float* __restrict__ da, float* __restrict__ db) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const double s = 2.0 * (double)gout[0] / (double)n;
    if (da) da[idx] = (float)(s * ((double)a[idx] - 1.0));
    if (db) db[idx] = (float)(s * (double)b[idx]);
}

inline bool misaligned(const void* ptr, uintptr_t a) { return ((uintptr_t)ptr & (a - 1)) != 0; }

constexpr int RL_MAX_B = 65535, RL_MAX_T = 1 << 20, RL_MAX_K = 1 << 16;

// the geometry every LSTM entry takes; K = 2 C F
inline bool geometry_ok(int C, int F, int B, int T, int Tp, int Jp) {
    if (C <= 0 || F <= 0 || B <= 0 || B > RL_MAX_B || T <= 0 || T > RL_MAX_T) return false;
    if ((long long)C * F > RL_MAX_K / 2) return false;
    if (Tp < T + 1 || (Jp & 3)) return false;
    if ((long long)B * Tp > (long long)Jp || (long long)Jp > 0x7fffffffLL - 4 * 256) return false;
    return true;
}

inline int nchunk_of(int K) { return (K + RL_KC - 1) / RL_KC; }
inline int ntile_of(int Jp) { return (Jp + RL_COLS - 1) / RL_COLS; }

}  // namespace

extern "C" long long idv_rlstm1_save_doubles(int B, int T) {
    if (B <= 0 || B > RL_MAX_B || T <= 0 || T > RL_MAX_T) return -1;
    return (long long)RL_NSAVE * B * T;
}

extern "C" long long idv_rlstm1_fwd_scratch_doubles(int K, int Jp) {
    if (K <= 0 || K > RL_MAX_K || Jp <= 0) return -1;
    return (long long)(4 + 4 * nchunk_of(K)) * Jp;
}

extern "C" long long idv_rlstm1_bwd_scratch_doubles(int K, int B, int Jp) {
    if (K <= 0 || K > RL_MAX_K || B <= 0 || B > RL_MAX_B || Jp <= 0) return -1;
    return (long long)4 * Jp + (long long)RL_NPART * B + (long long)ntile_of(Jp) * 4 * K;
}

extern "C" int idv_rlstm1_fwd(const float* x, int C, int F, int B, int T, int Tp, int Jp, const float* wih0, const float* whh0,
                              const float* bih0, const float* bhh0, const float* wih1, const float* whh1, const float* bih1,
                              const float* bhh1, double* save, double* scratch, float* y, void* stream) {
    if (!x || !wih0 || !whh0 || !bih0 || !bhh0 || !wih1 || !whh1 || !bih1 || !bhh1 || !scratch || !y) return IDV_EINVAL;
    if (!geometry_ok(C, F, B, T, Tp, Jp)) return IDV_EINVAL;
    if (misaligned(x, 16) || misaligned(save, 8) || misaligned(scratch, 8) || misaligned(y, 4) || misaligned(wih0, 4) ||
        misaligned(whh0, 4) || misaligned(bih0, 4) || misaligned(bhh0, 4) || misaligned(wih1, 4) || misaligned(whh1, 4) ||
        misaligned(bih1, 4) || misaligned(bhh1, 4))
        return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int CF = C * F, K = 2 * CF, J = B * Tp, nchunk = nchunk_of(K);
    double* G0 = scratch;
    double* part = scratch + (size_t)4 * Jp;
    hipLaunchKernelGGL(rl_proj_kernel, dim3(ntile_of(Jp), nchunk), dim3(256), 0, st, x, wih0, CF, K, J, Jp, Tp, T, part);
    hipLaunchKernelGGL(rl_gsum_kernel, dim3((Jp + 255) / 256, 4), dim3(256), 0, st, (const double*)part, nchunk, bih0, bhh0, Jp, G0);
    hipLaunchKernelGGL(rl_scan_kernel, dim3((B + 63) / 64), dim3(64), 0, st, (const double*)G0, B, T, Tp, Jp, whh0, wih1, whh1, bih1,
                       bhh1, save, y);
    return idv_launch_status();
}

extern "C" int idv_rlstm1_bwd(const float* x, int C, int F, int B, int T, int Tp, int Jp, const float* dy, const float* wih0,
                              const float* whh0, const float* wih1, const float* whh1, const double* save, double* scratch,
                              float* dx, float* dwih0, float* dsmall, void* stream) {
    if (!x || !dy || !wih0 || !whh0 || !wih1 || !whh1 || !save || !scratch || !dsmall) return IDV_EINVAL;
    if (!geometry_ok(C, F, B, T, Tp, Jp)) return IDV_EINVAL;
    if (misaligned(x, 16) || misaligned(dx, 16) || misaligned(save, 8) || misaligned(scratch, 8) || misaligned(dy, 4) ||
        misaligned(wih0, 4) || misaligned(whh0, 4) || misaligned(wih1, 4) || misaligned(whh1, 4) || misaligned(dwih0, 4) ||
        misaligned(dsmall, 4))
        return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int CF = C * F, K = 2 * CF, J = B * Tp, ntile = ntile_of(Jp);
    double* dG0 = scratch;
    double* part = scratch + (size_t)4 * Jp;
    double* wpart = part + (size_t)RL_NPART * B;
    hipLaunchKernelGGL(rl_bptt_kernel, dim3((B + 63) / 64), dim3(64), 0, st, save, dy, B, T, Tp, Jp, whh0, wih1, whh1, dG0, part);
    hipLaunchKernelGGL(rl_small_kernel, dim3(1), dim3(64), 0, st, (const double*)part, B, dsmall);
    const dim3 grid(ntile, (K + RL_PC - 1) / RL_PC);
    if (dx && dwih0)
        hipLaunchKernelGGL((rl_back_kernel<true, true>), grid, dim3(256), 0, st, x, (const double*)dG0, wih0, CF, K, J, Jp, Tp, T, dx, wpart);
    else if (dx)
        hipLaunchKernelGGL((rl_back_kernel<true, false>), grid, dim3(256), 0, st, x, (const double*)dG0, wih0, CF, K, J, Jp, Tp, T, dx, wpart);
    else if (dwih0)
        hipLaunchKernelGGL((rl_back_kernel<false, true>), grid, dim3(256), 0, st, x, (const double*)dG0, wih0, CF, K, J, Jp, Tp, T, dx, wpart);
    if (dwih0)
        hipLaunchKernelGGL(rl_dw_kernel, dim3((4 * K + 255) / 256), dim3(256), 0, st, (const double*)wpart, ntile, CF, K, dwih0);
    return idv_launch_status();
}

extern "C" int idv_lsgan(const float* a, const float* b, long long n, float* out, void* stream) {
    if (!a || !out || n <= 0 || n > (1LL << 28) || misaligned(a, 4) || misaligned(b, 4) || misaligned(out, 4)) return IDV_EINVAL;
    hipLaunchKernelGGL(lsgan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, b, n, out);
    return idv_launch_status();
}

extern "C" int idv_lsgan_bwd(const float* a, const float* b, long long n, const float* gout, float* da, float* db, void* stream) {
    if (!gout || n <= 0 || n > (1LL << 28) || (!da && !db) || (da && !a) || (db && !b)) return IDV_EINVAL;
    if (misaligned(a, 4) || misaligned(b, 4) || misaligned(gout, 4) || misaligned(da, 4) || misaligned(db, 4)) return IDV_EINVAL;
    hipLaunchKernelGGL(lsgan_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, n, gout, da, db);
    return idv_launch_status();
}
