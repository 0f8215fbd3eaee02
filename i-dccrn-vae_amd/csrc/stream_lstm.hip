// Streaming two-layer complex LSTM (model/complex_progress.py:39-74) over the k steps of one push, with h and c of both layers
// carried in device state buffers from push to push.  The layer-0 input projection (W_ih0 x + b_ih0 + b_hh0) comes from
// idv_pw_gemm with the idv_pack_lstm_ih fragments, as in the offline path; this kernel adds W_hh0 h0, runs the cell, then
// layer 1 (W_ih1 h0 + W_hh1 h1 + b1) for the same step.
//
// One workgroup = one run (input part z x weight set s, run = 2z + s) x SB streams; thread r owns gate row r (torch order
// i, f, g, o).  The three [4H][H] matrices of the weight set are read transposed ([H][4H], coalesced along r) from L2 on
// every step: 3 x 256 KiB per weight set at H = 128.  No cooperative launch, no spin-wait.
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int SL_H = 128;
constexpr int SL_SB = 8;

// ROWS (idv_stream_clstm_rows): k is k_launch and stream b runs only its first k_b = rows[b][IDV_ROW_K] steps; from step k_b on
// its h and c of both layers stay as they are, in LDS, in registers and in state, and its rows of hout are zero.
template <bool ROWS>
__device__ __forceinline__ void lstm_body(const float* __restrict__ G, const float* __restrict__ wt, const float* __restrict__ b1,
                                          float* __restrict__ state, float* __restrict__ hout, int B, int k,
                                          const long long* __restrict__ rows) {
    constexpr int H = SL_H, SB = SL_SB, G4 = 4 * H;
    __shared__ float hs0[SB][H], hs1[SB][H], gs[SB][G4];
    const int r = threadIdx.x;
    const int run = blockIdx.y, z = run >> 1, s = run & 1;
    const int b0 = blockIdx.x * SB;
    constexpr int PAIRS = SB * H / G4;              // (stream, unit) pairs whose cells this thread updates
    int kq[PAIRS];                                  // steps of the stream of pair q
    int ksteps = k;                                 // steps this workgroup runs: the most any of its streams has
    if (ROWS) {
        ksteps = 0;
        for (int sb = 0; sb < SB; ++sb)
            if (b0 + sb < B) ksteps = max(ksteps, (int)rows[(size_t)(b0 + sb) * IDV_STREAM_ROW_FIELDS + IDV_ROW_K]);
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) {
            const int b = b0 + (r + q * G4) / H;
            kq[q] = b < B ? (int)rows[(size_t)b * IDV_STREAM_ROW_FIELDS + IDV_ROW_K] : 0;
            for (int t = kq[q]; t < k; ++t)
                if (b < B) hout[((size_t)run * k * B + (size_t)t * B + b) * H + (r + q * G4) % H] = 0.f;
        }
        if (ksteps == 0) return;                    // the same for every thread of the workgroup
    } else {
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) kq[q] = k;
    }
    const float* w_hh0 = wt + (size_t)(s * 3 + 0) * H * G4;
    const float* w_ih1 = wt + (size_t)(s * 3 + 1) * H * G4;
    const float* w_hh1 = wt + (size_t)(s * 3 + 2) * H * G4;
    const float bias1 = b1[s * G4 + r];
    // state[run][layer][h | c][B][H]
    float* st = state + (size_t)run * 4 * B * H;
    const size_t sz = (size_t)B * H;

    float c0[PAIRS], c1[PAIRS];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
        const int e = r + q * G4, sb = e / H, u = e % H, b = b0 + sb;
        const bool ok = b < B;
        hs0[sb][u] = ok ? st[0 * sz + (size_t)b * H + u] : 0.f;
        c0[q] = ok ? st[1 * sz + (size_t)b * H + u] : 0.f;
        hs1[sb][u] = ok ? st[2 * sz + (size_t)b * H + u] : 0.f;
        c1[q] = ok ? st[3 * sz + (size_t)b * H + u] : 0.f;
    }
    // column of gate row r in the idv_pack_lstm_ih order: set s, ((u/16)*4 + g)*16 + u%16
    const int g_r = r / H, u_r = r % H;
    const int colp = s * G4 + ((u_r >> 4) * 4 + g_r) * 16 + (u_r & 15);
    __syncthreads();

    for (int t = 0; t < ksteps; ++t) {
        float acc[SB];
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) {
            const int b = min(b0 + sb, B - 1);
            acc[sb] = G[(size_t)z * k * B * 2 * G4 + ((size_t)t * B + b) * 2 * G4 + colp];
        }
        for (int kk = 0; kk < H; ++kk) {
            const float w = w_hh0[(size_t)kk * G4 + r];
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) acc[sb] = fmaf(w, hs0[sb][kk], acc[sb]);
        }
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) gs[sb][r] = acc[sb];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) {
            const int e = r + q * G4, sb = e / H, u = e % H;
            if (ROWS && t >= kq[q]) continue;
            const float ig = sigmoidf_(gs[sb][u]), fg = sigmoidf_(gs[sb][H + u]);
            const float gg = tanhf_(gs[sb][2 * H + u]), og = sigmoidf_(gs[sb][3 * H + u]);
            c0[q] = fg * c0[q] + ig * gg;
            hs0[sb][u] = og * tanhf_(c0[q]);
        }
        __syncthreads();
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) acc[sb] = bias1;
        for (int kk = 0; kk < H; ++kk) {
            const float w = w_ih1[(size_t)kk * G4 + r];
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) acc[sb] = fmaf(w, hs0[sb][kk], acc[sb]);
        }
        for (int kk = 0; kk < H; ++kk) {
            const float w = w_hh1[(size_t)kk * G4 + r];
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) acc[sb] = fmaf(w, hs1[sb][kk], acc[sb]);
        }
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) gs[sb][r] = acc[sb];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PAIRS; ++q) {
            const int e = r + q * G4, sb = e / H, u = e % H, b = b0 + sb;
            if (ROWS && t >= kq[q]) continue;
            const float ig = sigmoidf_(gs[sb][u]), fg = sigmoidf_(gs[sb][H + u]);
            const float gg = tanhf_(gs[sb][2 * H + u]), og = sigmoidf_(gs[sb][3 * H + u]);
            c1[q] = fg * c1[q] + ig * gg;
            const float h = og * tanhf_(c1[q]);
            hs1[sb][u] = h;
            if (b < B) hout[((size_t)run * k * B + (size_t)t * B + b) * H + u] = h;
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
        const int e = r + q * G4, sb = e / H, u = e % H, b = b0 + sb;
        if (b >= B) continue;
        st[0 * sz + (size_t)b * H + u] = hs0[sb][u];
        st[1 * sz + (size_t)b * H + u] = c0[q];
        st[2 * sz + (size_t)b * H + u] = hs1[sb][u];
        st[3 * sz + (size_t)b * H + u] = c1[q];
    }
}

__global__ __launch_bounds__(4 * SL_H) void stream_lstm_kernel(const float* __restrict__ G, const float* __restrict__ wt,
                                                               const float* __restrict__ b1, float* __restrict__ state,
                                                               float* __restrict__ hout, int B, int k) {
    lstm_body<false>(G, wt, b1, state, hout, B, k, nullptr);
}

__global__ __launch_bounds__(4 * SL_H) void stream_lstm_rows_kernel(const float* __restrict__ G, const float* __restrict__ wt,
                                                                    const float* __restrict__ b1, float* __restrict__ state,
                                                                    float* __restrict__ hout, int B, int k,
                                                                    const long long* __restrict__ rows) {
    lstm_body<true>(G, wt, b1, state, hout, B, k, rows);
}

// real = rr - ii, imag = ir + ri (runs 0, 3, 2, 1) -> planar [2][H][Jp] at column b*Tp + 1 + t
// ROWS (idv_stream_clstm_wide_rows): k is k_launch; the columns t >= k_b of slot b are zero and their rows of h, which no step
// wrote, are not read.
template <bool ROWS>
__global__ void stream_lstm_combine_kernel(const float* __restrict__ h, int H, int B, int k, int Tp, int Jp, float* __restrict__ out,
                                           const long long* __restrict__ rows) {
    const long long n = (long long)H * B * k;
    const size_t run = (size_t)k * B * H;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int u = (int)(e % H);
        const long long tb = e / H;                       // t * B + b
        const int t = (int)(tb / B), b = (int)(tb % B);
        const size_t o = (size_t)tb * H + u;
        const size_t j = (size_t)u * Jp + (size_t)b * Tp + 1 + t;
        if (ROWS && t >= rows[(size_t)b * IDV_STREAM_ROW_FIELDS + IDV_ROW_K]) {
            out[j] = 0.f;
            out[(size_t)H * Jp + j] = 0.f;
            continue;
        }
        out[j] = h[o] - h[3 * run + o];
        out[(size_t)H * Jp + j] = h[2 * run + o] + h[run + o];
    }
}

// ---- wide form (idv_stream_clstm_wide): H up to 768, the hidden sizes of the VAE encoders (3 * zdim * latent_num).
// One launch per layer per step; the stream orders the steps, nothing waits on another workgroup inside a launch.  A workgroup
// (one wave) owns WL_U hidden units of one run for WL_SB streams: thread r holds gate row (r / WL_U) * H + u0 + r % WL_U, so
// all four gates of a unit meet in the workgroup and the cell update is local.  A launch reads h of ALL units of the previous
// step (or of this step's layer 0) while its sibling workgroups write this step's h, so h is never updated in place: step t
// reads the row step t - 1 wrote into hstep (step 0: state) and writes its own row; wide_carry_kernel copies the last rows to
// state afterwards.  c belongs to the unit's workgroup alone and is updated in state.
// Every pre-activation is one fmaf chain in a thread: G (layer 0) or b1 (layer 1) first, then the products in increasing k
// (layer 1: W_ih1 h0, then W_hh1 h1), whatever k, t or the stream's place in its tile is.
constexpr int WL_U = 16;
constexpr int WL_SB = 8;
constexpr int WL_ROWS = 4 * WL_U;
constexpr int WL_HMAX = 768;
constexpr int WL_KB = 16;                            // k per weight block; divides H

// hstep: [2 layers][4 runs][k][B][H]
// ROWS (idv_stream_clstm_wide_rows): k is k_launch and slot b takes part in the steps t < k_b = rows[b][IDV_ROW_K] only.  In a
// step t >= k_b nothing of the slot is written (c in state, its hstep row), and since no step wrote its hstep rows either, zeros
// are staged in their place: its chains run on them and their results are dropped.  A chain belongs to one stream, so an active
// stream's bits do not depend on its tile neighbours.  A workgroup without an active stream returns before its first barrier.
template <int LAYER, bool ROWS>
__global__ __launch_bounds__(WL_ROWS) void wide_step_kernel(const float* __restrict__ G, const float* __restrict__ wt,
                                                            const float* __restrict__ b1, float* __restrict__ state,
                                                            float* __restrict__ hstep, int H, int B, int k, int t,
                                                            const long long* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) float wl_lds[];
    const int KT = (LAYER + 1) * H;                 // layer 0: h0(t-1); layer 1: h0(t) then h1(t-1)
    float* hs = wl_lds;                             // [WL_SB][KT]
    float* gs = wl_lds + (size_t)WL_SB * KT;        // [WL_SB][WL_ROWS]
    const int r = threadIdx.x;
    const int u0 = blockIdx.x * WL_U, run = blockIdx.y, z = run >> 1, s = run & 1;
    const int b0 = blockIdx.z * WL_SB;
    bool act[WL_SB];                                // stream sb runs step t (lock-step: every stream does)
    if (ROWS) {
        bool any = false;
#pragma unroll
        for (int sb = 0; sb < WL_SB; ++sb) {
            act[sb] = b0 + sb < B && t < rows[(size_t)(b0 + sb) * IDV_STREAM_ROW_FIELDS + IDV_ROW_K];
            any = any || act[sb];
        }
        if (!any) return;                           // the same for every thread of the workgroup
    } else {
#pragma unroll
        for (int sb = 0; sb < WL_SB; ++sb) act[sb] = true;
    }
    const int G4 = 4 * H;
    const size_t sz = (size_t)B * H;
    float* st = state + (size_t)run * 4 * sz;       // [layer][h | c][B][H]
    const float* h0row = hstep + ((size_t)run * k) * sz;
    const float* h1row = hstep + ((size_t)(4 + run) * k) * sz;
    const float* src0 = LAYER == 0 ? (t == 0 ? st : h0row + (size_t)(t - 1) * sz) : h0row + (size_t)t * sz;
    const float* src1 = t == 0 ? st + 2 * sz : h1row + (size_t)(t - 1) * sz;
    for (int u = r; u < H; u += WL_ROWS) {          // the loads of the 8 streams are independent: all in flight together
        float v0[WL_SB], v1[WL_SB];
#pragma unroll
        for (int sb = 0; sb < WL_SB; ++sb) {
            const size_t o = (size_t)min(b0 + sb, B - 1) * H + u;
            v0[sb] = (!ROWS || act[sb]) ? src0[o] : 0.f;
            if (LAYER == 1) v1[sb] = (!ROWS || act[sb]) ? src1[o] : 0.f;
        }
#pragma unroll
        for (int sb = 0; sb < WL_SB; ++sb) {
            hs[sb * KT + u] = v0[sb];
            if (LAYER == 1) hs[sb * KT + H + u] = v1[sb];
        }
    }
    __syncthreads();

    const int g_r = r / WL_U, row = g_r * H + u0 + (r % WL_U);
    float acc[WL_SB];
    if (LAYER == 0) {
        // column of gate row `row` in the idv_pack_lstm_ih order, set s: ((u/16)*4 + g)*16 + u%16 = 64 * (u0/16) + r
        const int colp = s * G4 + u0 * 4 + r;
#pragma unroll
        for (int sb = 0; sb < WL_SB; ++sb) {
            const int b = min(b0 + sb, B - 1);
            acc[sb] = G[((size_t)z * k * B + (size_t)t * B + b) * 2 * G4 + colp];
        }
    } else {
        const float bias1 = b1[s * G4 + row];
#pragma unroll
        for (int sb = 0; sb < WL_SB; ++sb) acc[sb] = bias1;
    }
    const float* w = wt + (size_t)(s * 3 + (LAYER == 0 ? 0 : 1)) * H * G4 + row;     // W_hh0 | W_ih1 followed by W_hh1, [H][4H] each
    // blocks of WL_KB k: the weights of the next block are loaded (WL_KB independent loads) while this block's chains run;
    // KT % WL_KB == 0 as H % 16 == 0, and the last block reloads itself instead of reading past the matrices
    float wv[WL_KB];
#pragma unroll
    for (int j = 0; j < WL_KB; ++j) wv[j] = w[(size_t)j * G4];
    for (int k0 = 0; k0 < KT; k0 += WL_KB) {
        const int kn = k0 + WL_KB < KT ? k0 + WL_KB : k0;
        float wn[WL_KB];
#pragma unroll
        for (int j = 0; j < WL_KB; ++j) wn[j] = w[(size_t)(kn + j) * G4];
#pragma unroll
        for (int j4 = 0; j4 < WL_KB; j4 += 4) {
            f32x4 hv[WL_SB];
#pragma unroll
            for (int sb = 0; sb < WL_SB; ++sb) hv[sb] = *reinterpret_cast<const f32x4*>(hs + sb * KT + k0 + j4);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int sb = 0; sb < WL_SB; ++sb) acc[sb] = fmaf(wv[j4 + jj], hv[sb][jj], acc[sb]);
        }
#pragma unroll
        for (int j = 0; j < WL_KB; ++j) wv[j] = wn[j];
    }
#pragma unroll
    for (int sb = 0; sb < WL_SB; ++sb) gs[sb * WL_ROWS + r] = acc[sb];
    __syncthreads();

    float* cst = st + (size_t)(2 * LAYER + 1) * sz;
    float* hout = hstep + ((size_t)(LAYER * 4 + run) * k + t) * sz;
    for (int e = r; e < WL_SB * WL_U; e += WL_ROWS) {
        const int sb = e / WL_U, ul = e % WL_U, b = b0 + sb;
        if (b >= B) continue;
        if (ROWS && t >= rows[(size_t)b * IDV_STREAM_ROW_FIELDS + IDV_ROW_K]) continue;
        const float* gq = gs + sb * WL_ROWS + ul;
        const float ig = sigmoidf_(gq[0]), fg = sigmoidf_(gq[WL_U]);
        const float gg = tanhf_(gq[2 * WL_U]), og = sigmoidf_(gq[3 * WL_U]);
        const size_t o = (size_t)b * H + u0 + ul;
        const float c = fg * cst[o] + ig * gg;
        cst[o] = c;
        hout[o] = og * tanhf_(c);
    }
}

// h of both layers after the last step -> state (the c halves are already there)
// ROWS: the last step of slot b is k_b - 1; a slot with k_b = 0 keeps its state
template <bool ROWS>
__global__ void wide_carry_kernel(const float* __restrict__ hstep, float* __restrict__ state, int H, int B, int k,
                                  const long long* __restrict__ rows) {
    const size_t sz = (size_t)B * H;
    const long long n = 8LL * (long long)sz;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int lr = (int)(e / (long long)sz), layer = lr >> 2, run = lr & 3;
        const size_t o = (size_t)(e % (long long)sz);
        int last = k - 1;
        if (ROWS) {
            last = (int)rows[(o / H) * IDV_STREAM_ROW_FIELDS + IDV_ROW_K] - 1;
            if (last < 0) continue;
        }
        state[((size_t)run * 4 + 2 * layer) * sz + o] = hstep[((size_t)lr * k + last) * sz + o];
    }
}

}  // namespace

static const long long* const no_rows = nullptr;      // the table argument of a lock-step instantiation, which never reads it

extern "C" int idv_stream_lstm_supported(int H) { return H == SL_H ? 1 : 0; }

extern "C" int idv_stream_clstm_wide_supported(int H) { return (H >= WL_U && H <= WL_HMAX && H % WL_U == 0) ? 1 : 0; }

extern "C" long long idv_stream_clstm_wide_hstep_floats(int H, int B, int k) {
    if (!idv_stream_clstm_wide_supported(H) || B <= 0 || k <= 0) return -1;
    return 8LL * k * B * H;
}

extern "C" int idv_stream_clstm_wide(const float* G, const float* wt, const float* b1, float* state, float* hstep, float* out, int H,
                                     int B, int k, int Tp, int Jp, void* stream) {
    if (!G || !wt || !b1 || !state || !hstep || !out || B <= 0 || k <= 0 || Tp < k + 1 || Jp < B * Tp) return IDV_EINVAL;
    if (!idv_stream_clstm_wide_supported(H)) return IDV_EINVAL;
    const long long tiles = ((long long)B + WL_SB - 1) / WL_SB;
    if (tiles > 65535) return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(H / WL_U), 4, (unsigned)tiles);
    const size_t lds0 = sizeof(float) * WL_SB * ((size_t)H + WL_ROWS), lds1 = sizeof(float) * WL_SB * ((size_t)2 * H + WL_ROWS);
    for (int t = 0; t < k; ++t) {
        hipLaunchKernelGGL((wide_step_kernel<0, false>), grid, dim3(WL_ROWS), lds0, st, G, wt, b1, state, hstep, H, B, k, t, no_rows);
        hipLaunchKernelGGL((wide_step_kernel<1, false>), grid, dim3(WL_ROWS), lds1, st, G, wt, b1, state, hstep, H, B, k, t, no_rows);
    }
    int rc = idv_launch_status();
    if (rc) return rc;
    long long g = ((long long)H * B * k + 255) / 256;
    g = g > 4096 ? 4096 : (g < 1 ? 1 : g);
    hipLaunchKernelGGL(stream_lstm_combine_kernel<false>, dim3((unsigned)g), dim3(256), 0, st, hstep + (size_t)4 * k * B * H, H, B, k, Tp,
                       Jp, out, no_rows);
    long long gc = (8LL * B * H + 255) / 256;
    gc = gc > 4096 ? 4096 : gc;
    hipLaunchKernelGGL(wide_carry_kernel<false>, dim3((unsigned)gc), dim3(256), 0, st, hstep, state, H, B, k, no_rows);
    return idv_launch_status();
}

extern "C" int idv_stream_clstm_wide_rows(const float* G, const float* wt, const float* b1, float* state, float* hstep, float* out,
                                          int H, int B, int k_launch, int Tp, int Jp, const long long* rows, void* stream) {
    const int k = k_launch;
    if (!G || !wt || !b1 || !state || !hstep || !out || !rows || B <= 0 || k <= 0 || Tp < k + 1 || Jp < B * Tp) return IDV_EINVAL;
    if (!idv_stream_clstm_wide_supported(H)) return IDV_EINVAL;
    const long long tiles = ((long long)B + WL_SB - 1) / WL_SB;
    if (tiles > 65535) return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(H / WL_U), 4, (unsigned)tiles);
    const size_t lds0 = sizeof(float) * WL_SB * ((size_t)H + WL_ROWS), lds1 = sizeof(float) * WL_SB * ((size_t)2 * H + WL_ROWS);
    for (int t = 0; t < k; ++t) {
        hipLaunchKernelGGL((wide_step_kernel<0, true>), grid, dim3(WL_ROWS), lds0, st, G, wt, b1, state, hstep, H, B, k, t, rows);
        hipLaunchKernelGGL((wide_step_kernel<1, true>), grid, dim3(WL_ROWS), lds1, st, G, wt, b1, state, hstep, H, B, k, t, rows);
    }
    int rc = idv_launch_status();
    if (rc) return rc;
    long long g = ((long long)H * B * k + 255) / 256;
    g = g > 4096 ? 4096 : (g < 1 ? 1 : g);
    hipLaunchKernelGGL(stream_lstm_combine_kernel<true>, dim3((unsigned)g), dim3(256), 0, st, hstep + (size_t)4 * k * B * H, H, B, k, Tp,
                       Jp, out, rows);
    long long gc = (8LL * B * H + 255) / 256;
    gc = gc > 4096 ? 4096 : gc;
    hipLaunchKernelGGL(wide_carry_kernel<true>, dim3((unsigned)gc), dim3(256), 0, st, hstep, state, H, B, k, rows);
    return idv_launch_status();
}

// rows NULL: the lock-step entry
static int launch_clstm(const float* G, const float* wt, const float* b1, float* state, float* hout, float* out, int H, int B, int k,
                        int Tp, int Jp, const long long* rows, void* stream) {
    if (!G || !wt || !b1 || !state || !hout || !out || B <= 0 || k <= 0 || Tp < k + 1 || Jp < B * Tp) return IDV_EINVAL;
    if (!idv_stream_lstm_supported(H)) return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + SL_SB - 1) / SL_SB), 4);
    if (rows)
        hipLaunchKernelGGL(stream_lstm_rows_kernel, grid, dim3(4 * SL_H), 0, st, G, wt, b1, state, hout, B, k, rows);
    else
        hipLaunchKernelGGL(stream_lstm_kernel, grid, dim3(4 * SL_H), 0, st, G, wt, b1, state, hout, B, k);
    int rc = idv_launch_status();
    if (rc) return rc;
    long long g = ((long long)H * B * k + 255) / 256;
    g = g > 4096 ? 4096 : (g < 1 ? 1 : g);
    hipLaunchKernelGGL(stream_lstm_combine_kernel<false>, dim3((unsigned)g), dim3(256), 0, st, hout, H, B, k, Tp, Jp, out, no_rows);
    return idv_launch_status();
}

extern "C" int idv_stream_clstm(const float* G, const float* wt, const float* b1, float* state, float* hout, float* out, int H, int B,
                                int k, int Tp, int Jp, void* stream) {
    return launch_clstm(G, wt, b1, state, hout, out, H, B, k, Tp, Jp, nullptr, stream);
}

extern "C" int idv_stream_clstm_rows(const float* G, const float* wt, const float* b1, float* state, float* hout, float* out, int H,
                                     int B, int k_launch, int Tp, int Jp, const long long* rows, void* stream) {
    if (!rows) return IDV_EINVAL;
    return launch_clstm(G, wt, b1, state, hout, out, H, B, k_launch, Tp, Jp, rows, stream);
}
