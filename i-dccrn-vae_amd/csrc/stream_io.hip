// Signal ends of the streamers (streaming.py): framing from the carried input ring, the ring update, and the overlap-add with
// the carried overlap, the istft envelope and emission of the samples that became final; then the draws and the repeated skips
// of the VAE streamers.  Each signal-end step is one kernel body, template <bool ROWS>: the lock-step streamers hand it their
// ranges by value (SigRow), the sessions streamers one row per slot in a table.  "Slot b's samples are the lock-step streamer's
// bits" holds for these steps because both forms are the same statements; the host checks of the ranges are shared likewise.
//
// Index conventions (torch.stft / torch.istft, center=True, reflect padding; model/pvae_module.py:12-42): half = n_fft/2,
// left = (n_fft - win)/2.  Frame t holds original samples s = hop*t + left - half + i, i in [0, win); s < 0 reads x[-s], and
// at the end of the signal (L known) s >= L reads x[2(L-1) - s].  Output sample m sits at padded position P = m + half and
// collects frame t at window index P - hop*t - left.  The host-side schedule (streaming.StreamPlan / SessionPlan) computes every
// range these kernels are given.
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

inline int grid_of(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

// What the signal-end kernels read of a slot's row (the IDV_ROW_* fields of include/idccrn_hip.h).  A lock-step launch is handed
// one by value, for all B rows alike; a sessions launch loads row b of its table.
struct SigRow {
    long long n_prev, count, L_end, t0, k, parity, e0, e1, p_end, carry_in, T_total, y_off;
};

__device__ __forceinline__ SigRow load_row(const long long* __restrict__ rows, int b) {
    const long long* r = rows + (size_t)b * IDV_STREAM_ROW_FIELDS;
    return {r[IDV_ROW_N_PREV], r[IDV_ROW_COUNT], r[IDV_ROW_L_END], r[IDV_ROW_T0],       r[IDV_ROW_K],       r[IDV_ROW_PARITY],
            r[IDV_ROW_E0],     r[IDV_ROW_E1],    r[IDV_ROW_P_END], r[IDV_ROW_CARRY_IN], r[IDV_ROW_T_TOTAL], r[IDV_ROW_Y_OFF]};
}

// Each step below is one body.  ROWS = false (StreamingDCCRN): `lock` holds the ranges and the table is never read, so no lane
// loads a row; ROWS = true (StreamingSessions): slot b takes its ranges from row b, which differs from lane to lane.  ROWS is
// a compile-time constant for that reason, as in stream_conv.hpp and stream_lstm.hip.

// frames[i][b*Tp + 1 + tl] for the frames t0 .. t0+k-1, tl < k_launch (lock-step: k = k_launch); samples below n_prev come from
// ring[b][s mod R], the others from x[b][s - n_prev] (this push's input, row stride ldx).  ROWS: the columns tl >= k_b of a
// slot are zeroed: the kernels downstream run over all k_launch columns and must not meet stale data.
template <bool ROWS>
__global__ void stream_frames_kernel(const float* __restrict__ ring, int R, const float* __restrict__ x, long long ldx, SigRow lock,
                                     const long long* __restrict__ rows, int B, int n_fft, int win, int hop, int k_launch,
                                     float* __restrict__ frames, int Tp, int Jp) {
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long n = (long long)win * B * k_launch;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int tl = (int)(e % k_launch);
        const int b = (int)((e / k_launch) % B);
        const int i = (int)(e / ((long long)k_launch * B));
        const SigRow r = ROWS ? load_row(rows, b) : lock;
        float v = 0.f;
        if (!ROWS || tl < r.k) {
            long long s = (long long)hop * (r.t0 + tl) + left - half + i;
            if (s < 0) s = -s;
            if (r.L_end >= 0 && s >= r.L_end) s = 2 * (r.L_end - 1) - s;
            v = s >= r.n_prev ? x[(size_t)b * ldx + (size_t)(s - r.n_prev)] : ring[(size_t)b * R + (size_t)(s % R)];
        }
        frames[(size_t)i * Jp + (size_t)b * Tp + 1 + tl] = v;
    }
}

// the last min(count, R) of the count new samples of a row go to the ring at the row's position; n_max = min(widest count, R)
// sizes the launch (lock-step: count = n_new for every row, so every j < n_max is written)
template <bool ROWS>
__global__ void stream_ring_kernel(float* __restrict__ ring, int R, const float* __restrict__ x, long long ldx, int n_max, SigRow lock,
                                   const long long* __restrict__ rows, int B) {
    const long long n = (long long)n_max * B;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(e / n_max);
        const long long j = e % n_max;
        const SigRow r = ROWS ? load_row(rows, b) : lock;
        const long long first = r.count > R ? r.count - R : 0;          // index into x[b] of the oldest sample kept
        if (ROWS && first + j >= r.count) continue;
        const long long s = r.n_prev + first + j;
        ring[(size_t)b * R + (size_t)(s % R)] = x[(size_t)b * ldx + (size_t)(first + j)];
    }
}

// padded positions P in [p_start, p_end), p_start = half + e0, at most span_max of them per row (lock-step: exactly): carried
// partial sum (positions below p_start + carry_in) plus the frames t0 .. t0+k-1 in increasing t; P - half < e1 is final and
// goes to y at y_off (times 1 / envelope as idv_make_dft computes it), the rest becomes the carry for positions from half + e1
// on.  Lock-step: cin and cout_ are the carry read and the carry written.  ROWS: both are the [2][B][cap] carry, of which slot
// b reads half parity_b and writes the other; a slot that sits the group out leaves its carry where it is.
template <bool ROWS>
__global__ void stream_ola_kernel(const float* __restrict__ frames, int Tp, int Jp, const float* cin, float* cout_, int cap, SigRow lock,
                                  const long long* __restrict__ rows, int B, int n_fft, int win, int hop, long long span_max,
                                  float* __restrict__ y, long long ldy) {
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long n = span_max * B;
    const double two_pi = 6.283185307179586476925286766559;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(e / span_max);
        const SigRow r = ROWS ? load_row(rows, b) : lock;
        const int k = (int)r.k;
        if (ROWS && k == 0 && r.e0 == r.e1) continue;
        const long long p_start = half + r.e0, p_new = half + r.e1;
        const long long P = p_start + e % span_max;
        if (ROWS && P >= r.p_end) continue;
        const float* ci = ROWS ? cin + (size_t)r.parity * B * cap : cin;
        float* co = ROWS ? cout_ + (size_t)(1 - r.parity) * B * cap : cout_;
        float v = (P - p_start < r.carry_in) ? ci[(size_t)b * cap + (size_t)(P - p_start)] : 0.f;
        for (int tl = 0; tl < k; ++tl) {
            const long long i = P - (long long)hop * (r.t0 + tl) - left;
            if (i >= 0 && i < win) v += frames[(size_t)i * Jp + (size_t)b * Tp + 1 + tl];
        }
        if (P < p_new) {
            // frames whose window covers P: P - win < hop*t + left <= P (at most ceil(win/hop) of them, wherever the stream is)
            double env = 0.0;
            long long t_hi = (P - left) / hop;
            if (r.T_total >= 0 && t_hi > r.T_total - 1) t_hi = r.T_total - 1;
            long long t_lo = P - left - win >= 0 ? (P - left - win) / hop + 1 : 0;
            for (long long t = t_lo; t <= t_hi; ++t) {
                const long long i = P - (long long)hop * t - left;
                if (i >= 0 && i < win) {
                    const double wn = 0.5 - 0.5 * cos(two_pi * i / win);
                    env += wn * wn;
                }
            }
            const float inv = env > 1e-11 ? (float)(1.0 / env) : 0.f;
            y[(size_t)b * ldy + (size_t)(r.y_off + P - p_start)] = v * inv;
        } else {
            co[(size_t)b * cap + (size_t)(P - p_new)] = v;
        }
    }
}

// buf viewed as [outer][B][inner]: zero the slots listed
__global__ void stream_zero_rows_kernel(float* __restrict__ buf, long long outer, int B, long long inner,
                                        const long long* __restrict__ slots, int n_slots) {
    const long long per = outer * inner, n = per * n_slots;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long b = slots[e / per], r = e % per;
        buf[((size_t)(r / inner) * B + (size_t)b) * inner + (size_t)(r % inner)] = 0.f;
    }
}

// ---- streaming.StreamingVAE: the Gaussian draws of the reparameterisation and the skips at batch B * ns

// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32x32 -> 64 multiplies, the key bumped by the Weyl constants
__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t& w0, uint32_t& w1, uint32_t& w2, uint32_t& w3) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w0 = c0;
    w1 = c1;
    w2 = c2;
    w3 = c3;
}

// two words of a Philox block -> one complex Gaussian draw (Box-Muller in fp32)
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& re, float& im) {
    const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;                  // (0, 1]
    const float th = 6.283185307179586476925286766559f * ((float)(wb >> 8) * 0x1p-24f);
    const float rad = sqrtf(-2.0f * logf(u1));
    re = rad * cosf(th);
    im = rad * sinf(th);
}

// eps_r, eps_i [B][ns][k][zdim] for frames t0 .. t0+k-1: counter (t low, t high, b*ns + s, u), key (seed low, seed high); words
// 0 and 1 through Box-Muller.  A draw depends on (seed, b, s, t, u) only.
// ROWS (idv_stream_eps_rows): k is k_launch, slot b = bs / ns starts at its own t0_b and draws its first k_b frames; the rest of
// its entries are zero.
// PAIR (idv_stream_eps_pair): words 2 and 3 of the same block through the same Box-Muller give a second, independent pair
// (eps2_r, eps2_i), the noise latent's draws; words 0 and 1 are what the kernel without PAIR writes.
// SEEDS (idv_stream_eps_pair_rows, with ROWS): the key of slot b is seeds[b] in place of seed.  seeds is the last parameter, so
// the kernel arguments of the forms without SEEDS sit where they sat.
// AS (idv_stream_eps_pair_rows_as, with SEEDS): the counter word of slot b is draw_slots[b] * ns + s in place of b * ns + s, so
// a stream that was saved in slot draw_slots[b] and loaded into slot b keeps its draws.  draw_slots is the last parameter, for
// the same reason.
template <bool ROWS, bool PAIR, bool SEEDS, bool AS = false>
__global__ void stream_eps_kernel(unsigned long long seed, long long t0, int k, int Bn, int zdim, float* __restrict__ eps_r,
                                  float* __restrict__ eps_i, float* __restrict__ eps2_r, float* __restrict__ eps2_i, int ns,
                                  const long long* __restrict__ rows, const long long* __restrict__ seeds,
                                  const long long* __restrict__ draw_slots) {
    static_assert(ROWS || !SEEDS, "per-slot seeds come with the row table");
    static_assert(SEEDS || !AS, "per-slot draw slots come with the per-slot seeds");
    const long long n = (long long)Bn * k * zdim;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const uint32_t u = (uint32_t)(e % zdim);
        const long long tl = (e / zdim) % k;
        const uint32_t bs = (uint32_t)(e / ((long long)zdim * k));
        uint32_t word = bs;                                                    // counter word 2: b * ns + s
        if (ROWS) {
            const uint32_t b = bs / (uint32_t)ns;
            const long long* row = rows + (size_t)b * IDV_STREAM_ROW_FIELDS;
            if (tl >= row[IDV_ROW_K]) {
                eps_r[e] = 0.f;
                eps_i[e] = 0.f;
                if (PAIR) {
                    eps2_r[e] = 0.f;
                    eps2_i[e] = 0.f;
                }
                continue;
            }
            t0 = row[IDV_ROW_T0];
            if (SEEDS) seed = (unsigned long long)seeds[b];
            if (AS) word = (uint32_t)draw_slots[b] * (uint32_t)ns + (bs - b * (uint32_t)ns);
        }
        const unsigned long long t = (unsigned long long)(t0 + tl);
        uint32_t w0, w1, w2, w3;
        philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)t, (uint32_t)(t >> 32), word, u, w0, w1, w2, w3);
        box_muller(w0, w1, eps_r[e], eps_i[e]);
        if (PAIR) box_muller(w2, w3, eps2_r[e], eps2_i[e]);
    }
}

// rows of x (pitch Jp, column b*Tp + 1 + tl, tl < k) -> xn (pitch Jpn, column (b*ns + s)*Tp + 1 + tl); hist[rows][B] -> histn[rows][B*ns]
// ROWS (idv_stream_repeat_rows): k is k_launch, hist / histn hold two parity halves; the columns tl < k_b of slot b and its
// history of half parity_b (to the same half of histn) are copied, and a slot with k_b = 0 is not touched.
template <bool ROWS>
__global__ void stream_repeat_kernel(const float* __restrict__ x, const float* __restrict__ hist, long long rows, int B, int ns, int k,
                                     int Tp, int Jp, float* __restrict__ xn, float* __restrict__ histn, int Jpn,
                                     const long long* __restrict__ table) {
    const int Bn = B * ns, kc = k + 1;                                        // column kc - 1 of a row's span stands for the history
    const long long n = rows * Bn * kc;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int tl = (int)(e % kc);
        const int bn = (int)((e / kc) % Bn);
        const long long row = e / ((long long)kc * Bn);
        const int b = bn / ns;
        size_t half = 0, halfn = 0;                                           // offsets of the history half read
        if (ROWS) {
            const long long kb = table[(size_t)b * IDV_STREAM_ROW_FIELDS + IDV_ROW_K];
            if (kb == 0 || (tl < k && tl >= kb)) continue;
            const size_t par = (size_t)table[(size_t)b * IDV_STREAM_ROW_FIELDS + IDV_ROW_PARITY];
            half = par * (size_t)rows * B;
            halfn = par * (size_t)rows * Bn;
        }
        if (tl < k)
            xn[(size_t)row * Jpn + (size_t)bn * Tp + 1 + tl] = x[(size_t)row * Jp + (size_t)b * Tp + 1 + tl];
        else if (hist)
            histn[halfn + (size_t)row * Bn + bn] = hist[half + (size_t)row * B + b];
    }
}

}  // namespace

static const long long* const no_rows = nullptr;      // the table argument of a lock-step instantiation, which never reads it
static const SigRow no_row = {};                      // the by-value row of a ROWS instantiation, which loads its own from the table
static float* const no_eps = nullptr;                 // the second pair of an instantiation without PAIR, which never writes it
static const long long* const no_seeds = nullptr;     // the seed array of an instantiation without SEEDS, which never reads it
static const long long* const no_draw_slots = nullptr;      // the draw slots of an instantiation without AS, which never reads them

extern "C" int idv_stream_eps(long long seed, long long t0, int k, int B, int ns, int zdim, float* eps_r, float* eps_i, void* stream) {
    if (t0 < 0 || k <= 0 || B <= 0 || ns <= 0 || zdim <= 0 || !eps_r || !eps_i || (long long)B * ns > 0x7fffffffLL) return IDV_EINVAL;
    hipLaunchKernelGGL((stream_eps_kernel<false, false, false>), dim3(grid_of((long long)B * ns * k * zdim)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long)seed, t0, k, B * ns, zdim, eps_r, eps_i, no_eps, no_eps, ns, no_rows, no_seeds, no_draw_slots);
    return idv_launch_status();
}

extern "C" int idv_stream_eps_pair(long long seed, long long t0, int k, int B, int ns, int zdim, float* eps_sr, float* eps_si,
                                   float* eps_nr, float* eps_ni, void* stream) {
    if (t0 < 0 || k <= 0 || B <= 0 || ns <= 0 || zdim <= 0 || !eps_sr || !eps_si || !eps_nr || !eps_ni ||
        (long long)B * ns > 0x7fffffffLL)
        return IDV_EINVAL;
    hipLaunchKernelGGL((stream_eps_kernel<false, true, false>), dim3(grid_of((long long)B * ns * k * zdim)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long)seed, t0, k, B * ns, zdim, eps_sr, eps_si, eps_nr, eps_ni, ns, no_rows, no_seeds, no_draw_slots);
    return idv_launch_status();
}

extern "C" int idv_stream_repeat(const float* x, const float* hist, int C, int F, int B, int ns, int k, int Tp, int Jp, float* xn,
                                 float* histn, int Jpn, void* stream) {
    if (!x || !xn || (hist != nullptr) != (histn != nullptr) || C <= 0 || F <= 0 || B <= 0 || ns <= 0 || k <= 0 || Tp < k + 1 ||
        Jp < B * Tp || (long long)B * ns * Tp > Jpn)
        return IDV_EINVAL;
    const long long rows = 2LL * C * F;
    hipLaunchKernelGGL(stream_repeat_kernel<false>, dim3(grid_of(rows * B * ns * (k + 1))), dim3(256), 0, (hipStream_t)stream, x, hist, rows,
                       B, ns, k, Tp, Jp, xn, histn, Jpn, no_rows);
    return idv_launch_status();
}

extern "C" int idv_stream_eps_rows(long long seed, const long long* rows, int B, int ns, int zdim, int k_launch, float* eps_r,
                                   float* eps_i, void* stream) {
    if (!rows || k_launch <= 0 || B <= 0 || ns <= 0 || zdim <= 0 || !eps_r || !eps_i || (long long)B * ns > 0x7fffffffLL)
        return IDV_EINVAL;
    hipLaunchKernelGGL((stream_eps_kernel<true, false, false>), dim3(grid_of((long long)B * ns * k_launch * zdim)), dim3(256), 0,
                       (hipStream_t)stream, (unsigned long long)seed, 0LL, k_launch, B * ns, zdim, eps_r, eps_i, no_eps, no_eps, ns, rows,
                       no_seeds, no_draw_slots);
    return idv_launch_status();
}

extern "C" int idv_stream_eps_pair_rows(const long long* seeds, const long long* rows, int B, int ns, int zdim, int k_launch,
                                        float* eps_sr, float* eps_si, float* eps_nr, float* eps_ni, void* stream) {
    if (!seeds || !rows || k_launch <= 0 || B <= 0 || ns <= 0 || zdim <= 0 || !eps_sr || !eps_si ||
        (eps_nr != nullptr) != (eps_ni != nullptr) || (long long)B * ns > 0x7fffffffLL)
        return IDV_EINVAL;
    const dim3 grid(grid_of((long long)B * ns * k_launch * zdim));
    if (eps_nr)
        hipLaunchKernelGGL((stream_eps_kernel<true, true, true>), grid, dim3(256), 0, (hipStream_t)stream, 0ULL, 0LL, k_launch,
                           B * ns, zdim, eps_sr, eps_si, eps_nr, eps_ni, ns, rows, seeds, no_draw_slots);
    else      // the single-pair form: the speech draws alone
        hipLaunchKernelGGL((stream_eps_kernel<true, false, true>), grid, dim3(256), 0, (hipStream_t)stream, 0ULL, 0LL, k_launch,
                           B * ns, zdim, eps_sr, eps_si, no_eps, no_eps, ns, rows, seeds, no_draw_slots);
    return idv_launch_status();
}

extern "C" int idv_stream_eps_pair_rows_as(const long long* seeds, const long long* draw_slots, const long long* rows, int B, int ns,
                                           int zdim, int k_launch, float* eps_sr, float* eps_si, float* eps_nr, float* eps_ni,
                                           void* stream) {
    if (!seeds || !draw_slots || !rows || k_launch <= 0 || B <= 0 || ns <= 0 || zdim <= 0 || !eps_sr || !eps_si ||
        (eps_nr != nullptr) != (eps_ni != nullptr) || (long long)B * ns > 0x7fffffffLL)
        return IDV_EINVAL;
    const dim3 grid(grid_of((long long)B * ns * k_launch * zdim));
    if (eps_nr)
        hipLaunchKernelGGL((stream_eps_kernel<true, true, true, true>), grid, dim3(256), 0, (hipStream_t)stream, 0ULL, 0LL, k_launch,
                           B * ns, zdim, eps_sr, eps_si, eps_nr, eps_ni, ns, rows, seeds, draw_slots);
    else      // the single-pair form: the speech draws alone
        hipLaunchKernelGGL((stream_eps_kernel<true, false, true, true>), grid, dim3(256), 0, (hipStream_t)stream, 0ULL, 0LL, k_launch,
                           B * ns, zdim, eps_sr, eps_si, no_eps, no_eps, ns, rows, seeds, draw_slots);
    return idv_launch_status();
}

extern "C" int idv_stream_repeat_rows(const float* x, const float* hist, int C, int F, int B, int ns, int k_launch, int Tp, int Jp,
                                      const long long* rows, float* xn, float* histn, int Jpn, void* stream) {
    if (!x || !xn || !rows || (hist != nullptr) != (histn != nullptr) || C <= 0 || F <= 0 || B <= 0 || ns <= 0 || k_launch <= 0 ||
        Tp < k_launch + 1 || Jp < B * Tp || (long long)B * ns * Tp > Jpn)
        return IDV_EINVAL;
    const long long nrow = 2LL * C * F;
    hipLaunchKernelGGL(stream_repeat_kernel<true>, dim3(grid_of(nrow * B * ns * (k_launch + 1))), dim3(256), 0, (hipStream_t)stream, x,
                       hist, nrow, B, ns, k_launch, Tp, Jp, xn, histn, Jpn, rows);
    return idv_launch_status();
}

// The reach and range conditions of a row, shared by the scalar entries and idv_stream_rows_check: a table passes exactly when
// the scalar entry would take each row's values.

// every sample the frames t0 .. t0+k-1 (k > 0) read is in the ring or among the n_new samples of x; the start mirror is there
static bool frames_in_reach(int R, long long n_prev, long long n_new, long long L_end, int n_fft, int win, int hop, long long t0,
                            long long k) {
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    const long long first = (long long)hop * t0 + left - half, last = (long long)hop * (t0 + k - 1) + left - half + win - 1;
    const long long lo_read = first < 0 ? 0 : first;
    const long long hi_read = (L_end >= 0 && last >= L_end) ? L_end - 1 : last;
    return !(hi_read >= n_prev + n_new || (lo_read < n_prev && n_prev - lo_read > R) || (first < 0 && -first >= n_prev + n_new) ||
             (first < 0 && n_prev > R));
}

// the overlap-add ranges: the final samples and the carried positions lie in [half + e0, p_end), the carry written fits cap, and
// the last frame ends inside p_end
static bool ola_in_range(int cap, int n_fft, int win, int hop, long long t0, long long k, long long e0, long long e1, long long p_end,
                         long long carry_in) {
    const int left = (n_fft - win) / 2, half = n_fft / 2;
    return !(p_end < half + e1 || p_end - (half + e0) < carry_in || p_end - (half + e1) > cap ||
             (k > 0 && (long long)hop * (t0 + k - 1) + left + win > p_end));
}

extern "C" int idv_stream_frames(const float* ring, int R, const float* x, long long ldx, int n_new, long long n_prev, long long L_end,
                                 int B, int n_fft, int win, int hop, long long t0, int k, float* frames, int Tp, int Jp, void* stream) {
    if (!ring || R <= 0 || (n_new > 0 && (!x || ldx < n_new)) || n_new < 0 || n_prev < 0 || B <= 0 || n_fft <= 0 || win <= 0 || win > n_fft ||
        hop <= 0 || t0 < 0 || k <= 0 || !frames || Tp < k + 1 || Jp < B * Tp)
        return IDV_EINVAL;
    if (!frames_in_reach(R, n_prev, n_new, L_end, n_fft, win, hop, t0, k)) return IDV_EINVAL;
    SigRow lock = {};
    lock.n_prev = n_prev, lock.L_end = L_end, lock.t0 = t0, lock.k = k;
    hipLaunchKernelGGL(stream_frames_kernel<false>, dim3(grid_of((long long)win * B * k)), dim3(256), 0, (hipStream_t)stream, ring, R, x,
                       ldx, lock, no_rows, B, n_fft, win, hop, k, frames, Tp, Jp);
    return idv_launch_status();
}

extern "C" int idv_stream_ring(float* ring, int R, const float* x, long long ldx, int n_new, long long n_prev, int B, void* stream) {
    if (!ring || R <= 0 || n_new < 0 || (n_new > 0 && (!x || ldx < n_new)) || n_prev < 0 || B <= 0) return IDV_EINVAL;
    if (n_new == 0) return IDV_OK;
    const int n_max = n_new < R ? n_new : R;
    SigRow lock = {};
    lock.n_prev = n_prev, lock.count = n_new;
    hipLaunchKernelGGL(stream_ring_kernel<false>, dim3(grid_of((long long)n_max * B)), dim3(256), 0, (hipStream_t)stream, ring, R, x, ldx,
                       n_max, lock, no_rows, B);
    return idv_launch_status();
}

extern "C" int idv_stream_ola(const float* frames, int Tp, int Jp, const float* carry_in, int carry_in_len, float* carry_out, int cap,
                              int B, int n_fft, int win, int hop, long long t0, int k, long long T_total, long long e0, long long e1,
                              long long p_end, float* y, int ldy, long long y_off, void* stream) {
    if ((k > 0 && !frames) || k < 0 || !carry_in || !carry_out || cap <= 0 || carry_in_len < 0 || carry_in_len > cap || B <= 0 ||
        n_fft <= 0 || win <= 0 || win > n_fft || hop <= 0 || t0 < 0 || e1 < e0 || e0 < 0 || (e1 > e0 && !y) || y_off < 0 ||
        (k > 0 && (Tp < k + 1 || Jp < B * Tp)))
        return IDV_EINVAL;
    if (!ola_in_range(cap, n_fft, win, hop, t0, k, e0, e1, p_end, carry_in_len) || y_off + (e1 - e0) > ldy) return IDV_EINVAL;
    const long long p_start = n_fft / 2 + e0;
    if (p_end <= p_start) return IDV_OK;
    SigRow lock = {};
    lock.t0 = t0, lock.k = k, lock.e0 = e0, lock.e1 = e1, lock.p_end = p_end, lock.carry_in = carry_in_len, lock.T_total = T_total,
    lock.y_off = y_off;
    hipLaunchKernelGGL(stream_ola_kernel<false>, dim3(grid_of((p_end - p_start) * B)), dim3(256), 0, (hipStream_t)stream, frames, Tp, Jp,
                       carry_in, carry_out, cap, lock, no_rows, B, n_fft, win, hop, p_end - p_start, y, (long long)ldy);
    return idv_launch_status();
}

extern "C" int idv_stream_row_fields(void) { return IDV_STREAM_ROW_FIELDS; }

extern "C" int idv_stream_rows_check(const long long* host_rows, int B, int R, int n_x, int n_fft, int win, int hop, int cap,
                                     int k_launch, int Tp, long long ldy, long long span_max) {
    if (!host_rows || B <= 0 || R <= 0 || n_x < 0 || n_fft <= 0 || win <= 0 || win > n_fft || hop <= 0 || cap <= 0 || k_launch < 0 ||
        Tp < k_launch + 1 || ldy < 0 || span_max < 0)
        return IDV_EINVAL;
    for (int b = 0; b < B; ++b) {
        const long long* r = host_rows + (size_t)b * IDV_STREAM_ROW_FIELDS;
        const long long n_prev = r[IDV_ROW_N_PREV], count = r[IDV_ROW_COUNT], L_end = r[IDV_ROW_L_END], t0 = r[IDV_ROW_T0],
                        k = r[IDV_ROW_K], parity = r[IDV_ROW_PARITY], e0 = r[IDV_ROW_E0], e1 = r[IDV_ROW_E1], p_end = r[IDV_ROW_P_END],
                        carry_in = r[IDV_ROW_CARRY_IN], T_total = r[IDV_ROW_T_TOTAL], y_off = r[IDV_ROW_Y_OFF];
        if (n_prev < 0 || count < 0 || count > n_x || L_end < -1 || t0 < 0 || k < 0 || k > k_launch || (parity != 0 && parity != 1) ||
            e0 < 0 || e1 < e0 || carry_in < 0 || carry_in > cap || y_off < 0 || y_off + (e1 - e0) > ldy || (L_end < 0) != (T_total < 0))
            return IDV_EINVAL;
        if (k > 0 && !frames_in_reach(R, n_prev, count, L_end, n_fft, win, hop, t0, k)) return IDV_EINVAL;    // x[b, :count]
        if (k == 0 && e0 == e1) continue;
        if (!ola_in_range(cap, n_fft, win, hop, t0, k, e0, e1, p_end, carry_in) || p_end - (n_fft / 2 + e0) > span_max) return IDV_EINVAL;
    }
    return IDV_OK;
}

extern "C" int idv_stream_frames_rows(const float* ring, int R, const float* x, long long ldx, const long long* rows, int B, int n_fft,
                                      int win, int hop, int k_launch, float* frames, int Tp, int Jp, void* stream) {
    if (!ring || R <= 0 || ldx < 0 || !rows || B <= 0 || n_fft <= 0 || win <= 0 || win > n_fft || hop <= 0 || k_launch <= 0 || !frames ||
        Tp < k_launch + 1 || Jp < B * Tp)
        return IDV_EINVAL;
    hipLaunchKernelGGL(stream_frames_kernel<true>, dim3(grid_of((long long)win * B * k_launch)), dim3(256), 0, (hipStream_t)stream, ring,
                       R, x, ldx, no_row, rows, B, n_fft, win, hop, k_launch, frames, Tp, Jp);
    return idv_launch_status();
}

extern "C" int idv_stream_ring_rows(float* ring, int R, const float* x, long long ldx, int n_x, const long long* rows, int B,
                                    void* stream) {
    if (!ring || R <= 0 || n_x < 0 || (n_x > 0 && (!x || ldx < n_x)) || !rows || B <= 0) return IDV_EINVAL;
    if (n_x == 0) return IDV_OK;
    const int n_max = n_x < R ? n_x : R;
    hipLaunchKernelGGL(stream_ring_kernel<true>, dim3(grid_of((long long)n_max * B)), dim3(256), 0, (hipStream_t)stream, ring, R, x, ldx,
                       n_max, no_row, rows, B);
    return idv_launch_status();
}

extern "C" int idv_stream_ola_rows(const float* frames, int Tp, int Jp, float* carry, int cap, const long long* rows, int B, int n_fft,
                                   int win, int hop, int k_launch, long long span_max, float* y, long long ldy, void* stream) {
    if ((k_launch > 0 && !frames) || k_launch < 0 || !carry || cap <= 0 || !rows || B <= 0 || n_fft <= 0 || win <= 0 || win > n_fft ||
        hop <= 0 || span_max < 0 || ldy < 0 || (ldy > 0 && !y) || (k_launch > 0 && (Tp < k_launch + 1 || Jp < B * Tp)))
        return IDV_EINVAL;
    if (span_max == 0) return IDV_OK;
    hipLaunchKernelGGL(stream_ola_kernel<true>, dim3(grid_of(span_max * B)), dim3(256), 0, (hipStream_t)stream, frames, Tp, Jp, carry, carry,
                       cap, no_row, rows, B, n_fft, win, hop, span_max, y, ldy);
    return idv_launch_status();
}

extern "C" int idv_stream_zero_rows(float* buf, long long outer, int B, long long inner, const long long* slots, int n_slots,
                                    void* stream) {
    if (!buf || outer <= 0 || B <= 0 || inner <= 0 || !slots || n_slots < 0 || n_slots > B) return IDV_EINVAL;
    if (n_slots == 0) return IDV_OK;
    hipLaunchKernelGGL(stream_zero_rows_kernel, dim3(grid_of(outer * inner * n_slots)), dim3(256), 0, (hipStream_t)stream, buf, outer, B,
                       inner, slots, n_slots);
    return idv_launch_status();
}
