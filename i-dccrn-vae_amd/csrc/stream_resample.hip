// Stateful rational polyphase resampler: streaming.StreamingResampler / StreamingResamplerSessions.
//
// The definition is resample.hip's, scipy.signal.resample_poly(x, up, down) with its default filter:
//
//   y[n] = float( up * sum_j x[j] h[half + n*down - j*up] ),  max(0, ceil((n*down - half)/up)) <= j <= min(L - 1, floor((n*down + half)/up))
//
// fp32 samples and taps, one double accumulator per output, j increasing, no atomics.  A product of two floats is exact in double, so
// the bits follow from the order of j alone: a push that adds the same terms in the same order returns the bits of idv_resample.
//
// After P samples output n is final once its last term has arrived, n*down + half < P*up: n_final(P) = max(0, ceil((P*up - half) /
// down)).  A push from position P0 to P1 = P0 + count returns n_final(P0) .. n_final(P1) - 1; the end of a signal of L samples returns
// the rest up to ceil(L*up/down) - 1 with j clipped at L - 1.  No pending output reads further back than H - 1 = floor(2*half/up)
// samples before P0, so the state of a stream is its last H samples: hist[2 parities][B][H], sample P0 - H + k of row b at
// hist[parity][b][k].  Sample j of a row is x[b][j - P0] for j >= P0 and hist[parity][b][H + j - P0] before that.
//
// One launch per push over a flat position space of W = ycols + H positions per row, 256 to a workgroup: position (b, col) is output
// n0_b + col for col < m_b, a zero for m_b <= col < ycols, and from ycols on sample P1 - H + (col - ycols) of the new history, which
// goes to the OTHER parity half: no workgroup reads what another one of the launch writes.  One stream with 100 outputs fills a
// workgroup and 1024 streams fill the device; the cost of a push does not depend on the position (64-bit positions, 32-bit offsets
// from P0).  Two instantiations read the taps differently and add the same terms in the same order: from memory (up > 1: an output
// touches only the 2*half/up + 1 taps of its phase, staging all 2*half + 1 would cost more than the sum) or from LDS at resample.hip's
// skewed index (up = 1: every output reads every tap).  Row b reads nothing at or past x[b][count_b] and nothing of another row.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int SR_MAXM = 640;                          // max(up, down), as resample.hip
constexpr long long SR_MAX_POS = 1LL << 50;           // positions: P * 640 and n * 640 stay far inside 64 bits
constexpr long long SR_MAX_GRID = 2147483647LL - 256; // flat positions of one launch

struct SrRow {          // what one row does in a launch
    long long P0, n0;   // samples before this call; first output of this call
    int count, m;       // new samples x[b][0 .. count-1]; outputs n0 .. n0 + m - 1
    int parity, update; // history half read; whether half 1 - parity receives the new history
};

__host__ __device__ __forceinline__ int skew(int k) { return k + (k >> 5); }
__host__ __device__ __forceinline__ long long fdiv(long long a, long long d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }
__host__ __device__ __forceinline__ long long cdiv(long long a, long long d) { return -fdiv(-a, d); }
inline long long n_final_of(long long P, int up, int down, int half) {
    const long long v = cdiv(P * up - half, down);
    return v > 0 ? v : 0;
}
inline long long n_out_of(long long L, int up, int down) { return (L * up + down - 1) / down; }

template <bool LDS>
__global__ __launch_bounds__(256) void stream_resample_kernel(float* hist, int H, const float* __restrict__ x, long long ldx,
                                                              int n_x, const long long* __restrict__ rows, SrRow lock, int B, int up,
                                                              int down, int half, const float* __restrict__ taps,
                                                              float* __restrict__ y, long long ldy, int ycols, int W) {
    extern __shared__ float hs[];                                  // LDS: skew(2 * half) + 1 floats
    if (LDS) {
        const int ntap = 2 * half + 1;
        for (int k = threadIdx.x; k < ntap; k += 256) hs[skew(k)] = taps[k];
        __syncthreads();
    }
    const long long pos = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pos >= (long long)B * W) return;
    const int b = (int)(pos / W), col = (int)(pos % W);
    SrRow r = lock;
    if (rows) {
        const long long* t = rows + (size_t)b * IDV_SR_ROW_FIELDS;
        r.P0 = t[IDV_SR_ROW_P0];
        r.n0 = t[IDV_SR_ROW_N0];
        // what idv_stream_resample_rows_check holds a table to, once more where it costs nothing: no count past the width of x, no
        // output past the row of y
        r.count = (int)max(0LL, min(t[IDV_SR_ROW_COUNT], (long long)n_x));
        r.m = (int)max(0LL, min(t[IDV_SR_ROW_M], (long long)ycols));
        r.parity = t[IDV_SR_ROW_PARITY] != 0;
        r.update = t[IDV_SR_ROW_IDLE] == 0 && t[IDV_SR_ROW_END] == 0;
    }
    const float* hin = hist + ((size_t)r.parity * B + b) * H + H;  // hin[d], -H <= d < 0: sample P0 + d
    const float* xr = x + (size_t)b * ldx;                          // xr[d], 0 <= d < count: sample P0 + d
    if (col >= ycols) {                                             // the new history: samples P1 - H .. P1 - 1
        if (!r.update) return;
        const int kk = col - ycols, d = r.count - H + kk;           // kk < H: W - ycols is H or 0
        float v = 0.f;
        if (r.P0 + d >= 0) v = d >= 0 ? xr[d] : hin[d];
        hist[((size_t)(1 - r.parity) * B + b) * H + kk] = v;
        return;
    }
    float v = 0.f;
    if (col < r.m) {
        const long long n = r.n0 + col;
        const long long c = n * down + half;                        // tap index of j = 0
        // j from ceil((n*down - half)/up), not below 0 and (for a table that passed its check, never) not below the history's reach
        const long long jlo = max(max(0LL, r.P0 - H), cdiv(c - 2LL * half, up));
        const long long jhi = min(r.P0 + r.count - 1, c / up);
        int k = (int)(c - jlo * up);                                // in [0, 2*half] for jlo <= j <= jhi
        int d = (int)min(jlo - r.P0, (long long)r.count);           // >= -H; the upper clamp only keeps the cast exact
        const int dhi = (int)max(jhi - r.P0, -(long long)H - 1);    // <= count - 1; the lower clamp only keeps the cast exact
        double acc = 0;
        for (; d <= dhi; ++d, k -= up) {
            const float s = d >= 0 ? xr[d] : hin[d];
            acc += (double)s * (double)(LDS ? hs[skew(k)] : taps[k]);
        }
        v = (float)((double)up * acc);
    }
    y[(size_t)b * ldy + col] = v;
}

int gcd_of(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// a reduced ratio within the tap limit -> half = 10 max(up, down); 0 otherwise
int half_of(int up, int down) {
    if (up <= 0 || down <= 0 || gcd_of(up, down) != 1) return 0;
    const int m = up > down ? up : down;
    return m > SR_MAXM ? 0 : 10 * m;
}

int launch(float* hist, int H, const float* x, long long ldx, int n_x, const long long* rows, SrRow lock, int B, int up, int down,
           int half, const float* taps, int taps_mode, float* y, long long ldy, int ycols, int W, hipStream_t st) {
    const long long total = (long long)B * W;
    if (total <= 0) return IDV_OK;
    if (total > SR_MAX_GRID) return IDV_EINVAL;
    const dim3 grid((unsigned)((total + 255) / 256));
    const bool lds = taps_mode == IDV_SR_TAPS_AUTO ? up == 1 : taps_mode == IDV_SR_TAPS_LDS;
    if (lds)
        hipLaunchKernelGGL(stream_resample_kernel<true>, grid, dim3(256), ((size_t)skew(2 * half) + 1) * sizeof(float), st, hist, H, x, ldx,
                           n_x, rows, lock, B, up, down, half, taps, y, ldy, ycols, W);
    else
        hipLaunchKernelGGL(stream_resample_kernel<false>, grid, dim3(256), 0, st, hist, H, x, ldx, n_x, rows, lock, B, up, down, half, taps,
                           y, ldy, ycols, W);
    return idv_launch_status();
}

}  // namespace

extern "C" int idv_stream_resample_hist(int up, int down) {
    const int half = half_of(up, down);
    return half ? 2 * half / up + 1 : IDV_EINVAL;
}

extern "C" long long idv_stream_resample_final(long long P, int up, int down) {
    const int half = half_of(up, down);
    if (!half || P < 0 || P > SR_MAX_POS) return IDV_EINVAL;
    return n_final_of(P, up, down, half);
}

extern "C" int idv_stream_resample_row_fields(void) { return IDV_SR_ROW_FIELDS; }

extern "C" int idv_stream_resample(float* hist, int H, int parity, const float* x, long long ldx, int n_new, long long P0, int flush,
                                   long long n0, int m, int B, int up, int down, const float* taps, int taps_mode, float* y,
                                   long long ldy, void* stream) {
    const int half = half_of(up, down);
    if (!half || !hist || !taps || H != 2 * half / up + 1 || (parity != 0 && parity != 1) || n_new < 0 || n_new > ROWS_MAX_LEN ||
        (n_new > 0 && (!x || ldx < n_new)) || P0 < 0 || P0 > SR_MAX_POS || (flush != 0 && flush != 1) || B < 1 || B > ROWS_MAX_ROWS ||
        m < 0 || ldy < m || (m > 0 && !y) || taps_mode < IDV_SR_TAPS_AUTO || taps_mode > IDV_SR_TAPS_LDS)
        return IDV_EINVAL;
    // the output range is the host's to know (it sizes y) and this entry's to hold to the definition: nothing else bounds the reads
    const long long P1 = P0 + n_new;
    if (n0 != n_final_of(P0, up, down, half) || n0 + m != (flush ? n_out_of(P1, up, down) : n_final_of(P1, up, down, half)))
        return IDV_EINVAL;
    const int update = !flush && n_new > 0;
    const SrRow lock{P0, n0, n_new, m, parity, update};
    return launch(hist, H, x, ldx, n_new, nullptr, lock, B, up, down, half, taps, taps_mode, y, ldy, m, m + (update ? H : 0),
                  (hipStream_t)stream);
}

extern "C" int idv_stream_resample_rows_check(const long long* host_rows, int B, int n_x, int up, int down, int H, long long ldy) {
    const int half = half_of(up, down);
    if (!half || !host_rows || B < 1 || B > ROWS_MAX_ROWS || n_x < 0 || n_x > ROWS_MAX_LEN || H != 2 * half / up + 1 || ldy < 0)
        return IDV_EINVAL;
    for (int b = 0; b < B; ++b) {
        const long long* r = host_rows + (size_t)b * IDV_SR_ROW_FIELDS;
        const long long P0 = r[IDV_SR_ROW_P0], count = r[IDV_SR_ROW_COUNT], n0 = r[IDV_SR_ROW_N0], m = r[IDV_SR_ROW_M],
                        parity = r[IDV_SR_ROW_PARITY], end = r[IDV_SR_ROW_END], idle = r[IDV_SR_ROW_IDLE];
        if (P0 < 0 || P0 > SR_MAX_POS || count < 0 || count > n_x || m < 0 || m > ldy || (parity != 0 && parity != 1) ||
            (end != 0 && end != 1) || (idle != 0 && idle != 1))
            return IDV_EINVAL;
        if (idle != (count == 0 && !end)) return IDV_EINVAL;       // idle: no samples and no end; nothing of the slot's state moves
        const long long P1 = P0 + count;
        if (n0 != n_final_of(P0, up, down, half) || n0 + m != (end ? n_out_of(P1, up, down) : n_final_of(P1, up, down, half)))
            return IDV_EINVAL;
    }
    return IDV_OK;
}

extern "C" int idv_stream_resample_rows(float* hist, int H, const float* x, long long ldx, int n_x, const long long* rows, int B, int up,
                                        int down, const float* taps, int taps_mode, float* y, long long ldy, void* stream) {
    const int half = half_of(up, down);
    if (!half || !hist || !taps || H != 2 * half / up + 1 || n_x < 0 || n_x > ROWS_MAX_LEN || (n_x > 0 && (!x || ldx < n_x)) || !rows ||
        B < 1 || B > ROWS_MAX_ROWS || ldy < 0 || ldy > 2147483647LL - H || (ldy > 0 && !y) || taps_mode < IDV_SR_TAPS_AUTO ||
        taps_mode > IDV_SR_TAPS_LDS)
        return IDV_EINVAL;
    return launch(hist, H, x, ldx, n_x, rows, SrRow{}, B, up, down, half, taps, taps_mode, y, ldy, (int)ldy, (int)ldy + H,
                  (hipStream_t)stream);
}
