// DNSMOS P.808 (the P808_MOS column of the blind-set script) on the device: the librosa mel front end of model_v8.onnx, the head of
// that network and the per-clip mean (dnsmos.py P808).  The convolutions are those of dnsmos.hip.
//
//   mel power   a = the first 144000 samples of a segment (sample j of it is x[row][(start + j) mod lengths[row]]: the clip the script
//               tiles is never built, nothing at or past a row's length is read).  Frame t of 900 is a[160 t - 160 .. 160 t + 160],
//               zero outside [0, 144000) (the centred STFT with n_fft = 321 and constant padding).  re / im [t][k] = frame x the two
//               windowed DFT tables [161][324] (double, made on the host, k padded with zeros), p = re re + im im, S [t][m] = sum_k
//               mel[m][k] p[t][k]: both products on v_mfma_f64_16x16x4_f64, everything in double.  A float32 DFT moves the feature by
//               4e-5 in the bins 60 - 80 dB below the segment's maximum that top_db keeps alive; the double one by 1e-10.
//   dB          (10 log10(max(1e-10, S)) - 10 log10(max(1e-10, max S)), clamped at -80, + 40) / 40 in double, rounded once.
//   head, clip  dense 64 -> 64 ReLU -> 64 ReLU -> 1; the clip's value is the double mean of its segments in order.
//
// A workgroup of four waves owns 16 frames of one segment.  It stages the 16 x 321 frame samples in LDS as float ([frame][325]: the
// zeros of the definition are put in here), and wave w forms the 16 x 16 tiles of bins 16 (w + 4 q) .. + 15: the A operand is a frame
// sample converted to double at the LDS read, the B operand one double of the table read from global memory (each lane walks its own
// table row; the 0.8 MB of both tables stay in L2).  re and im share the A operand.  The power tile goes to LDS as double
// [frame][bin, 177], bins 161 .. 175 as zeros, and after one barrier wave w forms the mel tiles 16 (w + 4 q) of S the same way.
// Every sum runs over k in ascending steps of 4 inside one accumulator: an element's bits follow from its own segment and indices,
// never from the batch or the chunking.  The maximum is taken per workgroup and folded by a second kernel; no atomics.
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int P8_T = 900, P8_HOP = 160, P8_NFFT = 321, P8_KP = 324, P8_BINS = 161, P8_MELS = 120;
constexpr int P8_A = 144000;                        // samples of a segment the feature reads
constexpr int P8_FT = (P8_T + 15) / 16;             // 57 frame tiles
constexpr int P8_BT = (P8_BINS + 15) / 16;          // 11 bin tiles
constexpr int P8_MT = (P8_MELS + 15) / 16;          // 8 mel tiles
constexpr int P8_XP = 325;                          // floats per staged frame
constexpr int P8_PP = P8_BT * 16 + 1;               // doubles per power row
constexpr int P8_MK = 164;                          // 161 bins in steps of 4

__global__ __launch_bounds__(256) void p808_mel_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lengths, int B,
                                                       const int* __restrict__ seg, int nseg, const double* __restrict__ dft,
                                                       const double* __restrict__ mel, double* __restrict__ S,
                                                       double* __restrict__ part) {
    __shared__ float xs[16 * P8_XP];
    __shared__ double pw[16 * P8_PP];
    __shared__ double wmax[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int s = blockIdx.x / P8_FT, ft = blockIdx.x % P8_FT;
    const int row = seg[2 * s], start = seg[2 * s + 1];
    const bool rowok = (unsigned)row < (unsigned)B;
    const long long L = rowok ? lengths[row] : 0;
    const bool live = rowok && L > 0 && start >= 0;
    const float* xr = x + (size_t)(rowok ? row : 0) * ldx;

    for (int idx = tid; idx < 16 * P8_KP; idx += 256) {
        const int fr = idx / P8_KP, n = idx % P8_KP;
        const int t = ft * 16 + fr;
        const int j = P8_HOP * t - P8_HOP + n;
        float v = 0.f;
        if (live && t < P8_T && n < P8_NFFT && j >= 0 && j < P8_A) v = xr[((long long)start + j) % L];
        xs[fr * P8_XP + n] = v;
    }
    __syncthreads();

    // D[frame = lk + 4 reg][bin = li];  A[frame = li][k = 4 step + lk];  B[k = 4 step + lk][bin = li]
    const float* pa = xs + li * P8_XP + lk;
    for (int bt = wave; bt < P8_BT; bt += 4) {
        const int bin = bt * 16 + li;
        const bool bok = bin < P8_BINS;
        const double* pc = dft + (size_t)(bok ? bin : 0) * P8_KP + lk;
        const double* ps = pc + (size_t)P8_BINS * P8_KP;
        f64x4 ar = {0., 0., 0., 0.}, ai = {0., 0., 0., 0.};
#pragma unroll 3
        for (int k = 0; k < P8_KP; k += 4) {
            const double va = (double)pa[k];
            const double vc = bok ? pc[k] : 0.0, vs = bok ? ps[k] : 0.0;
            ar = __builtin_amdgcn_mfma_f64_16x16x4f64(va, vc, ar, 0, 0, 0);
            ai = __builtin_amdgcn_mfma_f64_16x16x4f64(va, vs, ai, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            pw[(lk + 4 * reg) * P8_PP + bin] = __dadd_rn(__dmul_rn(ar[reg], ar[reg]), __dmul_rn(ai[reg], ai[reg]));
    }
    __syncthreads();

    // D[frame = lk + 4 reg][mel = li];  A[frame = li][bin = 4 step + lk];  B[bin = 4 step + lk][mel = li]
    double m = -INFINITY;
    const double* qa = pw + li * P8_PP + lk;
    for (int mt = wave; mt < P8_MT; mt += 4) {
        const int mm = mt * 16 + li;
        const bool mok = mm < P8_MELS;
        const double* pb = mel + (size_t)(mok ? mm : 0) * P8_BINS;
        f64x4 acc = {0., 0., 0., 0.};
#pragma unroll 4
        for (int k = 0; k < P8_MK; k += 4) {
            const int kb = k + lk;
            const double vb = (mok && kb < P8_BINS) ? pb[kb] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[k], vb, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int t = ft * 16 + lk + 4 * reg;
            if (mok && t < P8_T) {
                S[((size_t)s * P8_T + t) * P8_MELS + mm] = acc[reg];
                m = fmax(m, acc[reg]);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    if (tid == 0) part[(size_t)s * P8_FT + ft] = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
}

__global__ void p808_max_kernel(const double* __restrict__ part, int nseg, double* __restrict__ smax) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    double m = part[(size_t)s * P8_FT];
    for (int k = 1; k < P8_FT; ++k) m = fmax(m, part[(size_t)s * P8_FT + k]);
    smax[s] = m;
}

// S [nseg][per] (double), smax [nseg] -> feat [nseg][per] (float).  max(ls) is ls at the maximum element, which is x - x = 0.
__global__ void p808_db_kernel(const double* __restrict__ S, const double* __restrict__ smax, long long per, long long n,
                               float* __restrict__ feat) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const double ref = __dmul_rn(10.0, log10(fmax(1e-10, smax[e / per])));
        double ls = __dsub_rn(__dmul_rn(10.0, log10(fmax(1e-10, S[e]))), ref);
        ls = fmax(ls, -80.0);
        feat[e] = (float)__ddiv_rn(__dadd_rn(ls, 40.0), 40.0);
    }
}

// g [N][64] -> raw [N]: dense 64 -> 64 ReLU, 64 -> 64 ReLU, 64 -> 1; weights [in][out]; k-ascending fmaf chains, then the bias
__global__ __launch_bounds__(64) void p808_head_kernel(const float* __restrict__ g, const float* __restrict__ w0, const float* __restrict__ b0,
                                                       const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ raw) {
    __shared__ float v0[64], v1[64], v2[64];
    const int n = blockIdx.x, j = threadIdx.x;
    v0[j] = g[(size_t)n * 64 + j];
    __syncthreads();
    {
        float acc = 0.f;
        for (int k = 0; k < 64; ++k) acc = fmaf(v0[k], w0[k * 64 + j], acc);
        v1[j] = fmaxf(acc + b0[j], 0.f);
    }
    __syncthreads();
    {
        float acc = 0.f;
        for (int k = 0; k < 64; ++k) acc = fmaf(v1[k], w1[k * 64 + j], acc);
        v2[j] = fmaxf(acc + b1[j], 0.f);
    }
    __syncthreads();
    if (j == 0) {
        float acc = 0.f;
        for (int k = 0; k < 64; ++k) acc = fmaf(v2[k], w2[k], acc);
        raw[n] = acc + b2[0];
    }
}

// raw [nseg], clip b = segments first[b] .. first[b] + count[b] - 1 -> out [B] = their mean; a double sum in segment order
__global__ void p808_clip_kernel(const float* __restrict__ raw, const int* __restrict__ first, const int* __restrict__ count, int B, int nseg,
                                 double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int f = first[b], c = count[b];
    double sum = 0.;
    for (int s = 0; s < c; ++s) {
        const int g = f + s;
        if ((unsigned)g < (unsigned)nseg) sum = __dadd_rn(sum, (double)raw[g]);
    }
    out[b] = sum / (double)c;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" long long idv_p808_mel_work_doubles(int nseg) { return nseg > 0 && nseg <= (1 << 20) ? (long long)nseg * P8_FT : -1; }

extern "C" int idv_p808_mel(const float* x, long long ldx, const int* lengths, int B, const int* seg, int nseg, const double* dft,
                            const double* mel, double* S, double* smax, double* work, void* stream) {
    if (!x || !lengths || !seg || !dft || !mel || !S || !smax || !work || B <= 0 || nseg <= 0 || nseg > (1 << 20) || ldx <= 0 ||
        !aligned(x, 4) || !aligned(lengths, 4) || !aligned(seg, 4) || !aligned(dft, 8) || !aligned(mel, 8) || !aligned(S, 8) ||
        !aligned(smax, 8) || !aligned(work, 8))
        return IDV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(p808_mel_kernel, dim3((unsigned)(nseg * P8_FT)), dim3(256), 0, st, x, ldx, lengths, B, seg, nseg, dft, mel, S, work);
    hipLaunchKernelGGL(p808_max_kernel, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, st, work, nseg, smax);
    return idv_launch_status();
}

extern "C" int idv_p808_db(const double* S, const double* smax, int nseg, long long per, float* feat, void* stream) {
    if (!S || !smax || !feat || nseg <= 0 || nseg > (1 << 20) || per <= 0 || per > (1LL << 31) || !aligned(S, 8) || !aligned(smax, 8) ||
        !aligned(feat, 4))
        return IDV_EINVAL;
    const long long n = (long long)nseg * per;
    long long g = (n + 255) / 256;
    g = g > 65536 ? 65536 : g;
    hipLaunchKernelGGL(p808_db_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, S, smax, per, n, feat);
    return idv_launch_status();
}

extern "C" int idv_p808_head(const float* g, int N, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                             const float* b2, float* raw, void* stream) {
    if (!g || !w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !raw || N <= 0 || !aligned(g, 4) || !aligned(w0, 4) || !aligned(b0, 4) ||
        !aligned(w1, 4) || !aligned(b1, 4) || !aligned(w2, 4) || !aligned(b2, 4) || !aligned(raw, 4))
        return IDV_EINVAL;
    hipLaunchKernelGGL(p808_head_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, g, w0, b0, w1, b1, w2, b2, raw);
    return idv_launch_status();
}

extern "C" int idv_p808_clip(const float* raw, int nseg, const int* first, const int* count, int B, double* out, void* stream) {
    if (!raw || !first || !count || !out || nseg <= 0 || B <= 0 || !aligned(raw, 4) || !aligned(first, 4) || !aligned(count, 4) ||
        !aligned(out, 8))
        return IDV_EINVAL;
    hipLaunchKernelGGL(p808_clip_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, (hipStream_t)stream, raw, first, count, B, nseg, out);
    return idv_launch_status();
}
