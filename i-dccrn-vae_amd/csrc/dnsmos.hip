// DNSMOS P.835 (SIG / BAK / OVRL) on the device: the network of sig_bak_ovr.onnx and the script around it (dnsmos.py).
//
//   front end   one launch gathers the segments out of the padded batch in place (sample (start + j) mod L of its row: the clip the
//               script tiles by appending it to itself is never materialised), forms the 900 frames of 320 samples and multiplies them
//               with the two learned [161, 320] matrices on v_mfma_f32_32x32x2_f32; the epilogue squares, clamps and takes the log.
//   conv3x3     a real 3x3 convolution (stride 1, zero pad 1, bias, ReLU) as an implicit GEMM on the fp32 matrix cores over NHWC
//               activations: M = pixels, N = Cout, K = 9 Cin in chunks of 32 input channels.  Optional 2x2 / 2 max-pool in the
//               epilogue, optional 1 -> C first layer computed on the vector ALU while the chunk is staged.
//   head        global max, three dense layers, the polynomials and the per-clip means.
//
// Every sum has a fixed order that follows from the element's own indices: k ascends chunk by chunk, tap by tap, channel pair by
// channel pair inside one accumulator; nothing depends on the batch around a segment; no atomics.
//
// conv3x3 tiling.  A workgroup of four waves owns CT_H x CT_W = 16 x 16 output pixels of one image and all Cout channels.  Per chunk
// it stages the 18 x 18 halo tile of 32 channels in LDS as [pixel][LSTRIDE = 33] (pixels outside the image are written as zeros: the
// padding exists only here), so a lane's A operand -- pixel lane & 31, channel 2 kk + (lane >> 5) -- is one ds_read_b32 without bank
// conflicts among the 32 pixels.  A wave owns four rows = two MFMA row tiles of 2 x 16 pixels.  Row i of a tile is the pixel
// (dy, dx) = ((i >> 1) & 1, ((i >> 2) << 1) | (i & 1)), so the four rows a lane holds in accumulator registers 4 g .. 4 g + 3 are one
// 2 x 2 pooling window: the max-pool is three v_max in the epilogue and the un-pooled map never exists.  The B operand (weights) is
// packed once per model as [co tile of 32][K / 2][64 lanes] and read straight from global memory, 256 coalesced bytes per wave and MFMA
// pair, one tap ahead of the MFMAs that use it; every wave of the card reads the same few hundred KB, which stay in L2.  The next
// chunk's halo tile is loaded into registers before the MFMAs of the current one are issued.
#include "common.hpp"

namespace {

constexpr int CT_H = 16, CT_W = 16;            // output pixels per workgroup (the tests name these)
constexpr int CCH = 32;                        // input channels per K chunk
constexpr int HALO_W = CT_W + 2, HALO_H = CT_H + 2, HALO = HALO_W * HALO_H;
constexpr int LSTRIDE = CCH + 1;
constexpr int FH_W = CT_W + 4, FH_H = CT_H + 4, FHALO = FH_W * FH_H;   // feature halo of the fused first layer
constexpr int CTHREADS = 256;
constexpr int NQ = HALO * (CCH / 4);           // float4 loads per chunk
constexpr int NPRE = (NQ + CTHREADS - 1) / CTHREADS;

struct ConvArgs {
    const float* x;      // [N][H][W][Cin], or the feature [N][H][W] when fused
    const float* wp;     // packed weights
    const float* bias;   // [Cout]
    const float* w1;     // fused first layer: [Cin][9]
    const float* b1;     // [Cin]
    float* y;
    int N, H, W, Cin, Cout, tiles_x, tiles_y;
};

// the 1 -> C first layer's value: one fmaf chain over the taps ky * 3 + kx in ascending order, then the bias, then ReLU
__device__ __forceinline__ float c1_value(const float (&w)[9], float b, const float (&f)[9]) {
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc = fmaf(w[t], f[t], acc);
    return fmaxf(acc + b, 0.f);
}

template <int NCO, bool POOL, bool FUSE1>
__global__ __launch_bounds__(CTHREADS) void conv3x3_kernel(const ConvArgs a) {
    __shared__ float tile[HALO * LSTRIDE];
    __shared__ float feat[FUSE1 ? FHALO : 1];

    const int bid = blockIdx.x;
    const int tx = bid % a.tiles_x;
    const int rest = bid / a.tiles_x;
    const int ty = rest % a.tiles_y;
    const int n = rest / a.tiles_y;
    const int x0 = tx * CT_W, y0 = ty * CT_H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hk = lane >> 5, i = lane & 31;
    const int H = a.H, W = a.W, Cin = a.Cin;
    const size_t img = (size_t)n * H * W;

    int abase[2];
    {
        const int dx = ((i >> 2) << 1) | (i & 1), dy = (i >> 1) & 1;
#pragma unroll
        for (int t = 0; t < 2; ++t) abase[t] = ((wave * 4 + t * 2 + dy) * HALO_W + dx) * LSTRIDE + hk;
    }

    f32x16 acc[2][NCO];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < NCO; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][c][e] = 0.f;

    if (FUSE1) {
        for (int idx = tid; idx < FHALO; idx += CTHREADS) {
            const int fy = y0 - 2 + idx / FH_W, fx = x0 - 2 + idx % FH_W;
            feat[idx] = ((unsigned)fy < (unsigned)H && (unsigned)fx < (unsigned)W) ? a.x[img * 1 + (size_t)fy * W + fx] : 0.f;
        }
    }

    f32x4 pre[NPRE];
    auto gload = [&](int c) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int idx = tid + j * CTHREADS;
            const int pix = idx >> 3, q = idx & 7;
            const int gy = y0 - 1 + pix / HALO_W, gx = x0 - 1 + pix % HALO_W;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (idx < NQ && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
                v = *reinterpret_cast<const f32x4*>(a.x + (img + (size_t)gy * W + gx) * Cin + c * CCH + q * 4);
            pre[j] = v;
        }
    };
    if (!FUSE1) gload(0);

    const int nchunk = Cin / CCH;
    const size_t khalf = (size_t)Cin * 9 / 2;
    // the B operands of one tap (16 k pairs x NCO column tiles), loaded one tap ahead of the MFMAs that use them: the loads of tap
    // g + 1 are in flight while tap g computes, and those of a chunk's first tap while the chunk is staged
    constexpr int NW = (CCH / 2) * NCO;
    const int ntap = nchunk * 9;
    float wnext[NW];
    auto wload = [&](int g) {
        const float* wt = a.wp + (size_t)min(g, ntap - 1) * (CCH / 2) * 64 + lane;
#pragma unroll
        for (int co = 0; co < NCO; ++co)
#pragma unroll
            for (int kk = 0; kk < CCH / 2; ++kk) wnext[co * (CCH / 2) + kk] = wt[(co * khalf + kk) * 64];
    };
    wload(0);
    for (int c = 0; c < nchunk; ++c) {
        if (c > 0 || FUSE1) __syncthreads();          // the previous chunk's reads are done / the feature halo is in place
        if (FUSE1) {
            const int cl = tid & 31, ci = c * CCH + cl;
            float w[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) w[t] = a.w1[ci * 9 + t];
            const float b = a.b1[ci];
            for (int pix = tid >> 5; pix < HALO; pix += CTHREADS / 32) {
                const int py = pix / HALO_W, px = pix % HALO_W;
                const int gy = y0 - 1 + py, gx = x0 - 1 + px;
                float v = 0.f;
                if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
                    float f[9];
#pragma unroll
                    for (int t = 0; t < 9; ++t) f[t] = feat[(py + t / 3) * FH_W + px + t % 3];
                    v = c1_value(w, b, f);
                }
                tile[pix * LSTRIDE + cl] = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NPRE; ++j) {
                const int idx = tid + j * CTHREADS;
                if (idx < NQ) {
                    float* d = tile + (idx >> 3) * LSTRIDE + (idx & 7) * 4;
                    d[0] = pre[j][0]; d[1] = pre[j][1]; d[2] = pre[j][2]; d[3] = pre[j][3];
                }
            }
        }
        __syncthreads();
        if (!FUSE1 && c + 1 < nchunk) gload(c + 1);

#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll 1
            for (int kx = 0; kx < 3; ++kx) {
                const int toff = (ky * HALO_W + kx) * LSTRIDE;
                const float* a0 = tile + abase[0] + toff;
                const float* a1 = tile + abase[1] + toff;
                float wcur[NW];
#pragma unroll
                for (int q = 0; q < NW; ++q) wcur[q] = wnext[q];
                wload(c * 9 + ky * 3 + kx + 1);
#pragma unroll
                for (int kk = 0; kk < CCH / 2; ++kk) {
                    const float va0 = a0[2 * kk], va1 = a1[2 * kk];
#pragma unroll
                    for (int co = 0; co < NCO; ++co) {
                        const float vb = wcur[co * (CCH / 2) + kk];
                        acc[0][co] = __builtin_amdgcn_mfma_f32_32x32x2f32(va0, vb, acc[0][co], 0, 0, 0);
                        acc[1][co] = __builtin_amdgcn_mfma_f32_32x32x2f32(va1, vb, acc[1][co], 0, 0, 0);
                    }
                }
            }
        }
    }

    // D: column (output channel) = lane & 31, row (pixel of the tile) m = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    const int Cout = a.Cout;
#pragma unroll
    for (int co = 0; co < NCO; ++co) {
        const int ch = co * 32 + i;
        const float b = a.bias[ch];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int yb = y0 + wave * 4 + t * 2;
            if (POOL) {
                const int Ho = H >> 1, Wo = W >> 1, py = yb >> 1;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int px = (x0 >> 1) + hk + 2 * g;
                    const float v = fmaxf(fmaxf(acc[t][co][4 * g], acc[t][co][4 * g + 1]), fmaxf(acc[t][co][4 * g + 2], acc[t][co][4 * g + 3]));
                    if (py < Ho && px < Wo) a.y[(((size_t)n * Ho + py) * Wo + px) * Cout + ch] = fmaxf(v + b, 0.f);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = (e & 3) + 8 * (e >> 2) + 4 * hk;
                    const int yy = yb + ((m >> 1) & 1), xx = x0 + (((m >> 2) << 1) | (m & 1));
                    if (yy < H && xx < W) a.y[((img + (size_t)yy * W + xx)) * Cout + ch] = fmaxf(acc[t][co][e] + b, 0.f);
                }
            }
        }
    }
}

// w [Cout][Cin][3][3] -> [co tile][K / 2][64]: lane l holds B[k = 2 kp + (l >> 5)][co = 32 tile + (l & 31)], k = (chunk * 9 + tap) * 32 + ci % 32
__global__ void conv3x3_pack_kernel(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ p) {
    const long long n = (long long)Cin * 9 * Cout;
    const long long khalf = (long long)Cin * 9 / 2;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(e & 63);
        const long long kp = (e >> 6) % khalf;
        const int tile = (int)((e >> 6) / khalf);
        const int k = (int)(2 * kp + (lane >> 5));
        const int chunk = k / (9 * CCH), r = k % (9 * CCH);
        const int tap = r / CCH, ci = chunk * CCH + r % CCH;
        const int co = tile * 32 + (lane & 31);
        p[e] = w[((size_t)co * Cin + ci) * 9 + tap];
    }
}

// the first layer alone: f [N][H][W] -> y [N][H][W][C]
__global__ void conv3x3_c1_kernel(const float* __restrict__ f, const float* __restrict__ w1, const float* __restrict__ b1, int N, int H, int W,
                                  int C, float* __restrict__ y) {
    const long long n = (long long)N * H * W * C;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long long pix = e / C;
        const int xx = (int)(pix % W);
        const int yy = (int)((pix / W) % H);
        const long long im = pix / ((long long)W * H);
        float w[9], v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            w[t] = w1[c * 9 + t];
            const int fy = yy - 1 + t / 3, fx = xx - 1 + t % 3;
            v[t] = ((unsigned)fy < (unsigned)H && (unsigned)fx < (unsigned)W) ? f[(im * H + fy) * W + fx] : 0.f;
        }
        y[e] = c1_value(w, b1[c], v);
    }
}

// the first layer with the 2x2 / 2 floor max-pool behind it: f [N][H][W] -> y [N][H / 2][W / 2][C].  One thread per output reads the
// 4 x 4 feature patch under its pooling window once and takes the maximum of the four c1_value: the bits of the pool of
// conv3x3_c1_kernel's map, which is never written
__global__ void conv3x3_c1_pool_kernel(const float* __restrict__ f, const float* __restrict__ w1, const float* __restrict__ b1, int N, int H,
                                       int W, int C, float* __restrict__ y) {
    const int Ho = H >> 1, Wo = W >> 1;
    const long long n = (long long)N * Ho * Wo * C;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long long pix = e / C;
        const int px = (int)(pix % Wo);
        const int py = (int)((pix / Wo) % Ho);
        const long long im = pix / ((long long)Wo * Ho);
        float w[9], patch[16];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = w1[c * 9 + t];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int fy = 2 * py - 1 + q / 4, fx = 2 * px - 1 + q % 4;
            patch[q] = ((unsigned)fy < (unsigned)H && (unsigned)fx < (unsigned)W) ? f[(im * H + fy) * W + fx] : 0.f;
        }
        const float b = b1[c];
        float m = 0.f;                               // every c1_value is >= 0 (ReLU)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t] = patch[(d / 2 + t / 3) * 4 + d % 2 + t % 3];
            m = fmaxf(m, c1_value(w, b, v));
        }
        y[e] = m;
    }
}

// x [N][P][C] -> out [N][C] = max over the P pixels (exact: a maximum has no order)
__global__ __launch_bounds__(256) void gmax_kernel(const float* __restrict__ x, long long P, int C, float* __restrict__ out) {
    __shared__ float part[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int c = tid % C, s = tid / C, ns = 256 / C;
    float m = -INFINITY;
    for (long long p = s; p < P; p += ns) m = fmaxf(m, x[((size_t)n * P + p) * C + c]);
    part[tid] = m;
    __syncthreads();
    if (tid < C) {
        for (int k = 1; k < ns; ++k) m = fmaxf(m, part[k * C + tid]);
        out[(size_t)n * C + tid] = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------- front end
constexpr int FE_T = 900, FE_HOP = 160, FE_WIN = 320, FE_BINS = 161;
constexpr int FE_FT = (FE_T + 31) / 32, FE_BT = (FE_BINS + 31) / 32;
constexpr int FE_UNITS = FE_FT * FE_BT;

// re / im [161][320] -> [bin tile][k pair][re, im][64]: lane l holds B[k = 2 kp + (l >> 5)][bin = 32 tile + (l & 31)], zero past bin 160
__global__ void fe_pack_kernel(const float* __restrict__ re, const float* __restrict__ im, float* __restrict__ p) {
    const int n = FE_BT * (FE_WIN / 2) * 2 * 64;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int lane = e & 63, part = (e >> 6) & 1, kp = (e >> 7) % (FE_WIN / 2), bt = (e >> 7) / (FE_WIN / 2);
        const int bin = bt * 32 + (lane & 31), k = 2 * kp + (lane >> 5);
        p[e] = bin < FE_BINS ? (part ? im : re)[bin * FE_WIN + k] : 0.f;
    }
}

// one wave per (segment, tile of 32 frames, tile of 32 bins); no LDS, no barrier
__global__ __launch_bounds__(256) void fe_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lengths, int B,
                                                 const int* __restrict__ seg, int nseg, const float* __restrict__ mats, float floor_p,
                                                 float ln_div, float* __restrict__ feat) {
    const int lane = threadIdx.x & 63, hk = lane >> 5, i = lane & 31;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= (long long)nseg * FE_UNITS) return;
    const int s = (int)(u / FE_UNITS), r = (int)(u % FE_UNITS);
    const int ft = r / FE_BT, bt = r % FE_BT;
    const int row = seg[2 * s], start = seg[2 * s + 1];
    const bool rowok = (unsigned)row < (unsigned)B;
    const long long L = rowok ? lengths[row] : 0;
    const int t = ft * 32 + i;
    const bool live = rowok && L > 0 && start >= 0 && t < FE_T;
    const float* xr = x + (size_t)(rowok ? row : 0) * ldx;
    long long pos = live ? ((long long)start + (long long)FE_HOP * t + hk) % L : 0;

    f32x16 ar, ai;
#pragma unroll
    for (int e = 0; e < 16; ++e) ar[e] = ai[e] = 0.f;
    const float* m = mats + (size_t)bt * (FE_WIN / 2) * 128 + lane;
#pragma unroll 4
    for (int kp = 0; kp < FE_WIN / 2; ++kp) {
        const float va = live ? xr[pos] : 0.f;
        const float br = m[kp * 128], bi = m[kp * 128 + 64];
        ar = __builtin_amdgcn_mfma_f32_32x32x2f32(va, br, ar, 0, 0, 0);
        ai = __builtin_amdgcn_mfma_f32_32x32x2f32(va, bi, ai, 0, 0, 0);
        pos += 2;
        if (pos >= L && live) pos %= L;
    }
    const int bin = bt * 32 + i;
    if (bin >= FE_BINS) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int tt = ft * 32 + (e & 3) + 8 * (e >> 2) + 4 * hk;
        if (tt >= FE_T) continue;
        const float p = __fadd_rn(__fmul_rn(ar[e], ar[e]), __fmul_rn(ai[e], ai[e]));
        const float sq = __fsqrt_rn(p);
        const float q = fmaxf(floor_p, __fmul_rn(sq, sq));
        feat[((size_t)s * FE_T + tt) * FE_BINS + bin] = (float)(log((double)q) / (double)ln_div);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- head
// g [N][64] -> raw [N][3]: dense 64 -> 128 ReLU, 128 -> 64 ReLU, 64 -> 3; weights [in][out]; k-ascending fmaf chains, then the bias
__global__ __launch_bounds__(128) void head_kernel(const float* __restrict__ g, const float* __restrict__ w0, const float* __restrict__ b0,
                                                   const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                   const float* __restrict__ b2, float* __restrict__ raw) {
    __shared__ float v0[64], v1[128], v2[64];
    const int n = blockIdx.x, j = threadIdx.x;
    if (j < 64) v0[j] = g[(size_t)n * 64 + j];
    __syncthreads();
    {
        float acc = 0.f;
        for (int k = 0; k < 64; ++k) acc = fmaf(v0[k], w0[k * 128 + j], acc);
        v1[j] = fmaxf(acc + b0[j], 0.f);
    }
    __syncthreads();
    if (j < 64) {
        float acc = 0.f;
        for (int k = 0; k < 128; ++k) acc = fmaf(v1[k], w1[k * 64 + j], acc);
        v2[j] = fmaxf(acc + b1[j], 0.f);
    }
    __syncthreads();
    if (j < 3) {
        float acc = 0.f;
        for (int k = 0; k < 64; ++k) acc = fmaf(v2[k], w2[k * 3 + j], acc);
        raw[(size_t)n * 3 + j] = acc + b2[j];
    }
}

// raw [nseg][3], clip b = segments first[b] .. first[b] + count[b] - 1 -> out [B][6] = means of the raw values, means of the polynomials
// (poly [3][4], highest power first, Horner in double without contraction); double sums in segment order
__global__ void clip_kernel(const float* __restrict__ raw, const int* __restrict__ first, const int* __restrict__ count, int B, int nseg,
                            const double* __restrict__ poly, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int f = first[b], c = count[b];
    double sr[3] = {0., 0., 0.}, sp[3] = {0., 0., 0.};
    for (int s = 0; s < c; ++s) {
        const int g = f + s;
        if ((unsigned)g >= (unsigned)nseg) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v = (double)raw[(size_t)g * 3 + j];
            double y = poly[j * 4];
#pragma unroll
            for (int d = 1; d < 4; ++d) y = __dadd_rn(__dmul_rn(y, v), poly[j * 4 + d]);
            sr[j] = __dadd_rn(sr[j], v);
            sp[j] = __dadd_rn(sp[j], y);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[(size_t)b * 6 + j] = sr[j] / (double)c;
        out[(size_t)b * 6 + 3 + j] = sp[j] / (double)c;
    }
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int grid_for(long long n, int threads) {
    long long g = (n + threads - 1) / threads;
    return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

bool conv_dims_ok(int N, int H, int W, int Cin, int Cout, int pool) {
    if (N <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768) return false;
    if (!(Cin == 32 || Cin == 64 || Cin == 128) || !(Cout == 32 || Cout == 64)) return false;
    if (pool && (H < 2 || W < 2)) return false;
    const long long tiles = (long long)((H + CT_H - 1) / CT_H) * ((W + CT_W - 1) / CT_W) * N;
    return tiles <= 0x7fffffffLL;
}

template <bool FUSE1>
int launch_conv(const ConvArgs& a, int pool, hipStream_t st) {
    const dim3 grid((unsigned)((long long)a.tiles_x * a.tiles_y * a.N)), block(CTHREADS);
    const int nco = a.Cout / 32;
    if (nco == 1 && !pool) hipLaunchKernelGGL((conv3x3_kernel<1, false, FUSE1>), grid, block, 0, st, a);
    else if (nco == 1) hipLaunchKernelGGL((conv3x3_kernel<1, true, FUSE1>), grid, block, 0, st, a);
    else if (!pool) hipLaunchKernelGGL((conv3x3_kernel<2, false, FUSE1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((conv3x3_kernel<2, true, FUSE1>), grid, block, 0, st, a);
    return idv_launch_status();
}

}  // namespace

extern "C" int idv_conv3x3_tile(int which) { return which == 0 ? CT_H : CT_W; }

extern "C" long long idv_conv3x3_wfloats(int Cin, int Cout) {
    if (!conv_dims_ok(1, 2, 2, Cin, Cout, 0)) return -1;
    return (long long)Cin * 9 * Cout;
}

extern "C" int idv_conv3x3_pack(const float* w, int Cin, int Cout, float* packed, void* stream) {
    if (!w || !packed || !conv_dims_ok(1, 2, 2, Cin, Cout, 0) || !aligned(w, 4) || !aligned(packed, 4)) return IDV_EINVAL;
    hipLaunchKernelGGL(conv3x3_pack_kernel, dim3(grid_for((long long)Cin * 9 * Cout, 256)), dim3(256), 0, (hipStream_t)stream, w, Cin, Cout,
                       packed);
    return idv_launch_status();
}

extern "C" int idv_conv3x3_fwd(const float* x, const float* wp, const float* bias, int N, int H, int W, int Cin, int Cout, int pool,
                               float* y, void* stream) {
    if (!x || !wp || !bias || !y || !conv_dims_ok(N, H, W, Cin, Cout, pool) || !aligned(x, 16) || !aligned(wp, 4) || !aligned(bias, 4) ||
        !aligned(y, 4))
        return IDV_EINVAL;
    ConvArgs a{x, wp, bias, nullptr, nullptr, y, N, H, W, Cin, Cout, (W + CT_W - 1) / CT_W, (H + CT_H - 1) / CT_H};
    return launch_conv<false>(a, pool ? 1 : 0, (hipStream_t)stream);
}

extern "C" int idv_conv3x3_c1_fwd(const float* f, const float* w1, const float* b1, int N, int H, int W, int C, float* y, void* stream) {
    if (!f || !w1 || !b1 || !y || N <= 0 || H <= 0 || W <= 0 || H > 32768 || W > 32768 || C <= 0 || C > 1024 || !aligned(f, 4) ||
        !aligned(w1, 4) || !aligned(b1, 4) || !aligned(y, 4))
        return IDV_EINVAL;
    hipLaunchKernelGGL(conv3x3_c1_kernel, dim3(grid_for((long long)N * H * W * C, 256)), dim3(256), 0, (hipStream_t)stream, f, w1, b1, N, H, W,
                       C, y);
    return idv_launch_status();
}

extern "C" int idv_conv3x3_c1_pool_fwd(const float* f, const float* w1, const float* b1, int N, int H, int W, int C, float* y, void* stream) {
    if (!f || !w1 || !b1 || !y || N <= 0 || H < 2 || W < 2 || H > 32768 || W > 32768 || C <= 0 || C > 1024 || !aligned(f, 4) ||
        !aligned(w1, 4) || !aligned(b1, 4) || !aligned(y, 4))
        return IDV_EINVAL;
    hipLaunchKernelGGL(conv3x3_c1_pool_kernel, dim3(grid_for((long long)N * (H / 2) * (W / 2) * C, 256)), dim3(256), 0, (hipStream_t)stream, f,
                       w1, b1, N, H, W, C, y);
    return idv_launch_status();
}

extern "C" int idv_conv3x3_c1_fused_fwd(const float* f, const float* w1, const float* b1, int C1, const float* wp, const float* bias, int N,
                                        int H, int W, int Cout, int pool, float* y, void* stream) {
    if (!f || !w1 || !b1 || !wp || !bias || !y || !conv_dims_ok(N, H, W, C1, Cout, pool) || !aligned(f, 4) || !aligned(w1, 4) ||
        !aligned(b1, 4) || !aligned(wp, 4) || !aligned(bias, 4) || !aligned(y, 4))
        return IDV_EINVAL;
    ConvArgs a{f, wp, bias, w1, b1, y, N, H, W, C1, Cout, (W + CT_W - 1) / CT_W, (H + CT_H - 1) / CT_H};
    return launch_conv<true>(a, pool ? 1 : 0, (hipStream_t)stream);
}

extern "C" int idv_conv3x3_gmax(const float* x, int N, long long P, int C, float* out, void* stream) {
    if (!x || !out || N <= 0 || N > 0x7fffffff || P <= 0 || P > (1LL << 31) || C <= 0 || C > 256 || 256 % C != 0 || !aligned(x, 4) ||
        !aligned(out, 4))
        return IDV_EINVAL;
    hipLaunchKernelGGL(gmax_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, x, P, C, out);
    return idv_launch_status();
}

extern "C" long long idv_dnsmos_frontend_wfloats(void) { return (long long)FE_BT * (FE_WIN / 2) * 2 * 64; }

extern "C" int idv_dnsmos_frontend_pack(const float* re, const float* im, float* packed, void* stream) {
    if (!re || !im || !packed || !aligned(re, 4) || !aligned(im, 4) || !aligned(packed, 4)) return IDV_EINVAL;
    hipLaunchKernelGGL(fe_pack_kernel, dim3(grid_for(idv_dnsmos_frontend_wfloats(), 256)), dim3(256), 0, (hipStream_t)stream, re, im, packed);
    return idv_launch_status();
}

extern "C" int idv_dnsmos_frontend(const float* x, long long ldx, const int* lengths, int B, const int* seg, int nseg, const float* mats,
                                   float floor_p, float ln_div, float* feat, void* stream) {
    if (!x || !lengths || !seg || !mats || !feat || B <= 0 || nseg <= 0 || nseg > (1 << 20) || ldx <= 0 || !(floor_p > 0.f) ||
        !(ln_div > 0.f) || !aligned(x, 4) || !aligned(lengths, 4) || !aligned(seg, 4) || !aligned(mats, 4) || !aligned(feat, 4))
        return IDV_EINVAL;
    const long long units = (long long)nseg * FE_UNITS;
    hipLaunchKernelGGL(fe_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, lengths, B, seg, nseg, mats,
                       floor_p, ln_div, feat);
    return idv_launch_status();
}

extern "C" int idv_dnsmos_head(const float* g, int N, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                               const float* b2, float* raw, void* stream) {
    if (!g || !w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !raw || N <= 0 || !aligned(g, 4) || !aligned(w0, 4) || !aligned(b0, 4) ||
        !aligned(w1, 4) || !aligned(b1, 4) || !aligned(w2, 4) || !aligned(b2, 4) || !aligned(raw, 4))
        return IDV_EINVAL;
    hipLaunchKernelGGL(head_kernel, dim3((unsigned)N), dim3(128), 0, (hipStream_t)stream, g, w0, b0, w1, b1, w2, b2, raw);
    return idv_launch_status();
}

extern "C" int idv_dnsmos_clip(const float* raw, int nseg, const int* first, const int* count, int B, const double* poly, double* out,
                               void* stream) {
    if (!raw || !first || !count || !poly || !out || nseg <= 0 || B <= 0 || !aligned(raw, 4) || !aligned(first, 4) || !aligned(count, 4) ||
        !aligned(poly, 8) || !aligned(out, 8))
        return IDV_EINVAL;
    hipLaunchKernelGGL(clip_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, (hipStream_t)stream, raw, first, count, B, nseg, poly, out);
    return idv_launch_status();
}
