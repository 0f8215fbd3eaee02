// The streaming complex conv / transposed conv of stream_conv.hip in split-bf16 (bf16x3) arithmetic on the bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16): the same function, arguments, K parts, `work` layout, combine kernel and epilogue as the fp32 engines
// (stream_conv.hip, stream_conv_mfma.hip), with every product w x replaced by
//     w_lo x_hi + w_hi x_lo + w_hi x_hi          hi = the fp32 value with its low 16 bits cleared (a bf16 by truncation),
//                                                lo = round-to-nearest-even bf16 of the exact difference
// (tests/pw_ref.py split / split_model) and fp32 accumulation.  Sources, histories, outputs and `work` stay fp32: x is split in
// registers, the weights once by the pack kernel.  Not bit-identical to the fp32 engines; the dropped w_lo x_lo term is 2^-16
// relative.
//
// Operands: the 16 k of one MFMA are (4 input channels) x (2 time taps) x (re, im) of ONE frequency tap: lane half h = lane >> 5
// holds time tap h (0: x[t-1], 1: x[t]), element j = 2 c + ri of its fragment is channel 4 g + c, part ri.  One B fragment (xr, xi)
// serves both tiles, the real one with A = (wr, -wi) and the imaginary one with A = (wi, wr).  Per (group of 4 channels, kf): two
// B fragments (hi, lo), four pre-packed A fragments (16 bytes per lane each), six MFMAs in the order lo hi, hi lo, hi hi.
//
// What decides the arithmetic of an output position is a function of the layer shape and nsplit alone: channel ci sits in group
// ci / 4, slot ci % 4, whatever the K part; a part [ci0, ci1) walks the groups ci0 / 4 .. (ci1 - 1) / 4 in ascending order, kf
// inside a group (the parity's taps only when transposed), and the channels of a group outside the part, past Cin or at a frequency
// row outside the input enter as zero x operands (they are not skipped).  K parts go to `work` and the shared combine kernel adds
// them 0..nsplit-1.  B, k, the row table and the tiles per wave change none of it.
//
// Mapping: as stream_conv_mfma.hip.  The 32 columns of a tile are 32 consecutive positions q = fq * J + j (one output-bin parity,
// j = b * k + t); a lane reads the column of its time tap straight from the planar sources and the history (no LDS, no barrier); a
// wave owns NT = 1 or 2 tiles of the 32 output channels of its co tile, real and imaginary.  The operands of step s + 1 are loaded
// before the MFMAs of step s are issued.  NT is chosen from the launch size only.
#include "stream_conv.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BF_CO = 32;                       // output channels per workgroup: one real and one imaginary 32-row tile
constexpr int BF_WAVES = SC_THREADS / 64;
constexpr int BF_CG = 4;                        // input channels per MFMA
constexpr int BF_FRAG = 4 * 64;                 // u32x4 of one (group, kf): real hi, real lo, imaginary hi, imaginary lo, 64 lanes each

struct Pos {
    bool live;
    int fq, j, b, t;
};

__device__ __forceinline__ Pos pos_of(int q, int nq, int J, int k) {
    Pos p;
    p.live = q < nq;
    p.fq = p.live ? q / J : 0;
    p.j = p.live ? q - p.fq * J : 0;
    p.b = p.j / k;
    p.t = p.j - p.b * k;
    return p;
}

__device__ __forceinline__ float hi_of(float v) { return __uint_as_float(__float_as_uint(v) & 0xffff0000u); }

// (re, im) -> the word (bf16 re | bf16 im << 16) of the hi parts and of the lo parts
__device__ __forceinline__ void split2(float re, float im, unsigned& hi, unsigned& lo) {
    hi = (__float_as_uint(re) >> 16) | (__float_as_uint(im) & 0xffff0000u);
    const bf16x2 l = {(__bf16)(re - hi_of(re)), (__bf16)(im - hi_of(im))};
    lo = __builtin_bit_cast(unsigned, l);
}

// grid: x = blocks of BF_WAVES * NT * 32 positions, y = co tiles of 32, z = split * (transposed ? 2 : 1) + output-bin parity
template <int NT, bool ROWS>
__device__ __forceinline__ void cconv_bf16_body(const SconvArgs& a, const SconvRows& r) {
    const int J = a.B * a.k;
    const int par = a.transposed ? (int)(blockIdx.z & 1) : 0;
    const int split = a.transposed ? (int)(blockIdx.z >> 1) : (int)blockIdx.z;
    const int cot = blockIdx.y;
    const int Cin = a.C0 + a.C1;

    // last input column of x0 -> x0hist_out, as the vector-ALU kernel does it
    if (a.x0hist_out && blockIdx.y == 0 && blockIdx.z == 0) {
        const long long n = 2LL * a.C0 * a.Fin * a.B;
        for (long long e = blockIdx.x * (long long)SC_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * SC_THREADS) {
            const int b = (int)(e % a.B);
            const long long pf = e / a.B;                     // (ri * C0 + ci) * Fin + fi
            if (ROWS) {
                const RowOf rw = row_of(r, b);
                if (rw.k > 0) a.x0hist_out[(size_t)(1 - rw.parity) * r.h0_half + e] = a.x0[pf * a.Jp + (long long)b * a.Tp + rw.k];
            } else {
                a.x0hist_out[e] = a.x0[pf * a.Jp + (long long)b * a.Tp + a.k];
            }
        }
    }

    const int nfq = a.transposed ? (par == 0 ? a.Fin : a.Fin - 1) : a.Fout;
    const int nq = nfq * J;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, hk = lane >> 5;                // hk: the lane's time tap
    const int q0 = ((int)blockIdx.x * BF_WAVES + wave) * (NT * 32) + col;
    if (q0 - col >= nq) return;                               // the whole wave; the kernel has no barrier
    const int ci0 = split * a.cps, ci1 = min(Cin, ci0 + a.cps);
    const int nk = a.transposed ? (par == 0 ? 3 : 2) : 5;     // taps kf = par, par + 2, .. when transposed
    const int ngroup = (Cin + BF_CG - 1) / BF_CG;
    const u32x4* wt = reinterpret_cast<const u32x4*>(a.w) + (size_t)cot * ngroup * 5 * BF_FRAG + lane;

    f32x16 accr[NT], acci[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) accr[n][e] = acci[n][e] = 0.f;

    // per tile and source: the lane's column (of its time tap) in the re plane at input row fi0 (kf = 0), channel 0; rs: floats
    // from a row to the next (both sources), pl: from the re plane to the im plane
    const float* px[2][NT];
    long long pl[2][NT];
    int rs[NT], fi0[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const Pos p = pos_of(q0 + n * 32, nq, J, a.k);
        const int f0 = a.transposed ? p.fq + 1 : 2 * p.fq - 2;                 // fi = f0 + d, d = kf (conv) or -m (transposed)
        fi0[n] = p.live ? f0 : -0x40000000;
        const bool hist = hk == 0 && p.t == 0;                                 // x[t-1] of a stream's first frame
        rs[n] = hist ? a.B : a.Jp;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float* x = s ? a.x1 : a.x0;
            const float* hs = s ? a.h1 : a.h0;
            const int C = s ? a.C1 : a.C0;
            if (hist) {
                size_t half = 0;
                if (ROWS && p.live) half = (size_t)row_of(r, p.b).parity * (s ? r.h1_half : r.h0_half);
                px[s][n] = hs + half + (long long)f0 * a.B + p.b;
                pl[s][n] = (long long)C * a.Fin * a.B;
            } else {
                px[s][n] = x + (long long)f0 * a.Jp + (long long)p.b * a.Tp + p.t + hk;
                pl[s][n] = (long long)C * a.Fin * a.Jp;
            }
        }
    }

    struct Raw {
        u32x4 w[4];
        float x[NT][2 * BF_CG];
    };

    auto load = [&](int g, int m, Raw& f) {
        const int kf = a.transposed ? par + 2 * m : m;
        const int d = a.transposed ? -m : m;
        const u32x4* wk = wt + ((size_t)g * 5 + kf) * BF_FRAG;
#pragma unroll
        for (int e = 0; e < 4; ++e) f.w[e] = wk[64 * e];
#pragma unroll
        for (int c = 0; c < BF_CG; ++c) {
            const int ci = g * BF_CG + c;
            const bool in_part = ci >= ci0 && ci < ci1;
            const int s = ci >= a.C0 ? 1 : 0;
            const long long row = (long long)(s ? ci - a.C0 : ci) * a.Fin + d;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f.x[n][2 * c] = f.x[n][2 * c + 1] = 0.f;
                if (in_part && (unsigned)(fi0[n] + d) < (unsigned)a.Fin) {
                    const float* q = (s ? px[1][n] : px[0][n]) + row * rs[n];
                    f.x[n][2 * c] = q[0];
                    f.x[n][2 * c + 1] = q[s ? pl[1][n] : pl[0][n]];
                }
            }
        }
    };

    if (ci0 < ci1) {
        const int ge = (ci1 - 1) / BF_CG;
        Raw cur;
        int g = ci0 / BF_CG, m = 0;
        load(g, m, cur);
        for (;;) {
            int ng = g, nm = m + 1;
            if (nm == nk) { nm = 0; ++ng; }
            const bool more = ng <= ge;
            Raw nxt;
            load(more ? ng : g, more ? nm : m, nxt);
            const bf16x8 rh = __builtin_bit_cast(bf16x8, cur.w[0]), rl = __builtin_bit_cast(bf16x8, cur.w[1]);
            const bf16x8 ih = __builtin_bit_cast(bf16x8, cur.w[2]), il = __builtin_bit_cast(bf16x8, cur.w[3]);
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                u32x4 h, l;
#pragma unroll
                for (int c = 0; c < BF_CG; ++c) {
                    unsigned hw, lw;
                    split2(cur.x[n][2 * c], cur.x[n][2 * c + 1], hw, lw);
                    h[c] = hw; l[c] = lw;
                }
                const bf16x8 xh = __builtin_bit_cast(bf16x8, h), xl = __builtin_bit_cast(bf16x8, l);
                accr[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rl, xh, accr[n], 0, 0, 0);
                acci[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(il, xh, acci[n], 0, 0, 0);
                accr[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rh, xl, accr[n], 0, 0, 0);
                acci[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ih, xl, acci[n], 0, 0, 0);
                accr[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rh, xh, accr[n], 0, 0, 0);
                acci[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ih, xh, acci[n], 0, 0, 0);
            }
            if (!more) break;
            cur = nxt; g = ng; m = nm;
        }
    }

    // D: column = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); rows past Cout are the pack's zero padding
    const size_t slab = (size_t)a.Cout * a.Fout * J;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const Pos p = pos_of(q0 + n * 32, nq, J, a.k);
        if (!p.live) continue;
        const int fo = a.transposed ? 2 * p.fq + par : p.fq;
        RowOf rw{a.k, 0};
        if (ROWS) rw = row_of(r, p.b);
        float* hist = ROWS && a.hist_out ? a.hist_out + (size_t)(1 - rw.parity) * r.out_half : a.hist_out;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = cot * BF_CO + (e & 3) + 8 * (e >> 2) + 4 * hk;
            if (co >= a.Cout) continue;
            if (a.nsplit == 1) {
                epilogue(a, co, fo, p.b, p.t, accr[n][e], acci[n][e], hist, rw.k - 1);
            } else {
                const size_t o = (size_t)split * 2 * slab + ((size_t)co * a.Fout + fo) * J + p.j;
                a.work[o] = accr[n][e];
                a.work[o + slab] = acci[n][e];
            }
        }
    }
}

template <int NT>
__global__ __launch_bounds__(SC_THREADS) void stream_cconv_bf16_kernel(const SconvArgs a) {
    cconv_bf16_body<NT, false>(a, SconvRows{});
}

template <int NT>
__global__ __launch_bounds__(SC_THREADS) void stream_cconv_bf16_rows_kernel(const SconvArgs a, const SconvRows r) {
    cconv_bf16_body<NT, true>(a, r);
}

// w_re / w_im: conv [Cout][Cin][5][2], transposed [Cin][Cout][5][2] -> [co tiles of 32][groups of 4 ci][5][real hi, real lo,
// imaginary hi, imaginary lo][64 lanes][4 words].  Lane l holds the A operand of row co = 32 * tile + (l & 31) for time tap
// l >> 5 (0: the x[t-1] tap); word c is channel 4 g + c: (wr, -wi) for the real tile, (wi, wr) for the imaginary one, as two bf16.
// The negation comes before the split (both parts of the split are odd functions, so it makes no difference).
__global__ void stream_pack_cconv_bf16_kernel(const float* __restrict__ w_re, const float* __restrict__ w_im,
                                              const float* __restrict__ b_re, const float* __restrict__ b_im, int Cin, int Cout,
                                              int transposed, unsigned* __restrict__ w, float* __restrict__ bias) {
    const int ntile = (Cout + BF_CO - 1) / BF_CO, ngroup = (Cin + BF_CG - 1) / BF_CG;
    const long long n = (long long)ntile * ngroup * 5 * BF_FRAG * 4;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e & 3);
        const int lane = (int)((e >> 2) & 63);
        const int frag = (int)((e >> 8) & 3);
        const int kf = (int)((e >> 10) % 5);
        const int g = (int)((e / (5LL * 1024)) % ngroup);
        const int tile = (int)(e / (5LL * 1024 * ngroup));
        const int co = tile * BF_CO + (lane & 31), ci = g * BF_CG + c;
        float v0 = 0.f, v1 = 0.f;
        if (co < Cout && ci < Cin) {
            const int tap_prev = transposed ? 1 : 0;
            const int kt = (lane >> 5) ? 1 - tap_prev : tap_prev;
            const size_t src = transposed ? (((size_t)ci * Cout + co) * 5 + kf) * 2 + kt : (((size_t)co * Cin + ci) * 5 + kf) * 2 + kt;
            v0 = (frag & 2) ? w_im[src] : w_re[src];
            v1 = (frag & 2) ? w_re[src] : -w_im[src];
        }
        unsigned hi, lo;
        split2(v0, v1, hi, lo);
        w[e] = (frag & 1) ? lo : hi;
    }
    for (int co = blockIdx.x * blockDim.x + threadIdx.x; co < Cout; co += gridDim.x * blockDim.x) {
        bias[2 * co] = b_re[co] - b_im[co];
        bias[2 * co + 1] = b_re[co] + b_im[co];
    }
}

template <int NT>
void launch_nt(const SconvArgs& a, const SconvRows& r, bool rows, dim3 grid, hipStream_t st) {
    if (rows)
        hipLaunchKernelGGL(stream_cconv_bf16_rows_kernel<NT>, grid, dim3(SC_THREADS), 0, st, a, r);
    else
        hipLaunchKernelGGL(stream_cconv_bf16_kernel<NT>, grid, dim3(SC_THREADS), 0, st, a);
}

}  // namespace

// Cin < 4: at least 12 of the 16 k slots of every MFMA would hold zeros (enc0 has one input channel) and the six bf16 MFMAs of a
// step cost what three of the four fp32 ones they replace do; such blocks stay on the fp32 engines.  Measured with enc0 admitted
// (its bits checked on exact integers): no difference in a hop push at B = 1, 256 and 512.
extern "C" int idv_stream_cconv_bf16_supported(int transposed, int Cin, int Cout) {
    (void)transposed;
    if (Cin <= 0 || Cout <= 0) return -1;
    return Cout >= 16 && Cin >= BF_CG ? 1 : 0;
}

extern "C" long long idv_stream_cconv_bf16_wfloats(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return -1;
    return (long long)((Cout + BF_CO - 1) / BF_CO) * ((Cin + BF_CG - 1) / BF_CG) * 5 * BF_FRAG * 4;
}

extern "C" int idv_stream_pack_cconv_bf16(const float* w_re, const float* w_im, const float* b_re, const float* b_im, int Cin,
                                          int Cout, int transposed, float* w, float* bias, void* stream) {
    if (!w_re || !w_im || !b_re || !b_im || !w || !bias || Cin <= 0 || Cout <= 0) return IDV_EINVAL;
    if (reinterpret_cast<size_t>(w) % 16) return IDV_EINVAL;            // the kernel reads 16 bytes per lane
    const long long n = idv_stream_cconv_bf16_wfloats(Cin, Cout);
    long long g = (n + 255) / 256;
    g = g > 4096 ? 4096 : (g < 1 ? 1 : g);
    hipLaunchKernelGGL(stream_pack_cconv_bf16_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, w_re, w_im, b_re, b_im, Cin,
                       Cout, transposed ? 1 : 0, reinterpret_cast<unsigned*>(w), bias);
    return idv_launch_status();
}

// rows NULL: the lock-step entry
static int launch_cconv_bf16(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                             const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist_out,
                             float* x0hist_out, float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k, int Tp, int Jp,
                             const long long* rows, void* stream) {
    if (!x0 || !h0 || C0 <= 0 || C1 < 0 || (C1 > 0 && (!x1 || !h1)) || !w || !bias || !out || Cout <= 0 ||
        Fin <= 0 || B <= 0 || k <= 0 || Tp < k + 1 || Jp < B * Tp || nsplit <= 0 || (nsplit > 1 && !work))
        return IDV_EINVAL;
    if (idv_stream_cconv_bf16_supported(transposed, C0 + C1, Cout) != 1 || reinterpret_cast<size_t>(w) % 16) return IDV_EINVAL;
    SconvArgs a{};
    a.x0 = x0; a.h0 = h0; a.C0 = C0; a.x1 = x1; a.h1 = h1; a.C1 = C1;
    a.w = w; a.bias = bias; a.fold = fold; a.slope = prelu_slope;
    a.out = out; a.hist_out = hist_out; a.x0hist_out = x0hist_out; a.work = work;
    a.transposed = transposed ? 1 : 0; a.Cout = Cout; a.Fin = Fin; a.Fout = fout_of(a.transposed, Fin);
    a.B = B; a.k = k; a.Tp = Tp; a.Jp = Jp; a.nsplit = nsplit;
    const int Cin = C0 + C1;
    a.cps = (Cin + nsplit - 1) / nsplit;
    const long long J = (long long)B * k;
    const int nfq = a.transposed ? Fin : a.Fout;
    const long long pos = nfq * J;
    if (pos > 0x7fffffffLL - BF_WAVES * 2 * 32) return IDV_EINVAL;
    const unsigned gy = (unsigned)((Cout + BF_CO - 1) / BF_CO), gz = (unsigned)(nsplit * (a.transposed ? 2 : 1));
    // two tiles per wave where that still leaves about a workgroup per compute unit, else one (the rule of the fp32 MFMA engine)
    const int nt = (pos + BF_WAVES * 2 * 32 - 1) / (BF_WAVES * 2 * 32) * gy * gz < 256 ? 1 : 2;
    const dim3 grid((unsigned)((pos + BF_WAVES * nt * 32 - 1) / (BF_WAVES * nt * 32)), gy, gz);
    hipStream_t st = (hipStream_t)stream;
    const SconvRows r{rows, (size_t)2 * C0 * Fin * B, (size_t)2 * C1 * Fin * B, (size_t)2 * Cout * a.Fout * B};
    if (nt == 2) launch_nt<2>(a, r, rows != nullptr, grid, st);
    else launch_nt<1>(a, r, rows != nullptr, grid, st);
    const int rc = idv_launch_status();
    if (rc || nsplit == 1) return rc;
    return launch_combine(a, r, rows != nullptr, st);
}

extern "C" int idv_stream_cconv_bf16(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1,
                                     const float* w, const float* bias, const float* fold, const float* prelu_slope, float* out,
                                     float* hist_out, float* x0hist_out, float* work, int nsplit, int transposed, int Cout, int Fin,
                                     int B, int k, int Tp, int Jp, void* stream) {
    return launch_cconv_bf16(x0, h0, C0, x1, h1, C1, w, bias, fold, prelu_slope, out, hist_out, x0hist_out, work, nsplit, transposed,
                             Cout, Fin, B, k, Tp, Jp, nullptr, stream);
}

extern "C" int idv_stream_cconv_bf16_rows(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1,
                                          const float* w, const float* bias, const float* fold, const float* prelu_slope, float* out,
                                          float* hist, float* x0hist, float* work, int nsplit, int transposed, int Cout, int Fin, int B,
                                          int k_launch, int Tp, int Jp, const long long* rows, void* stream) {
    if (!rows) return IDV_EINVAL;
    return launch_cconv_bf16(x0, h0, C0, x1, h1, C1, w, bias, fold, prelu_slope, out, hist, x0hist, work, nsplit, transposed, Cout, Fin,
                             B, k_launch, Tp, Jp, rows, stream);
}
