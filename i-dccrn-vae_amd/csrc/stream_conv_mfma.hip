// The streaming complex conv / transposed conv of stream_conv.hip on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): the same
// function, the same arguments and, bit for bit, the same result.
//
// Why the bits agree: an f32 MFMA is a k-ordered fmaf chain with one rounding per product, and stream_conv.hip is an explicit
// fmaf chain.  The two k of one MFMA are (re, im) of ONE time tap, so per (ci, kf) four MFMAs feed the accumulators exactly the
// products of the vector-ALU kernel in its order:
//   real tile       A = (wr, -wi)   B = (xr, xi)    x[t-1] tap, then x[t] tap
//   imaginary tile  A = (wr,  wi)   B = (xi, xr)    x[t-1] tap, then x[t] tap
// ci ascends inside a K part, kf inside ci (the parity's taps only when transposed), frequency rows outside the input give
// zero operands (they are not skipped), K parts go to `work` and the shared combine kernel adds them 0..nsplit-1, and the
// epilogue is the one text of stream_conv.hpp.
//
// Mapping: the 32 columns of a tile are 32 consecutive positions q = fq * J + j of the vector-ALU kernel's position space (one
// output-bin parity, j = b * k + t), so a single stream with one frame still fills tiles with its output bins.  A lane holds
// column q = lane & 31 and k = lane >> 5: it reads "its" plane (re for k = 0, im for k = 1) for the real tile and the other one
// for the imaginary tile, straight from the planar source and the history (no LDS, no barrier: every operand is read once per
// wave, and the rows shared between output bins and co tiles come from L2).  A wave owns NT = 1 or 2 tiles (NT * 32 positions)
// of the 32 output channels of its co tile, real and imaginary: 2 * NT accumulators of 16 registers; the A fragments of a
// (ci, kf) are four coalesced 256-byte loads from the pre-packed weights, reused over the NT tiles.  The operands of step s + 1
// are loaded before the MFMAs of step s are issued.  NT is chosen from the launch size only to fill the card; no bit depends
// on it.
#include "stream_conv.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MF_CO = 32;                       // output channels per workgroup: one real and one imaginary 32-row tile
constexpr int MF_WAVES = SC_THREADS / 64;
constexpr int MF_FRAG = 4 * 64;                 // floats of one (ci, kf): re prev, re cur, im prev, im cur, 64 lanes each

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

// grid: x = blocks of MF_WAVES * NT * 32 positions, y = co tiles of 32, z = split * (transposed ? 2 : 1) + output-bin parity
template <int NT, bool ROWS>
__device__ __forceinline__ void cconv_mfma_body(const SconvArgs& a, const SconvRows& r) {
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
    const int col = lane & 31, hk = lane >> 5;
    const int q0 = ((int)blockIdx.x * MF_WAVES + wave) * (NT * 32) + col;
    if (q0 - col >= nq) return;                               // the whole wave; the kernel has no barrier
    const int ci0 = split * a.cps, ci1 = min(Cin, ci0 + a.cps);
    const int nk = a.transposed ? (par == 0 ? 3 : 2) : 5;     // taps kf = par, par + 2, .. when transposed
    const float* wt = a.w + (size_t)cot * Cin * 5 * MF_FRAG + lane;

    f32x16 accr[NT], acci[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) accr[n][e] = acci[n][e] = 0.f;

    struct Frag {
        float w[4];
        float x[NT][4];
    };

    for (int src = 0; src < 2; ++src) {
        const int cb = src ? max(ci0, a.C0) : ci0, ce = src ? ci1 : min(ci1, a.C0);
        if (cb >= ce) continue;
        const float* x = src ? a.x1 : a.x0;
        const float* hs = src ? a.h1 : a.h0;
        const int C = src ? a.C1 : a.C0, cbase = src ? a.C0 : 0;
        const long long xplane = (long long)C * a.Fin * a.Jp, hplane = (long long)C * a.Fin * a.B;
        const long long xd = hk ? -xplane : xplane;           // from the lane's own plane to the other one

        // per tile: the lane's column in its own plane at input row fi0 (kf = 0), for the x[t] and the x[t-1] tap
        const float* pc[NT];
        const float* pp[NT];
        long long pd[NT];
        int ps[NT], fi0[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const Pos p = pos_of(q0 + n * 32, nq, J, a.k);
            const int f0 = a.transposed ? p.fq + 1 : 2 * p.fq - 2;             // fi = f0 + d, d = kf (conv) or -m (transposed)
            fi0[n] = p.live ? f0 : -0x40000000;
            pc[n] = x + (hk ? xplane : 0) + (long long)f0 * a.Jp + (long long)p.b * a.Tp + 1 + p.t;
            if (p.t > 0) {
                pp[n] = pc[n] - 1; ps[n] = a.Jp; pd[n] = xd;
            } else {
                size_t half = 0;
                if (ROWS && p.live) half = (size_t)row_of(r, p.b).parity * (src ? r.h1_half : r.h0_half);
                pp[n] = hs + half + (hk ? hplane : 0) + (long long)f0 * a.B + p.b; ps[n] = a.B; pd[n] = hk ? -hplane : hplane;
            }
        }

        auto load = [&](int cl, int m, Frag& f) {
            const int kf = a.transposed ? par + 2 * m : m;
            const int d = a.transposed ? -m : m;
            const float* wk = wt + ((size_t)(cbase + cl) * 5 + kf) * MF_FRAG;
#pragma unroll
            for (int e = 0; e < 4; ++e) f.w[e] = wk[64 * e];
            const long long row = (long long)cl * a.Fin + d;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f.x[n][0] = f.x[n][1] = f.x[n][2] = f.x[n][3] = 0.f;
                if ((unsigned)(fi0[n] + d) < (unsigned)a.Fin) {
                    const float* c = pc[n] + row * a.Jp;
                    const float* p = pp[n] + row * ps[n];
                    f.x[n][0] = p[0];
                    f.x[n][1] = c[0];
                    f.x[n][2] = p[pd[n]];
                    f.x[n][3] = c[xd];
                }
            }
        };

        Frag cur;
        int cl = cb - cbase, m = 0;
        const int cle = ce - cbase;
        load(cl, m, cur);
        for (;;) {
            int ncl = cl, nm = m + 1;
            if (nm == nk) { nm = 0; ++ncl; }
            const bool more = ncl < cle;
            Frag nxt;
            load(more ? ncl : cl, more ? nm : m, nxt);
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                accr[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.w[0], cur.x[n][0], accr[n], 0, 0, 0);
                acci[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.w[2], cur.x[n][2], acci[n], 0, 0, 0);
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                accr[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.w[1], cur.x[n][1], accr[n], 0, 0, 0);
                acci[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.w[3], cur.x[n][3], acci[n], 0, 0, 0);
            }
            if (!more) break;
            cur = nxt; cl = ncl; m = nm;
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
            const int co = cot * MF_CO + (e & 3) + 8 * (e >> 2) + 4 * hk;
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
__global__ __launch_bounds__(SC_THREADS) void stream_cconv_mfma_kernel(const SconvArgs a) {
    cconv_mfma_body<NT, false>(a, SconvRows{});
}

template <int NT>
__global__ __launch_bounds__(SC_THREADS) void stream_cconv_mfma_rows_kernel(const SconvArgs a, const SconvRows r) {
    cconv_mfma_body<NT, true>(a, r);
}

// w_re / w_im: conv [Cout][Cin][5][2], transposed [Cin][Cout][5][2] -> [co tiles of 32][Cin][5][re prev, re cur, im prev, im cur][64]:
// lane l holds the A operand of row co = 32 * tile + (l & 31), k = l >> 5: wr for k = 0, -wi (real tile) or wi (imaginary tile)
// for k = 1; rows past Cout are zero.  The negation is done here, so the operand is exact.
__global__ void stream_pack_cconv_mfma_kernel(const float* __restrict__ w_re, const float* __restrict__ w_im,
                                              const float* __restrict__ b_re, const float* __restrict__ b_im, int Cin, int Cout,
                                              int transposed, float* __restrict__ w, float* __restrict__ bias) {
    const int ntile = (Cout + MF_CO - 1) / MF_CO;
    const long long n = (long long)ntile * Cin * 5 * MF_FRAG;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(e & 63);
        const int frag = (int)((e >> 6) & 3);
        const int kf = (int)((e / MF_FRAG) % 5);
        const int ci = (int)((e / (5LL * MF_FRAG)) % Cin);
        const int tile = (int)(e / (5LL * MF_FRAG * Cin));
        const int co = tile * MF_CO + (lane & 31);
        float v = 0.f;
        if (co < Cout) {
            const int tap_prev = transposed ? 1 : 0;
            const int kt = (frag & 1) ? 1 - tap_prev : tap_prev;
            const size_t src = transposed ? (((size_t)ci * Cout + co) * 5 + kf) * 2 + kt : (((size_t)co * Cin + ci) * 5 + kf) * 2 + kt;
            v = (lane >> 5) == 0 ? w_re[src] : ((frag & 2) ? w_im[src] : -w_im[src]);
        }
        w[e] = v;
    }
    for (int co = blockIdx.x * blockDim.x + threadIdx.x; co < Cout; co += gridDim.x * blockDim.x) {
        bias[2 * co] = b_re[co] - b_im[co];
        bias[2 * co + 1] = b_re[co] + b_im[co];
    }
}

template <int NT>
void launch_nt(const SconvArgs& a, const SconvRows& r, bool rows, dim3 grid, hipStream_t st) {
    if (rows)
        hipLaunchKernelGGL(stream_cconv_mfma_rows_kernel<NT>, grid, dim3(SC_THREADS), 0, st, a, r);
    else
        hipLaunchKernelGGL(stream_cconv_mfma_kernel<NT>, grid, dim3(SC_THREADS), 0, st, a);
}

}  // namespace

extern "C" int idv_stream_cconv_mfma_supported(int transposed, int Cin, int Cout) {
    (void)transposed;
    if (Cin <= 0 || Cout <= 0) return -1;
    return Cout >= 16 ? 1 : 0;
}

extern "C" long long idv_stream_cconv_mfma_wfloats(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return -1;
    return (long long)((Cout + MF_CO - 1) / MF_CO) * Cin * 5 * MF_FRAG;
}

extern "C" int idv_stream_pack_cconv_mfma(const float* w_re, const float* w_im, const float* b_re, const float* b_im, int Cin,
                                          int Cout, int transposed, float* w, float* bias, void* stream) {
    if (!w_re || !w_im || !b_re || !b_im || !w || !bias || Cin <= 0 || Cout <= 0) return IDV_EINVAL;
    const long long n = idv_stream_cconv_mfma_wfloats(Cin, Cout);
    long long g = (n + 255) / 256;
    g = g > 4096 ? 4096 : (g < 1 ? 1 : g);
    hipLaunchKernelGGL(stream_pack_cconv_mfma_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, w_re, w_im, b_re, b_im, Cin,
                       Cout, transposed ? 1 : 0, w, bias);
    return idv_launch_status();
}

// rows NULL: the lock-step entry
static int launch_cconv_mfma(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                             const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist_out,
                             float* x0hist_out, float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k, int Tp, int Jp,
                             const long long* rows, void* stream) {
    if (!x0 || !h0 || C0 <= 0 || C1 < 0 || (C1 > 0 && (!x1 || !h1)) || !w || !bias || !out || Cout <= 0 ||
        Fin <= 0 || B <= 0 || k <= 0 || Tp < k + 1 || Jp < B * Tp || nsplit <= 0 || (nsplit > 1 && !work))
        return IDV_EINVAL;
    if (idv_stream_cconv_mfma_supported(transposed, C0 + C1, Cout) != 1) return IDV_EINVAL;
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
    if (pos > 0x7fffffffLL - MF_WAVES * 2 * 32) return IDV_EINVAL;
    const unsigned gy = (unsigned)((Cout + MF_CO - 1) / MF_CO), gz = (unsigned)(nsplit * (a.transposed ? 2 : 1));
    // two tiles per wave where that still leaves about a workgroup per compute unit, else one (four tiles per wave need 280
    // registers, one wave per SIMD, and measured slower: DESIGN 3.6)
    const int nt = (pos + MF_WAVES * 2 * 32 - 1) / (MF_WAVES * 2 * 32) * gy * gz < 256 ? 1 : 2;
    const dim3 grid((unsigned)((pos + MF_WAVES * nt * 32 - 1) / (MF_WAVES * nt * 32)), gy, gz);
    hipStream_t st = (hipStream_t)stream;
    const SconvRows r{rows, (size_t)2 * C0 * Fin * B, (size_t)2 * C1 * Fin * B, (size_t)2 * Cout * a.Fout * B};
    if (nt == 2) launch_nt<2>(a, r, rows != nullptr, grid, st);
    else launch_nt<1>(a, r, rows != nullptr, grid, st);
    const int rc = idv_launch_status();
    if (rc || nsplit == 1) return rc;
    return launch_combine(a, r, rows != nullptr, st);
}

extern "C" int idv_stream_cconv_mfma(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1,
                                     const float* w, const float* bias, const float* fold, const float* prelu_slope, float* out,
                                     float* hist_out, float* x0hist_out, float* work, int nsplit, int transposed, int Cout, int Fin,
                                     int B, int k, int Tp, int Jp, void* stream) {
    return launch_cconv_mfma(x0, h0, C0, x1, h1, C1, w, bias, fold, prelu_slope, out, hist_out, x0hist_out, work, nsplit, transposed,
                             Cout, Fin, B, k, Tp, Jp, nullptr, stream);
}

extern "C" int idv_stream_cconv_mfma_rows(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1,
                                          const float* w, const float* bias, const float* fold, const float* prelu_slope, float* out,
                                          float* hist, float* x0hist, float* work, int nsplit, int transposed, int Cout, int Fin, int B,
                                          int k_launch, int Tp, int Jp, const long long* rows, void* stream) {
    if (!rows) return IDV_EINVAL;
    return launch_cconv_mfma(x0, h0, C0, x1, h1, C1, w, bias, fold, prelu_slope, out, hist, x0hist, work, nsplit, transposed, Cout, Fin,
                             B, k_launch, Tp, Jp, rows, stream);
}
