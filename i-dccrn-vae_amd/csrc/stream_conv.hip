// Streaming complex conv / transposed conv of the DCCRN blocks (model/complex_progress.py:8-36, 222-279) over the k frames
// that one push of streaming.StreamingDCCRN completes, with the frame before them taken from a per-stream history column.
//
// Time taps: conv y[t] = W0 x[t-1] + W1 x[t], transposed y[t] = W0 x[t] + W1 x[t-1] (causal crop).  x[t-1] of a stream's
// first frame comes from hist_in ([2][C][F][B]), of the others from the same source; the last output column of every stream
// goes to hist_out (NULL: no consumer), so the next push finds its x[t-1] there.  The caller double-buffers hist by push parity: a block reads
// hist[p] and writes hist[1-p], and the consumer of this block's output still finds the previous column in hist[p].
//
// Vector-ALU contraction: one lane = one (output bin, column), CO_T complex output channels in registers; the weights of one
// (ci, kf) are the same for the whole workgroup (scalar loads).  Split-K over the input channels: nsplit parts write
// partial sums, idv_stream_cconv_combine adds them in the order 0..nsplit-1 and runs the epilogue (bias, folded eval BN,
// PReLU).  nsplit is a function of the layer shape and B only (idv_stream_cconv_splits), so the arithmetic of every column
// is the same however a signal is cut into pushes.
#include "stream_conv.hpp"

namespace {

// grid: x = position blocks, y = co tiles, z = split * (transposed ? 2 : 1) + output-bin parity
template <int CO_T, bool ROWS>
__device__ __forceinline__ void cconv_body(const SconvArgs& a, const SconvRows& r) {
    const int J = a.B * a.k;
    const int par = a.transposed ? (int)(blockIdx.z & 1) : 0;
    const int split = a.transposed ? (int)(blockIdx.z >> 1) : (int)blockIdx.z;
    const int cot = blockIdx.y;
    const int Cin = a.C0 + a.C1;

    // last input column of x0 -> x0hist_out (the source's own producer cannot write its history)
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
    const int q = blockIdx.x * SC_THREADS + threadIdx.x;
    const bool live = q < nfq * J;
    const int fq = live ? q / J : 0, j = live ? q - (q / J) * J : 0;
    const int b = j / a.k, t = j - b * a.k;
    const int fo = a.transposed ? 2 * fq + par : fq;
    const int ci0 = split * a.cps, ci1 = min(Cin, ci0 + a.cps);
    RowOf rw{a.k, 0};
    if (ROWS) rw = row_of(r, b);
    const float* h0 = a.h0 + (ROWS ? (size_t)rw.parity * r.h0_half : 0);
    const float* h1 = a.h1 + (ROWS ? (size_t)rw.parity * r.h1_half : 0);

    float accr[CO_T], acci[CO_T];
#pragma unroll
    for (int c = 0; c < CO_T; ++c) accr[c] = acci[c] = 0.f;

    const size_t colc = (size_t)b * a.Tp + 1 + t;
    for (int ci = ci0; ci < ci1; ++ci) {
        const bool second = ci >= a.C0;
        const float* x = second ? a.x1 : a.x0;
        const float* hs = second ? h1 : h0;
        const int C = second ? a.C1 : a.C0;
        const int cl = second ? ci - a.C0 : ci;
        const size_t pr = (size_t)cl * a.Fin, pi = (size_t)(C + cl) * a.Fin;
        const float* wc = a.w + ((size_t)cot * Cin + ci) * 5 * CO_T * 4;
        for (int kf = a.transposed ? par : 0; kf < 5; kf += a.transposed ? 2 : 1) {
            const int fi = a.transposed ? (fo + 2 - kf) / 2 : 2 * fo - 2 + kf;
            const bool ok = live && fi >= 0 && fi < a.Fin;
            float xcr = 0.f, xci = 0.f, xpr = 0.f, xpi = 0.f;
            if (ok) {
                xcr = x[(pr + fi) * a.Jp + colc];
                xci = x[(pi + fi) * a.Jp + colc];
                if (t > 0) {
                    xpr = x[(pr + fi) * a.Jp + colc - 1];
                    xpi = x[(pi + fi) * a.Jp + colc - 1];
                } else {
                    xpr = hs[(pr + fi) * a.B + b];
                    xpi = hs[(pi + fi) * a.B + b];
                }
            }
            const float* wk = wc + kf * CO_T * 4;
#pragma unroll
            for (int c = 0; c < CO_T; ++c) {
                const float wrp = wk[4 * c], wip = wk[4 * c + 1], wrc = wk[4 * c + 2], wic = wk[4 * c + 3];
                accr[c] = fmaf(wrp, xpr, accr[c]);
                accr[c] = fmaf(-wip, xpi, accr[c]);
                accr[c] = fmaf(wrc, xcr, accr[c]);
                accr[c] = fmaf(-wic, xci, accr[c]);
                acci[c] = fmaf(wrp, xpi, acci[c]);
                acci[c] = fmaf(wip, xpr, acci[c]);
                acci[c] = fmaf(wrc, xci, acci[c]);
                acci[c] = fmaf(wic, xcr, acci[c]);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < CO_T; ++c) {
        const int co = cot * CO_T + c;
        if (co >= a.Cout) break;
        if (a.nsplit == 1) {
            epilogue(a, co, fo, b, t, accr[c], acci[c],
                     ROWS && a.hist_out ? a.hist_out + (size_t)(1 - rw.parity) * r.out_half : a.hist_out, rw.k - 1);
        } else {
            const size_t slab = (size_t)a.Cout * a.Fout * J;
            const size_t o = (size_t)split * 2 * slab + ((size_t)co * a.Fout + fo) * J + j;
            a.work[o] = accr[c];
            a.work[o + slab] = acci[c];
        }
    }
}

template <int CO_T>
__global__ __launch_bounds__(SC_THREADS) void stream_cconv_kernel(const SconvArgs a) {
    cconv_body<CO_T, false>(a, SconvRows{});
}

template <int CO_T>
__global__ __launch_bounds__(SC_THREADS) void stream_cconv_rows_kernel(const SconvArgs a, const SconvRows r) {
    cconv_body<CO_T, true>(a, r);
}

// w_re / w_im: conv [Cout][Cin][5][2], transposed [Cin][Cout][5][2]; taps reordered to (x[t-1], x[t])
__global__ void stream_pack_cconv_kernel(const float* __restrict__ w_re, const float* __restrict__ w_im,
                                         const float* __restrict__ b_re, const float* __restrict__ b_im, int Cin, int Cout,
                                         int transposed, int co_t, float* __restrict__ w, float* __restrict__ bias) {
    const int ntile = (Cout + co_t - 1) / co_t;
    const long long n = (long long)ntile * Cin * 5 * co_t * 4;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(e & 3);
        const int c = (int)((e >> 2) % co_t);
        const int kf = (int)((e / (4LL * co_t)) % 5);
        const int ci = (int)((e / (20LL * co_t)) % Cin);
        const int tile = (int)(e / (20LL * co_t * Cin));
        const int co = tile * co_t + c;
        float v = 0.f;
        if (co < Cout) {
            const int tap_prev = transposed ? 1 : 0;
            const int kt = (r < 2) ? tap_prev : 1 - tap_prev;
            const size_t src = transposed ? (((size_t)ci * Cout + co) * 5 + kf) * 2 + kt : (((size_t)co * Cin + ci) * 5 + kf) * 2 + kt;
            v = (r & 1) ? w_im[src] : w_re[src];
        }
        w[e] = v;
    }
    for (int co = blockIdx.x * blockDim.x + threadIdx.x; co < Cout; co += gridDim.x * blockDim.x) {
        bias[2 * co] = b_re[co] - b_im[co];
        bias[2 * co + 1] = b_re[co] + b_im[co];
    }
}

inline int co_tile(int Cout) { return Cout >= 16 ? 16 : 1; }

}  // namespace

extern "C" long long idv_stream_cconv_wfloats(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return -1;
    const int ct = co_tile(Cout);
    return (long long)((Cout + ct - 1) / ct) * Cin * 5 * ct * 4;
}

extern "C" int idv_stream_pack_cconv(const float* w_re, const float* w_im, const float* b_re, const float* b_im, int Cin, int Cout,
                                     int transposed, float* w, float* bias, void* stream) {
    if (!w_re || !w_im || !b_re || !b_im || !w || !bias || Cin <= 0 || Cout <= 0) return IDV_EINVAL;
    const long long n = idv_stream_cconv_wfloats(Cin, Cout);
    long long g = (n + 255) / 256;
    g = g > 4096 ? 4096 : (g < 1 ? 1 : g);
    hipLaunchKernelGGL(stream_pack_cconv_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, w_re, w_im, b_re, b_im, Cin,
                       Cout, transposed ? 1 : 0, co_tile(Cout), w, bias);
    return idv_launch_status();
}

extern "C" int idv_stream_cconv_splits(int transposed, int Cin, int Cout, int Fin, int B) {
    if (Cin <= 0 || Cout <= 0 || Fin <= 0 || B <= 0) return -1;
    // about 1024 workgroups at one frame per stream, no part below 8 input channels, at most 32 parts
    const int ct = co_tile(Cout);
    const long long pos = (long long)(transposed ? 2 * Fin - 1 : fout_of(0, Fin)) * B;
    const long long wgs = (pos + SC_THREADS - 1) / SC_THREADS * ((Cout + ct - 1) / ct);
    long long s = 1024 / (wgs > 0 ? wgs : 1);
    const long long smax = Cin / 8 > 1 ? Cin / 8 : 1;
    if (s > smax) s = smax;
    if (s > 32) s = 32;
    return s < 1 ? 1 : (int)s;
}

// rows NULL: the lock-step entry
static int launch_cconv(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                        const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist_out, float* x0hist_out,
                        float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k, int Tp, int Jp, const long long* rows,
                        void* stream) {
    if (!x0 || !h0 || C0 <= 0 || C1 < 0 || (C1 > 0 && (!x1 || !h1)) || !w || !bias || !out || Cout <= 0 ||
        Fin <= 0 || B <= 0 || k <= 0 || Tp < k + 1 || Jp < B * Tp || nsplit <= 0 || (nsplit > 1 && !work))
        return IDV_EINVAL;
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
    if (pos > 0x7fffffffLL) return IDV_EINVAL;
    const int ct = co_tile(Cout);
    dim3 grid((unsigned)((pos + SC_THREADS - 1) / SC_THREADS), (unsigned)((Cout + ct - 1) / ct),
              (unsigned)(nsplit * (a.transposed ? 2 : 1)));
    hipStream_t st = (hipStream_t)stream;
    const SconvRows r{rows, (size_t)2 * C0 * Fin * B, (size_t)2 * C1 * Fin * B, (size_t)2 * Cout * a.Fout * B};
    if (rows && ct == 16)
        hipLaunchKernelGGL(stream_cconv_rows_kernel<16>, grid, dim3(SC_THREADS), 0, st, a, r);
    else if (rows)
        hipLaunchKernelGGL(stream_cconv_rows_kernel<1>, grid, dim3(SC_THREADS), 0, st, a, r);
    else if (ct == 16)
        hipLaunchKernelGGL(stream_cconv_kernel<16>, grid, dim3(SC_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(stream_cconv_kernel<1>, grid, dim3(SC_THREADS), 0, st, a);
    int rc = idv_launch_status();
    if (rc || nsplit == 1) return rc;
    return launch_combine(a, r, rows != nullptr, st);
}

extern "C" int idv_stream_cconv(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1,
                                const float* w, const float* bias, const float* fold, const float* prelu_slope, float* out,
                                float* hist_out, float* x0hist_out, float* work, int nsplit, int transposed, int Cout, int Fin,
                                int B, int k, int Tp, int Jp, void* stream) {
    return launch_cconv(x0, h0, C0, x1, h1, C1, w, bias, fold, prelu_slope, out, hist_out, x0hist_out, work, nsplit, transposed, Cout,
                        Fin, B, k, Tp, Jp, nullptr, stream);
}

extern "C" int idv_stream_cconv_rows(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1,
                                     const float* w, const float* bias, const float* fold, const float* prelu_slope, float* out,
                                     float* hist, float* x0hist, float* work, int nsplit, int transposed, int Cout, int Fin, int B,
                                     int k_launch, int Tp, int Jp, const long long* rows, void* stream) {
    if (!rows) return IDV_EINVAL;
    return launch_cconv(x0, h0, C0, x1, h1, C1, w, bias, fold, prelu_slope, out, hist, x0hist, work, nsplit, transposed, Cout, Fin, B,
                        k_launch, Tp, Jp, rows, stream);
}
