// What the streaming conv units (stream_conv.hip: vector ALU, stream_conv_mfma.hip: fp32 MFMA) share: the launch arguments, the
// row table access, the epilogue and the split-K combine.  One text for both engines: a restated epilogue could be contracted
// differently by the compiler, and the engines are bit-identical only while they round the same way.
#pragma once
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int SC_THREADS = 256;

struct SconvArgs {
    const float* x0; const float* h0; int C0;
    const float* x1; const float* h1; int C1;
    const float* w;         // vector ALU: [co tiles][Cin][5][CO_T][4]: (wr, wi) of the x[t-1] tap, (wr, wi) of the x[t] tap
                            // MFMA: [co tiles of 32][Cin][5][4: re prev, re cur, im prev, im cur][64 lanes] (stream_conv_mfma.hip)
    const float* bias;      // [Cout][2]: (b_re - b_im, b_re + b_im)
    const float* fold;      // [Cout][6] or NULL
    const float* slope;     // PReLU slope or NULL
    float* out; float* hist_out; float* x0hist_out;
    float* work;            // [nsplit][2][Cout][Fout][J] partial sums (nsplit > 1)
    int transposed, Cout, Fin, Fout, B, k, Tp, Jp, nsplit, cps;
};

// The per-row entry (idv_stream_cconv_rows): k above is k_launch, h0 / h1 / hist_out / x0hist_out are the bases of both parity
// halves, and slot b reads half parity_b, writes half 1 - parity_b from its column k_b - 1 (nothing when k_b = 0).
struct SconvRows {
    const long long* rows;
    size_t h0_half, h1_half, out_half;      // floats per parity half of h0 / h1 / hist_out (x0hist_out: h0_half)
};

struct RowOf {
    int k, parity;
};

__device__ __forceinline__ RowOf row_of(const SconvRows& r, int b) {
    const long long* q = r.rows + (size_t)b * IDV_STREAM_ROW_FIELDS;
    return RowOf{(int)q[IDV_ROW_K], (int)q[IDV_ROW_PARITY]};
}

// t_hist: the column that goes to hist (the slot's last one)
__device__ __forceinline__ void epilogue(const SconvArgs& a, int co, int fo, int b, int t, float vr, float vi, float* hist, int t_hist) {
    vr += a.bias[2 * co];
    vi += a.bias[2 * co + 1];
    if (a.fold) {
        const float* z = a.fold + (size_t)co * 6;
        const float r = z[0] * vr + z[1] * vi + z[4];
        const float i = z[2] * vr + z[3] * vi + z[5];
        vr = r; vi = i;
    }
    if (a.slope) {
        const float s = *a.slope;
        vr = vr >= 0.f ? vr : s * vr;
        vi = vi >= 0.f ? vi : s * vi;
    }
    const size_t plane = (size_t)a.Fout * a.Jp;
    const size_t o = (size_t)co * plane + (size_t)fo * a.Jp + (size_t)b * a.Tp + 1 + t;
    a.out[o] = vr;
    a.out[(size_t)a.Cout * plane + o] = vi;
    if (hist && t == t_hist) {
        const size_t h = ((size_t)co * a.Fout + fo) * a.B + b;
        hist[h] = vr;
        hist[(size_t)a.Cout * a.Fout * a.B + h] = vi;
    }
}

template <bool ROWS>
__device__ __forceinline__ void combine_body(const SconvArgs& a, const SconvRows& r) {
    const int J = a.B * a.k;
    const long long n = (long long)a.Cout * a.Fout * J;
    const size_t slab = (size_t)n;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e % J);
        const int fo = (int)((e / J) % a.Fout);
        const int co = (int)(e / ((long long)J * a.Fout));
        float vr = 0.f, vi = 0.f;
        for (int s = 0; s < a.nsplit; ++s) {             // fixed order
            vr += a.work[(size_t)s * 2 * slab + e];
            vi += a.work[(size_t)s * 2 * slab + slab + e];
        }
        const int b = j / a.k;
        RowOf rw{a.k, 0};
        if (ROWS) rw = row_of(r, b);
        epilogue(a, co, fo, b, j % a.k, vr, vi, ROWS && a.hist_out ? a.hist_out + (size_t)(1 - rw.parity) * r.out_half : a.hist_out,
                 rw.k - 1);
    }
}

__global__ void stream_cconv_combine_kernel(const SconvArgs a) { combine_body<false>(a, SconvRows{}); }

__global__ void stream_cconv_combine_rows_kernel(const SconvArgs a, const SconvRows r) { combine_body<true>(a, r); }

// adds the nsplit partial sums of a launch in the order 0..nsplit-1 and runs the epilogue (rows: the per-row entry)
inline int launch_combine(const SconvArgs& a, const SconvRows& r, bool rows, hipStream_t st) {
    long long g = ((long long)a.Cout * a.Fout * a.B * a.k + 255) / 256;
    g = g > 4096 ? 4096 : (g < 1 ? 1 : g);
    if (rows)
        hipLaunchKernelGGL(stream_cconv_combine_rows_kernel, dim3((unsigned)g), dim3(256), 0, st, a, r);
    else
        hipLaunchKernelGGL(stream_cconv_combine_kernel, dim3((unsigned)g), dim3(256), 0, st, a);
    return idv_launch_status();
}

inline int fout_of(int transposed, int Fin) { return transposed ? 2 * Fin - 1 : (Fin - 1) / 2 + 1; }

}  // namespace
