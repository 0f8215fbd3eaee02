// Multi-tensor kernels of the data-parallel train step: the gradient bucket (gather before / scatter after the RCCL
// all-reduce) and the Adam update, each ONE launch over a pointer table instead of one torch kernel per parameter.
//
// The reference is single-GPU stock torch: `optimizer.step()` of torch.optim.Adam(lr, weight_decay = 0.001)
// (supervised_dccrn/train.py:109, 239-243; i_dccrn_vae/nsvae_dccrn/train_nsvae.py:200, 557-561;
// i_dccrn_vae/nsvae_dccrn/train_second_phase_decoder.py:420-433); the bucket is the MI355X-native addition north_star names
// ("a single RCCL all-reduce of gradients over xGMI per step").
//
// Layout: a bucket is a flat fp32 buffer in which tensor i occupies [off_i, off_i + numel_i), off_i a multiple of 4 floats
// (16 bytes) and the gap up to off_{i+1} padding (kept zero).  table[i] = {device pointer, off_i, numel_i} as three int64,
// sorted by off_i; `total` = off_n (multiple of 4).  A thread owns one 16-byte group of the flat buffer, which by the
// alignment of the offsets lies inside ONE tensor: float4 on the flat side always, float4 on the tensor side when its base
// pointer is 16-byte aligned (torch allocations are), scalar otherwise and for a tensor's last partial group.
// HBM-bound: 8 bytes moved per gradient element and direction (25 M parameters of the NSVAE encoder: 2 x 100 MB).
//
// Global gradient norm, clipping and the non-finite guard: bucket_sqnorm_kernel writes one double partial
// sum of squares per 4096 floats of a table, bucket_clip_finalize_kernel (one workgroup) adds the partials of all tables
// and writes the 32-byte ClipRecord, bucket_adam_clipped_kernel / bucket_scale_kernel read the coefficient (and the skip
// decision) from that record: no host read between them.  Every sum is a double sum of exact squares in a fixed order
// (per thread in increasing flat index, a fixed butterfly across the wave, the four wave sums in wave order), no atomics.
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

constexpr int BK_THREADS = 256;
constexpr int BK_CHUNK = BK_THREADS * 4;      // floats of the flat buffer per workgroup

// index of the tensor whose range holds flat element g (g < total): largest i with off_i <= g
__device__ __forceinline__ int bucket_find(const long long* __restrict__ table, int n, long long g0, long long g, int* s_idx) {
    if (threadIdx.x == 0) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[3 * mid + 1] <= g0) lo = mid; else hi = mid - 1;
        }
        *s_idx = lo;
    }
    __syncthreads();
    int idx = *s_idx;
    while (idx + 1 < n && table[3 * (idx + 1) + 1] <= g) ++idx;
    return idx;
}

// GATHER: flat <- tensors (a NULL pointer contributes zeros; padding is written as zero)
// !GATHER: tensors <- scale * flat
template <bool GATHER>
__global__ void __launch_bounds__(BK_THREADS) bucket_copy_kernel(const long long* __restrict__ table, int n, long long total,
                                                                 float* __restrict__ flat, float scale) {
    __shared__ int s_idx;
    const long long g0 = (long long)blockIdx.x * BK_CHUNK;
    const long long g = g0 + 4 * threadIdx.x;
    const int idx = bucket_find(table, n, g0, g < total ? g : g0, &s_idx);
    if (g >= total) return;
    float* tp = reinterpret_cast<float*>(table[3 * idx]);
    const long long local = g - table[3 * idx + 1];
    const long long left = table[3 * idx + 2] - local;          // valid elements from here (<= 0 inside the padding)
    float4* fl = reinterpret_cast<float4*>(flat + g);
    if (GATHER) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tp && left >= 4 && !(reinterpret_cast<uintptr_t>(tp) & 15)) {
            v = *reinterpret_cast<const float4*>(tp + local);
        } else if (tp && left > 0) {
            v.x = tp[local];
            if (left > 1) v.y = tp[local + 1];
            if (left > 2) v.z = tp[local + 2];
            if (left > 3) v.w = tp[local + 3];
        }
        *fl = v;
    } else {
        if (!tp || left <= 0) return;
        float4 v = *fl;
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        if (left >= 4 && !(reinterpret_cast<uintptr_t>(tp) & 15)) {
            *reinterpret_cast<float4*>(tp + local) = v;
        } else {
            tp[local] = v.x;
            if (left > 1) tp[local + 1] = v.y;
            if (left > 2) tp[local + 2] = v.z;
            if (left > 3) tp[local + 3] = v.w;
        }
    }
}

struct AdamArgs {
    const long long* ptable;      // parameters
    const long long* gtable;      // gradients (same offsets / sizes), or NULL: gflat
    const float* gflat;           // gradients in the bucket layout (e.g. the all-reduced bucket), or NULL: gtable
    float* m;                     // exp_avg, bucket layout
    float* v;                     // exp_avg_sq, bucket layout
    int n;
    long long total;
    float lr, beta1, beta2, omb1, omb2, eps, wd, bc1, bc2s, gscale;   // omb = 1 - beta rounded from double as torch does; bc1 = 1 - beta1^t, bc2s = sqrt(1 - beta2^t)
};

// The 32-byte device record of one norm pass (IDV_CLIP_* in the header are these byte offsets).
struct ClipRecord {
    double sumsq;                 // sum over every gradient element of (float)(g * grad_scale), squared in double
    double norm;                  // sqrt(sumsq)
    float coef;                   // min(1, max_norm / (norm + 1e-6)) formed in double, rounded once; 1 when max_norm <= 0
    int finite;                   // isfinite(sumsq)
    long long skipped;            // guarded steps refused so far (kept across calls; the host zeroes it when it rebases)
};
static_assert(sizeof(ClipRecord) == IDV_CLIP_RECORD_BYTES && offsetof(ClipRecord, sumsq) == IDV_CLIP_SUMSQ &&
              offsetof(ClipRecord, norm) == IDV_CLIP_NORM && offsetof(ClipRecord, coef) == IDV_CLIP_COEF &&
              offsetof(ClipRecord, finite) == IDV_CLIP_FINITE && offsetof(ClipRecord, skipped) == IDV_CLIP_SKIPPED, "ClipRecord layout");

// torch.optim.Adam (no amsgrad, no maximize), in its own order of operations:
//   g += wd * p;  m = lerp(m, g, 1 - beta1);  v = beta2 * v + (1 - beta2) g^2;  p -= (lr / bc1) * m / (sqrt(v) / bc2s + eps)
// CLIP: g = (g * grad_scale) * coef + wd * p with the product g * grad_scale ROUNDED first -- the value the norm pass squared --
// so coef == 1 returns the bits of the unclipped form whenever g * grad_scale is exact (grad_scale a power of two).
template <bool CLIP>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a, float coef) {
    if (CLIP) g = __fmaf_rn(__fmul_rn(g, a.gscale), coef, __fmul_rn(a.wd, p));
    else g = g * a.gscale + a.wd * p;
    m = m + (g - m) * a.omb1;
    v = a.beta2 * v + a.omb2 * g * g;
    const float denom = __fsqrt_rn(v) / a.bc2s + a.eps;
    p = p - (a.lr / a.bc1) * (m / denom);
}

// one 16-byte group of the bucket per thread; the caller has found idx (bucket_find) and checked g < a.total
template <bool CLIP>
__device__ __forceinline__ void adam_group(const AdamArgs& a, int idx, long long g, float coef) {
    float* pp = reinterpret_cast<float*>(a.ptable[3 * idx]);
    const long long local = g - a.ptable[3 * idx + 1];
    const long long left = a.ptable[3 * idx + 2] - local;
    if (!pp || left <= 0) return;
    const float* gp = a.gflat ? a.gflat + g : (reinterpret_cast<const float*>(a.gtable[3 * idx]) + local);
    if (!a.gflat && !a.gtable[3 * idx]) return;                 // parameter without a gradient: torch skips it
    const bool vec = left >= 4 && !(reinterpret_cast<uintptr_t>(pp) & 15) && !(reinterpret_cast<uintptr_t>(gp) & 15);
    float4 m4 = *reinterpret_cast<float4*>(a.m + g), v4 = *reinterpret_cast<float4*>(a.v + g);
    float pv[4], gv[4];
    float mv[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
    const int cnt = left >= 4 ? 4 : (int)left;
    if (vec) {
        const float4 p4 = *reinterpret_cast<const float4*>(pp + local), g4 = *reinterpret_cast<const float4*>(gp);
        pv[0] = p4.x; pv[1] = p4.y; pv[2] = p4.z; pv[3] = p4.w;
        gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            pv[e] = e < cnt ? pp[local + e] : 0.f;
            gv[e] = e < cnt ? gp[e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < cnt) adam_one<CLIP>(pv[e], gv[e], mv[e], vv[e], a, coef);
    if (vec) {
        *reinterpret_cast<float4*>(pp + local) = make_float4(pv[0], pv[1], pv[2], pv[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) pp[local + e] = pv[e];
    }
    *reinterpret_cast<float4*>(a.m + g) = make_float4(mv[0], mv[1], mv[2], mv[3]);
    *reinterpret_cast<float4*>(a.v + g) = make_float4(vv[0], vv[1], vv[2], vv[3]);
}

__global__ void __launch_bounds__(BK_THREADS) bucket_adam_kernel(const AdamArgs a) {
    __shared__ int s_idx;
    const long long g0 = (long long)blockIdx.x * BK_CHUNK;
    const long long g = g0 + 4 * threadIdx.x;
    const int idx = bucket_find(a.ptable, a.n, g0, g < a.total ? g : g0, &s_idx);
    if (g >= a.total) return;
    adam_group<false>(a, idx, g, 1.0f);
}

// The Adam step behind a norm pass.  coef and, with the guard, the skip decision and the count of refused steps come from the
// record: a refused step returns before any store, and the bias corrections are formed here from t = t_host - skipped, so a
// refused step does not advance them either.  Without the guard the host's corrections (a.bc1, a.bc2s) are used as they are.
__global__ void __launch_bounds__(BK_THREADS) bucket_adam_clipped_kernel(AdamArgs a, const ClipRecord* __restrict__ rec, int guard,
                                                                         long long t_host, double beta1d, double beta2d) {
    __shared__ int s_idx;
    __shared__ float s_bc[2];
    if (guard) {
        if (!rec->finite) return;                               // the same word for every thread of the grid
        if (threadIdx.x == 0) {
            long long t = t_host - rec->skipped;
            if (t < 1) t = 1;
            s_bc[0] = (float)(1.0 - pow(beta1d, (double)t));
            s_bc[1] = (float)sqrt(1.0 - pow(beta2d, (double)t));
        }
    }
    const float coef = rec->coef;
    const long long g0 = (long long)blockIdx.x * BK_CHUNK;
    const long long g = g0 + 4 * threadIdx.x;
    const int idx = bucket_find(a.ptable, a.n, g0, g < a.total ? g : g0, &s_idx);      // its barrier also publishes s_bc
    if (g >= a.total) return;
    if (guard) {
        a.bc1 = s_bc[0];
        a.bc2s = s_bc[1];
    }
    adam_group<true>(a, idx, g, coef);
}

// ---- sums of squares: double, fixed order ---------------------------------------------------------------------------------------
constexpr int SQ_GROUPS = 4;                          // 16-byte groups per thread, BK_CHUNK floats apart
constexpr int SQ_CHUNK = BK_CHUNK * SQ_GROUPS;        // floats of the flat buffer per workgroup = per partial

// sum over the workgroup, the same in every run: xor butterfly across the wave (both partners add the same two numbers), then
// the wave sums in wave order through LDS
__device__ __forceinline__ double block_sum(double s, double* s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = s_w[0];
#pragma unroll
    for (int w = 1; w < BK_THREADS / 64; ++w) t += s_w[w];
    return t;
}

// partials[first + blockIdx.x] = sum of ((double)(g * gscale))^2 over the elements of flat range [4096 k, 4096 (k + 1)) that
// belong to a present parameter with a gradient.  Padding and absent rows are never added (only loaded on the flat side).
__global__ void __launch_bounds__(BK_THREADS) bucket_sqnorm_kernel(const long long* __restrict__ ptable, const long long* __restrict__ gtable,
                                                                   const float* __restrict__ gflat, int n, long long total, float gscale,
                                                                   double* __restrict__ partials, long long first) {
    __shared__ int s_idx;
    __shared__ double s_w[BK_THREADS / 64];
    const long long g0 = (long long)blockIdx.x * SQ_CHUNK;
    const long long gt = g0 + 4 * threadIdx.x;
    int idx = bucket_find(ptable, n, g0, gt < total ? gt : g0, &s_idx);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < SQ_GROUPS; ++j) {
        const long long g = gt + (long long)j * BK_CHUNK;
        if (g >= total) break;
        while (idx + 1 < n && ptable[3 * (idx + 1) + 1] <= g) ++idx;
        const long long local = g - ptable[3 * idx + 1];
        const long long left = ptable[3 * idx + 2] - local;
        if (!ptable[3 * idx] || left <= 0) continue;
        if (!gflat && !gtable[3 * idx]) continue;
        const float* gp = gflat ? gflat + g : (reinterpret_cast<const float*>(gtable[3 * idx]) + local);
        const int cnt = left >= 4 ? 4 : (int)left;
        float gv[4];
        if (gflat || (left >= 4 && !(reinterpret_cast<uintptr_t>(gp) & 15))) {       // the flat side is aligned and padded to 4
            const float4 g4 = *reinterpret_cast<const float4*>(gp);
            gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[e] = e < cnt ? gp[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) {
                const double x = (double)__fmul_rn(gv[e], gscale);
                s += x * x;                                     // 24 x 24 bits: the square is exact in double
            }
    }
    const double t = block_sum(s, s_w);
    if (threadIdx.x == 0) partials[first + blockIdx.x] = t;
}

__global__ void __launch_bounds__(BK_THREADS) bucket_clip_finalize_kernel(const double* __restrict__ partials, int count, double max_norm,
                                                                          int guard, ClipRecord* __restrict__ rec) {
    __shared__ double s_w[BK_THREADS / 64];
    double s = 0.0;
    for (int k = threadIdx.x; k < count; k += BK_THREADS) s += partials[k];
    const double sumsq = block_sum(s, s_w);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(sumsq);
    double c = 1.0;
    if (max_norm > 0.0) {
        c = max_norm / (norm + 1e-6);
        c = c > 1.0 ? 1.0 : c;                                  // a NaN norm stays a NaN coefficient, as torch's clamp leaves it
    }
    const int finite = isfinite(sumsq) ? 1 : 0;
    rec->sumsq = sumsq;
    rec->norm = norm;
    rec->coef = (float)c;
    rec->finite = finite;
    if (guard && !finite) rec->skipped = rec->skipped + 1;
}

// tensors *= coef of the record (the scatter kernel's addressing without a flat side); coef == 1 writes nothing
__global__ void __launch_bounds__(BK_THREADS) bucket_scale_kernel(const long long* __restrict__ table, int n, long long total,
                                                                  const ClipRecord* __restrict__ rec) {
    __shared__ int s_idx;
    const float coef = rec->coef;
    if (coef == 1.0f) return;
    const long long g0 = (long long)blockIdx.x * BK_CHUNK;
    const long long g = g0 + 4 * threadIdx.x;
    const int idx = bucket_find(table, n, g0, g < total ? g : g0, &s_idx);
    if (g >= total) return;
    float* tp = reinterpret_cast<float*>(table[3 * idx]);
    const long long local = g - table[3 * idx + 1];
    const long long left = table[3 * idx + 2] - local;
    if (!tp || left <= 0) return;
    if (left >= 4 && !(reinterpret_cast<uintptr_t>(tp) & 15)) {
        float4 v = *reinterpret_cast<const float4*>(tp + local);
        v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
        *reinterpret_cast<float4*>(tp + local) = v;
    } else {
        tp[local] *= coef;
        if (left > 1) tp[local + 1] *= coef;
        if (left > 2) tp[local + 2] *= coef;
        if (left > 3) tp[local + 3] *= coef;
    }
}

int check_bucket(const void* table, int n, long long total, const void* flat) {
    if (!table || n <= 0 || total <= 0 || (total & 3) || !flat || (reinterpret_cast<uintptr_t>(flat) & 15)) return IDV_EINVAL;
    if ((total + BK_CHUNK - 1) / BK_CHUNK > 0x7fffffffLL) return IDV_EINVAL;
    return IDV_OK;
}

// the table side of check_bucket, for the entries that have no flat buffer of their own
int check_table(const void* table, int n, long long total) {
    if (!table || n <= 0 || total <= 0 || (total & 3)) return IDV_EINVAL;
    if ((total + BK_CHUNK - 1) / BK_CHUNK > 0x7fffffffLL) return IDV_EINVAL;
    return IDV_OK;
}

bool aligned8(const void* q) { return q && !(reinterpret_cast<uintptr_t>(q) & 7); }

}  // namespace

extern "C" int idv_bucket_gather(const long long* table, int n, long long total, float* flat, void* stream) {
    if (int rc = check_bucket(table, n, total, flat)) return rc;
    hipLaunchKernelGGL(bucket_copy_kernel<true>, dim3((unsigned)((total + BK_CHUNK - 1) / BK_CHUNK)), dim3(BK_THREADS), 0,
                       (hipStream_t)stream, table, n, total, flat, 1.0f);
    return idv_launch_status();
}

extern "C" int idv_bucket_scatter(const long long* table, int n, long long total, const float* flat, float scale, void* stream) {
    if (int rc = check_bucket(table, n, total, flat)) return rc;
    hipLaunchKernelGGL(bucket_copy_kernel<false>, dim3((unsigned)((total + BK_CHUNK - 1) / BK_CHUNK)), dim3(BK_THREADS), 0,
                       (hipStream_t)stream, table, n, total, const_cast<float*>(flat), scale);
    return idv_launch_status();
}

extern "C" int idv_bucket_adam(const long long* ptable, const long long* gtable, const float* gflat, float* exp_avg, float* exp_avg_sq,
                               int n, long long total, float lr, double beta1d, double beta2d, float eps, float weight_decay,
                               float bias_correction1, float bias_correction2_sqrt, float grad_scale, void* stream) {
    const float beta1 = (float)beta1d, beta2 = (float)beta2d;
    if (int rc = check_bucket(ptable, n, total, exp_avg)) return rc;
    if (!exp_avg_sq || (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15) || (!gtable == !gflat)) return IDV_EINVAL;
    if (gflat && (reinterpret_cast<uintptr_t>(gflat) & 15)) return IDV_EINVAL;
    if (!(bias_correction1 > 0.f) || !(bias_correction2_sqrt > 0.f)) return IDV_EINVAL;
    // 1 - beta in double, THEN rounded: what torch hands its kernels (1 - 0.999f in float is off by 1.3e-5 relative)
    AdamArgs a{ptable, gtable, gflat, exp_avg, exp_avg_sq, n, total, lr, beta1, beta2, (float)(1.0 - (double)beta1d), (float)(1.0 - (double)beta2d),
               eps, weight_decay, bias_correction1, bias_correction2_sqrt, grad_scale};
    hipLaunchKernelGGL(bucket_adam_kernel, dim3((unsigned)((total + BK_CHUNK - 1) / BK_CHUNK)), dim3(BK_THREADS), 0,
                       (hipStream_t)stream, a);
    return idv_launch_status();
}

extern "C" int idv_bucket_sqnorm_partials(long long total) {
    if (total <= 0 || (total & 3) || (total + BK_CHUNK - 1) / BK_CHUNK > 0x7fffffffLL) return -1;
    return (int)((total + SQ_CHUNK - 1) / SQ_CHUNK);
}

extern "C" int idv_bucket_sqnorm(const long long* ptable, const long long* gtable, const float* gflat, int n, long long total,
                                 float grad_scale, double* partials, long long first, void* stream) {
    if (int rc = check_table(ptable, n, total)) return rc;
    if ((!gtable == !gflat) || (gflat && (reinterpret_cast<uintptr_t>(gflat) & 15))) return IDV_EINVAL;
    if (!aligned8(partials) || first < 0) return IDV_EINVAL;
    hipLaunchKernelGGL(bucket_sqnorm_kernel, dim3((unsigned)((total + SQ_CHUNK - 1) / SQ_CHUNK)), dim3(BK_THREADS), 0, (hipStream_t)stream,
                       ptable, gtable, gflat, n, total, grad_scale, partials, first);
    return idv_launch_status();
}

extern "C" int idv_bucket_clip_finalize(const double* partials, int count, double max_norm, int guard, void* record, void* stream) {
    if (!aligned8(partials) || !aligned8(record) || count <= 0 || max_norm != max_norm) return IDV_EINVAL;
    hipLaunchKernelGGL(bucket_clip_finalize_kernel, dim3(1), dim3(BK_THREADS), 0, (hipStream_t)stream, partials, count, max_norm, guard,
                       static_cast<ClipRecord*>(record));
    return idv_launch_status();
}

extern "C" int idv_bucket_adam_clipped(const long long* ptable, const long long* gtable, const float* gflat, float* exp_avg, float* exp_avg_sq,
                                       int n, long long total, float lr, double beta1d, double beta2d, float eps, float weight_decay,
                                       float bias_correction1, float bias_correction2_sqrt, float grad_scale, const void* record, int guard,
                                       long long t_host, void* stream) {
    const float beta1 = (float)beta1d, beta2 = (float)beta2d;
    if (int rc = check_bucket(ptable, n, total, exp_avg)) return rc;
    if (!exp_avg_sq || (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15) || (!gtable == !gflat)) return IDV_EINVAL;
    if (gflat && (reinterpret_cast<uintptr_t>(gflat) & 15)) return IDV_EINVAL;
    if (!(bias_correction1 > 0.f) || !(bias_correction2_sqrt > 0.f)) return IDV_EINVAL;
    if (!aligned8(record) || (guard && t_host < 1)) return IDV_EINVAL;
    AdamArgs a{ptable, gtable, gflat, exp_avg, exp_avg_sq, n, total, lr, beta1, beta2, (float)(1.0 - (double)beta1d), (float)(1.0 - (double)beta2d),
               eps, weight_decay, bias_correction1, bias_correction2_sqrt, grad_scale};
    hipLaunchKernelGGL(bucket_adam_clipped_kernel, dim3((unsigned)((total + BK_CHUNK - 1) / BK_CHUNK)), dim3(BK_THREADS), 0,
                       (hipStream_t)stream, a, static_cast<const ClipRecord*>(record), guard, t_host, beta1d, beta2d);
    return idv_launch_status();
}

extern "C" int idv_bucket_scale(const long long* table, int n, long long total, const void* record, void* stream) {
    if (int rc = check_table(table, n, total)) return rc;
    if (!aligned8(record)) return IDV_EINVAL;
    hipLaunchKernelGGL(bucket_scale_kernel, dim3((unsigned)((total + BK_CHUNK - 1) / BK_CHUNK)), dim3(BK_THREADS), 0, (hipStream_t)stream,
                       table, n, total, static_cast<const ClipRecord*>(record));
    return idv_launch_status();
}
