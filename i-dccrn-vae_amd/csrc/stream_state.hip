// Save and load of a slot's stream (streaming._Slots.save / load): the per-slot state of a sessions object
// lies in up to 64 device buffers, each an [outer][B][inner] view (streaming._Slots._zero_views).  A slot's record is the
// concatenation of its [outer][inner] blocks of every view, per_slot floats; gather copies the records of the named slots to
// out[n_slots][per_slot], scatter copies them back, each in ONE launch whatever the number of views and slots.
//
// The view table (IDV_STATE_VIEW_FIELDS long longs per view: buffer address, outer, inner, offset of the view inside a record)
// is staged in LDS; element e of the [n_slots][per_slot] side finds its view by a binary search over the offsets, at most
// 6 steps for 64 views.  The record side is read / written coalesced (consecutive lanes, consecutive floats); the buffer side
// is contiguous for inner > 1 and strided by B for the histories (inner = 1).  Plain vector loads and stores, no atomics;
// nothing outside the named slots' elements is touched.  The device entries cannot look at device tables, so
// idv_stream_state_check holds the HOST copies of both tables to the contract before they are uploaded.
#include "common.hpp"
#include "../../include/idccrn_hip.h"

namespace {

inline int grid_of(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

template <bool SCATTER>
__global__ void stream_state_kernel(const long long* __restrict__ views, int n_views, int B, const long long* __restrict__ slots,
                                    int n_slots, float* rec, long long per_slot) {
    __shared__ long long tab[IDV_STATE_MAX_VIEWS * IDV_STATE_VIEW_FIELDS];
    for (int j = threadIdx.x; j < n_views * IDV_STATE_VIEW_FIELDS; j += blockDim.x) tab[j] = views[j];
    __syncthreads();
    const long long n = per_slot * n_slots;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long r = e % per_slot;
        const long long b = slots[e / per_slot];
        // the last view whose offset is <= r (the offsets increase from 0, so view 0 always qualifies)
        int lo = 0, hi = n_views - 1;
#pragma unroll 1
        for (int step = 0; step < 7 && lo < hi; ++step) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[mid * IDV_STATE_VIEW_FIELDS + IDV_STATE_VIEW_OFFSET] <= r)
                lo = mid;
            else
                hi = mid - 1;
        }
        const long long* v = tab + lo * IDV_STATE_VIEW_FIELDS;
        float* buf = reinterpret_cast<float*>(v[IDV_STATE_VIEW_ADDR]);
        const long long inner = v[IDV_STATE_VIEW_INNER];
        const long long q = r - v[IDV_STATE_VIEW_OFFSET];
        const size_t at = ((size_t)(q / inner) * B + (size_t)b) * inner + (size_t)(q % inner);
        if (SCATTER)
            buf[at] = rec[e];
        else
            rec[e] = buf[at];
    }
}

bool launch_args_ok(const long long* views, int n_views, int B, const long long* slots, int n_slots, const float* rec,
                    long long per_slot) {
    return views && slots && rec && n_views > 0 && n_views <= IDV_STATE_MAX_VIEWS && B > 0 && n_slots > 0 && n_slots <= B &&
           per_slot > 0;
}

}  // namespace

extern "C" int idv_stream_state_check(const long long* views_host, int n_views, int B, const long long* slots_host, int n_slots,
                                      long long per_slot) {
    if (!views_host || !slots_host || n_views <= 0 || n_views > IDV_STATE_MAX_VIEWS || B <= 0 || n_slots <= 0 || n_slots > B ||
        per_slot <= 0)
        return IDV_EINVAL;
    long long off = 0;                              // the views tile [0, per_slot): each starts where the one before it ends
    for (int j = 0; j < n_views; ++j) {
        const long long* v = views_host + (size_t)j * IDV_STATE_VIEW_FIELDS;
        if (v[IDV_STATE_VIEW_ADDR] == 0 || v[IDV_STATE_VIEW_OUTER] <= 0 || v[IDV_STATE_VIEW_INNER] <= 0 ||
            v[IDV_STATE_VIEW_OFFSET] != off)
            return IDV_EINVAL;
        if (v[IDV_STATE_VIEW_OUTER] > per_slot / v[IDV_STATE_VIEW_INNER]) return IDV_EINVAL;      // no overflow of the product
        off += v[IDV_STATE_VIEW_OUTER] * v[IDV_STATE_VIEW_INNER];
        if (off > per_slot) return IDV_EINVAL;
    }
    if (off != per_slot) return IDV_EINVAL;
    for (int s = 0; s < n_slots; ++s) {
        if (slots_host[s] < 0 || slots_host[s] >= B) return IDV_EINVAL;
        for (int t = 0; t < s; ++t)
            if (slots_host[t] == slots_host[s]) return IDV_EINVAL;
    }
    return IDV_OK;
}

extern "C" int idv_stream_state_gather(const long long* views, int n_views, int B, const long long* slots, int n_slots, float* out,
                                       long long per_slot, void* stream) {
    if (!launch_args_ok(views, n_views, B, slots, n_slots, out, per_slot)) return IDV_EINVAL;
    hipLaunchKernelGGL(stream_state_kernel<false>, dim3(grid_of(per_slot * n_slots)), dim3(256), 0, (hipStream_t)stream, views, n_views,
                       B, slots, n_slots, out, per_slot);
    return idv_launch_status();
}

extern "C" int idv_stream_state_scatter(const long long* views, int n_views, int B, const long long* slots, int n_slots,
                                        const float* in, long long per_slot, void* stream) {
    if (!launch_args_ok(views, n_views, B, slots, n_slots, in, per_slot)) return IDV_EINVAL;
    hipLaunchKernelGGL(stream_state_kernel<true>, dim3(grid_of(per_slot * n_slots)), dim3(256), 0, (hipStream_t)stream, views, n_views,
                       B, slots, n_slots, const_cast<float*>(in), per_slot);
    return idv_launch_status();
}
