// Room impulse responses of rectangular rooms by the image-source method (Allen & Berkley 1979): dataset/rir.py shoebox_rir,
// RirPool.shoebox (the definition is restated in float64 numpy by tests/ism_ref.py).
//
// Room b is the record geom[b][IDV_ISM_FIELDS]: size L, source s, microphone r, six wall coefficients beta, fs, c.  Image (m, q) of
// axis a lies at p = ((2 m) L + (q ? -s : s)) - r, was reflected e0 = |m - q| times at the wall at 0 and e1 = |m| times at the far
// wall, g = beta0^e0 beta1^e1.  With d = sqrt((px px + py py) + pz pz), A = gx gy gz / (4 pi d), tau = (d fs) / c, n_i = rint(tau),
// f = tau - n_i, u = n - tau:
//
//   h[n] = float( sum_i A sinc(u) w(u) ),  |u| < 40.5,   sinc(0) = 1,  sinc(u) = (-1)^(n - n_i + 1) sin(pi f) / (pi u),
//   w(u) = (1 + cos(2 pi u / 81)) / 2 = cos^2(pi u / 81)
//
// Floating-point contraction is OFF in this file: p, d and tau are the IEEE double operations above in that order, with the
// correctly rounded sqrt and division of the device, so tau, u and f have the bits the reference has and no image changes its sample
// or its side of |u| < 40.5 against it.
//
// One wave (a workgroup of 64 threads) owns a tile of 64 samples n0 .. n0 + 63 of one room; lane l owns sample n0 + l.  The images
// that touch the tile have tau in (n0 - 40.5, n0 + 103.5), a spherical shell of distances.  The lanes walk the columns (mx, qx, my,
// qy) of the lattice inside the shell's outer radius, 64 at a time in the order of the column index j = 4 (iy nmx + ix) + 2 qy + qx;
// each lane solves the ranges of mz, for qz = 0 and 1, whose |pz| lies between the shell's radii at the column (at most four
// ranges: qz = 0 below and above zero, then qz = 1), widened by a relative 1e-9 so that no rounding loses an image, and takes its
// r-th candidate in round r.  A candidate is kept on its exact tau (inside the tile's reach), the integer max_order test and A != 0.
// The kept candidates of a round are appended to an LDS list in lane order (ballot and prefix count); when the list could not take
// another round it is summed and emptied.  So the list's order is (column block, round, lane): a function of the room and n0 alone.
//
// Summing: lane l adds the candidates in list order.  k = n - n_i, u = n - tau; the window is cos^2 of pi u / 81 = pi k / 81 - pi f
// / 81 by the angle-addition formula, cos(pi k / 81) and sin(pi k / 81) from an 83-entry LDS table (|k| <= 41), cos and sin of the
// small angle pi f / 81 from the candidate: no cancellation except in the last sample of the window, where the value itself goes to
// zero.  A (sample, image) pair costs a table read, one division and a handful of multiplications; the transcendentals are per image.
//
// Order: every sum is double, in list order; tiles are independent and nothing depends on the batch, on Kmax, on taps[b] (the
// samples below taps[b] are the same for every tap count) or on the pitch.  No atomics.  Only room b's record, taps[b] and
// max_order[b] are read.  A record the kernel cannot walk (a value that is not finite, L, fs or c not positive, more than 8192
// images along an axis inside a tile's radius) gives a row of NaN; dataset/rir.py refuses such rooms on the host.
#include "rows.hpp"
#include "../../include/idccrn_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int ISM_MAX_TAPS = 1 << 16;
constexpr int ISM_W = 81;
constexpr double ISM_HALF = 40.5;
constexpr int ISM_REACH = 41;                     // |n - n_i| <= 41 wherever |u| < 40.5
constexpr int ISM_TILE = 64;                      // samples of a tile, one per lane
constexpr int ISM_CAP = 192;                      // candidates of the LDS list: summed when fewer than 64 places are left
constexpr int ISM_MAX_M = 8192;                   // images along an axis, each side
constexpr double ISM_PI = 3.14159265358979323846;

struct Cand {
    double tau, A, As, cf, sf;                    // As = A sin(pi f); cf, sf = cos, sin(pi f / 81)
    int ni, pad;
};

// lane's sample n += the cnt candidates of the list, in list order
__device__ __forceinline__ void ism_sum(const Cand* __restrict__ list, int cnt, const double* __restrict__ tab, int n, double& acc) {
    for (int i = 0; i < cnt; ++i) {
        const double tau = list[i].tau;
        const int k = n - list[i].ni;
        const double u = (double)n - tau;
        if (fabs(u) < ISM_HALF) {
            const int kk = min(max(k + ISM_REACH, 0), 2 * ISM_REACH);
            const double cw = fma(tab[2 * kk], list[i].cf, tab[2 * kk + 1] * list[i].sf);
            const double sg = (k & 1) ? 1.0 : -1.0;
            const double t = (u == 0.0) ? list[i].A : (sg * list[i].As) / (ISM_PI * u) * (cw * cw);
            acc += t;
        }
    }
}

__global__ __launch_bounds__(64) void ism_kernel(const double* __restrict__ geom, const int* __restrict__ taps,
                                                 const int* __restrict__ max_order, int Kmax, float* __restrict__ h, long long ldh,
                                                 long long* __restrict__ counts, int ntile) {
    __shared__ double tab[2 * (2 * ISM_REACH + 1)];
    __shared__ Cand list[ISM_CAP];
    const int lane = threadIdx.x, b = blockIdx.y;
    const int tile = ntile - 1 - (int)blockIdx.x;                       // the late tiles hold the most images: they start first
    const int n0 = tile * ISM_TILE, n = n0 + lane;
    const int K = max(1, min(taps[b], Kmax));
    float* hr = h + (long long)b * ldh;
    long long* cnt_out = counts + 2 * ((long long)b * ntile + tile);       // (candidates summed, images owned)
    if (n0 >= K) {
        if (n < Kmax) hr[n] = 0.f;
        if (lane < 2) cnt_out[lane] = 0;
        return;
    }
    for (int t = lane; t <= 2 * ISM_REACH; t += 64) {
        // cos and sin of pi k / 81; past |k| = 20 from the complement pi (81 - 2 |k|) / 162, so that the cosine keeps its
        // relative accuracy where it goes through zero (k = +-40.5)
        const int k = t - ISM_REACH, ak = abs(k);
        const double a = (ISM_PI / ISM_W) * (double)ak, co = (ISM_PI / (2 * ISM_W)) * (double)(ISM_W - 2 * ak);
        const double cv = ak > 20 ? sin(co) : cos(a), sv = ak > 20 ? cos(co) : sin(a);
        tab[2 * t] = cv;
        tab[2 * t + 1] = k < 0 ? -sv : sv;
    }
    const double* g = geom + (long long)b * IDV_ISM_FIELDS;
    const double Lx = g[IDV_ISM_LX], Ly = g[IDV_ISM_LY], Lz = g[IDV_ISM_LZ];
    const double sx = g[IDV_ISM_SX], sy = g[IDV_ISM_SY], sz = g[IDV_ISM_SZ];
    const double rx = g[IDV_ISM_RX], ry = g[IDV_ISM_RY], rz = g[IDV_ISM_RZ];
    const double fs = g[IDV_ISM_FS], c = g[IDV_ISM_C];
    const int mo = max_order ? max_order[b] : 0x7fffffff;
    bool fine = Lx > 0 && Ly > 0 && Lz > 0 && fs > 0 && c > 0;
    for (int t = 0; t < IDV_ISM_FIELDS; ++t) fine = fine && isfinite(g[t]);
    const double tlo = (double)n0 - ISM_HALF, thi = (double)(n0 + ISM_TILE - 1) + ISM_HALF;
    const double dhi = fine ? thi * c / fs * (1.0 + 1e-9) : 0.0;
    const double dlo = tlo > 0 ? tlo * c / fs * (1.0 - 1e-9) : 0.0;
    fine = fine && dhi / (2 * Lx) < ISM_MAX_M && dhi / (2 * Ly) < ISM_MAX_M && dhi / (2 * Lz) < ISM_MAX_M;
    if (!fine) {
        if (n < Kmax) hr[n] = n < K ? __builtin_nanf("") : 0.f;
        if (lane < 2) cnt_out[lane] = 0;
        return;
    }
    const double dhi2 = dhi * dhi, dlo2 = dlo * dlo;
    const int Mx = (int)floor(dhi / (2 * Lx)) + 1, My = (int)floor(dhi / (2 * Ly)) + 1;
    const int nmx = 2 * Mx + 1, nmy = 2 * My + 1;
    const int ncol = 4 * nmx * nmy;                                     // <= 4 * 16385^2 < 2^31
    const double tw = 2 * Lz;
    __syncthreads();                                                    // the table

    double acc = 0.0;
    int cnt = 0;
    long long total = 0, owned = 0;
    const bool last = n0 + ISM_TILE >= K;                               // the last tile also owns the images that peak past it,
    const double tset = (double)(K - 1) + ISM_HALF;                     // up to the end of the row's image set
    for (int j0 = 0; j0 < ncol; j0 += 64) {
        const int j = j0 + lane;
        int ra[4] = {0, 0, 0, 0}, rn[4] = {0, 0, 0, 0}, ntot = 0, mx = 0, qx = 0, my = 0, qy = 0, oxy = 0;
        double px = 0, py = 0;
        if (j < ncol) {
            const int col = j >> 2;
            qx = j & 1;
            qy = (j >> 1) & 1;
            mx = col % nmx - Mx;
            my = col / nmx - My;
            px = ((double)(2 * mx) * Lx + (qx ? -sx : sx)) - rx;
            py = ((double)(2 * my) * Ly + (qy ? -sy : sy)) - ry;
            oxy = abs(mx - qx) + abs(mx) + abs(my - qy) + abs(my);
            const double rho2 = px * px + py * py;
            if (rho2 < dhi2 && oxy <= mo) {
                const double zhi = sqrt(dhi2 - rho2), zlo = dlo2 > rho2 ? sqrt(dlo2 - rho2) : 0.0;
#pragma unroll
                for (int qz = 0; qz < 2; ++qz) {
                    const double cz = (qz ? -sz : sz) - rz;
                    const int pa = (int)ceil((zlo - cz) / tw - 1e-6), pb = (int)floor((zhi - cz) / tw + 1e-6);
                    const int na = (int)ceil((-zhi - cz) / tw - 1e-6), nb = min((int)floor((-zlo - cz) / tw + 1e-6), pa - 1);
                    ra[2 * qz] = na;
                    rn[2 * qz] = max(0, nb - na + 1);
                    ra[2 * qz + 1] = pa;
                    rn[2 * qz + 1] = max(0, pb - pa + 1);
                }
                ntot = rn[0] + rn[1] + rn[2] + rn[3];
            }
        }
        for (int r = 0; __ballot(r < ntot) != 0ull; ++r) {
            bool ok = false;
            Cand cd;
            cd.ni = 0;
            cd.tau = 0;
            if (r < ntot) {
                int t = r, base = ra[0], qz = 0;                         // the r-th of the four ranges laid end to end
                if (t >= rn[0]) {
                    t -= rn[0];
                    base = ra[1];
                    if (t >= rn[1]) {
                        t -= rn[1];
                        base = ra[2];
                        qz = 1;
                        if (t >= rn[2]) {
                            t -= rn[2];
                            base = ra[3];
                        }
                    }
                }
                const int mz = base + t;
                const double pz = ((double)(2 * mz) * Lz + (qz ? -sz : sz)) - rz;
                const double d = sqrt((px * px + py * py) + pz * pz);
                const double tau = d * fs / c;
                const int order = oxy + abs(mz - qz) + abs(mz);
                if (tau > tlo && tau < thi && order <= mo) {
                    const double gx = pow(g[IDV_ISM_BETA + 0], (double)abs(mx - qx)) * pow(g[IDV_ISM_BETA + 1], (double)abs(mx));
                    const double gy = pow(g[IDV_ISM_BETA + 2], (double)abs(my - qy)) * pow(g[IDV_ISM_BETA + 3], (double)abs(my));
                    const double gz = pow(g[IDV_ISM_BETA + 4], (double)abs(mz - qz)) * pow(g[IDV_ISM_BETA + 5], (double)abs(mz));
                    const double A = ((gx * gy) * gz) / ((4.0 * ISM_PI) * d);
                    if (A != 0.0) {
                        const double ni = rint(tau), f = tau - ni, af = (ISM_PI / ISM_W) * f;
                        cd.tau = tau;
                        cd.A = A;
                        cd.As = A * sin(ISM_PI * f);
                        cd.cf = cos(af);
                        cd.sf = sin(af);
                        cd.ni = (int)ni;
                        cd.pad = 0;
                        ok = true;
                    }
                }
            }
            const unsigned long long mask = __ballot(ok);
            const int add = __popcll(mask);
            if (cnt + add > ISM_CAP) {                                  // wave-uniform
                __syncthreads();
                ism_sum(list, cnt, tab, n, acc);
                __syncthreads();
                cnt = 0;
            }
            if (ok) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = cd;
            cnt += add;
            total += add;
            owned += __popcll(__ballot(ok && cd.ni >= n0 && (last ? cd.tau < tset : cd.ni < n0 + ISM_TILE)));
        }
    }
    __syncthreads();
    ism_sum(list, cnt, tab, n, acc);
    if (n < Kmax) hr[n] = n < K ? (float)acc : 0.f;
    if (lane == 0) {
        cnt_out[0] = total;
        cnt_out[1] = owned;
    }
}

// the index of max|h| of each row's taps[b] samples, the first on ties
__global__ __launch_bounds__(256) void ism_peaks_kernel(const float* __restrict__ h, long long ldh, const int* __restrict__ taps,
                                                        int* __restrict__ peaks) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = (int)max(1ll, min((long long)taps[b], min(ldh, (long long)ISM_MAX_TAPS)));
    const float* hr = h + (long long)b * ldh;
    float best = -1.f;
    int bi = 0x7fffffff;
    for (int i = tid; i < K; i += 256) {
        const float a = fabsf(hr[i]);
        if (a > best) {                                                 // increasing i: the first of equals stays
            best = a;
            bi = i;
        }
    }
    sv[tid] = best;
    si[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float a2 = sv[tid + o];
            const int i2 = si[tid + o];
            if (a2 > sv[tid] || (a2 == sv[tid] && i2 < si[tid])) {
                sv[tid] = a2;
                si[tid] = i2;
            }
        }
        __syncthreads();
    }
    if (tid == 0) peaks[b] = si[0] == 0x7fffffff ? 0 : si[0];
}

inline bool ism_batch_ok(int B, int Kmax) { return B >= 1 && B <= ROWS_MAX_ROWS && Kmax >= 1 && Kmax <= ISM_MAX_TAPS; }

}  // namespace

extern "C" long long idv_ism_work_bytes(int B, int Kmax) {
    if (!ism_batch_ok(B, Kmax)) return -1;
    return 2 * (long long)sizeof(long long) * B * ((Kmax + ISM_TILE - 1) / ISM_TILE);
}

extern "C" int idv_ism_rir(const double* geom, const int* taps, const int* max_order, int B, int Kmax, float* h, long long ldh, void* work,
                           long long work_bytes, void* stream) {
    if (!geom || !taps || !h || !work || !ism_batch_ok(B, Kmax) || ldh < Kmax) return IDV_EINVAL;
    if (work_bytes < idv_ism_work_bytes(B, Kmax)) return IDV_EINVAL;
    if (!aligned_to(8, {geom, work}) || !aligned_to(4, {taps, max_order, h})) return IDV_EINVAL;
    const int ntile = (Kmax + ISM_TILE - 1) / ISM_TILE;
    hipLaunchKernelGGL(ism_kernel, dim3(ntile, B), dim3(64), 0, (hipStream_t)stream, geom, taps, max_order, Kmax, h, ldh, (long long*)work,
                       ntile);
    return idv_launch_status();
}

extern "C" int idv_ism_peaks(const float* h, long long ldh, const int* taps, int B, int* peaks, void* stream) {
    if (!h || !taps || !peaks || B < 1 || B > ROWS_MAX_ROWS || ldh < 1) return IDV_EINVAL;
    if (!aligned_to(4, {h, taps, peaks})) return IDV_EINVAL;
    hipLaunchKernelGGL(ism_peaks_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, h, ldh, taps, peaks);
    return idv_launch_status();
}
