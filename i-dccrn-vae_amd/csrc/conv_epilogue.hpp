// What the epilogues of the four exact-fp32 conv kernel families share (cgemm_gauss.hip, cgemm_wino.hip, cgemm_tw.hip, cgemm_tw2.hip),
// and the start and end of their *_fwd entries.  Per output point (channel co, row fo, column j):
//     (re, im) = contraction (+ addend)  ->  Z (re, im) + s  |  (re, im) + b  ->  PReLU  ->  0 in the guard columns  ->  out,
// and in train mode the five moment sums of the result.  Every helper has the form that leaves every kernel's machine code as it
// was: values in, values or a small struct out, the guard-column select at the call site.  The column mask and the
// moment flush stay in the kernels: as helpers they changed the code of some instantiations.
#pragma once
#include "common.hpp"

struct EpiRow {
    f32x4 z;        // Zrr, Zri, Zir, Zii
    float sr, si;   // (Z b + s), or b without a fold
};
struct EpiPoint {
    float r, i;
};

// row co of the table [rows][8]; it is allocated for every row of every co tile
__device__ __forceinline__ EpiRow epi_row(const float* epi, int co) {
    EpiRow e;
    e.z = *(const f32x4*)(epi + (size_t)co * 8);
    e.sr = epi[(size_t)co * 8 + 4];
    e.si = epi[(size_t)co * 8 + 5];
    return e;
}

// the skip-once addend, planar [2][Cout][Fout][add_Jp], of plane-channel c (co | Cout + co) at row fo, addend column ja
__device__ __forceinline__ float epi_addend(const float* add, int c, int Fout, int fo, int add_Jp, int ja) {
    return add[((size_t)c * Fout + fo) * add_Jp + ja];
}

// folded complex batch norm (or the plain bias), then PReLU
__device__ __forceinline__ EpiPoint epi_point(float re, float im, f32x4 e0, float e4, float e5, int has_fold, bool has_act, float slope) {
    EpiPoint y;
    if (has_fold) {
        y.r = e0[0] * re + e0[1] * im + e4;
        y.i = e0[2] * re + e0[3] * im + e5;
    } else {
        y.r = re + e4;
        y.i = im + e5;
    }
    if (has_act) {
        y.r = y.r >= 0.f ? y.r : slope * y.r;
        y.i = y.i >= 0.f ? y.i : slope * y.i;
    }
    return y;
}

// the train-mode moment sums (r, i, rr, ii, ri) of one output point
__device__ __forceinline__ void epi_stats_add(float (&st)[5], float yr, float yi) {
    st[0] += yr;
    st[1] += yi;
    st[2] += yr * yr;
    st[3] += yi * yi;
    st[4] += yr * yi;
}

// ---- host: where a *_fwd entry's moment sums go.  stats alone: the kernels add to it.  stats and work: they add to one of `rep`
// replicas in work (a power of two, common.hpp) and finish() folds the replicas into stats.
struct EpiStatsTarget {
    double* stats;
    double* work;
    int rep;
    bool replicated() const { return stats && work; }
    bool ok() const { return !replicated() || (rep >= 2 && !(rep & (rep - 1))); }
    template <class Args>
    void set(Args& a) const {
        a.stats = replicated() ? work : stats;
        if (replicated()) a.stats_rep = rep;
    }
    int finish(int rc, int Cout, hipStream_t st) const {
        if (rc || !replicated()) return rc;
        return idv_launch_stats_collapse(work, rep, Cout * 5, stats, st);
    }
};
