// cgemm: the one MFMA contraction kernel behind every dense op on the hot path.
//
//   out[m][fo][j] = bias[m] + sum_{cc,kf,kt} W'[m][cc][kf][kt] * x[cc][fi(fo,kf)][j + kt + tshift]
//
// A complex Conv2d / ConvTranspose2d of the reference (model/complex_progress.py:8-36,
// :222-279: four real convolutions + stack) is ONE such real contraction over the planar
// channel index cc = 2*ci + ri with the block weight [[Wr,-Wi],[Wi,Wr]] (rows m = 2*co + ro),
// built once by pack.hip; eval-mode ComplexBatchNormal (complex_progress.py:161-209) is
// folded into W'/bias there, PReLU (pvae_module.py:58,82) runs in the epilogue, and in train
// mode the epilogue emits the five per-channel moments the batch statistics need.
// The same kernel in PW mode (1x1, k-pairs = plane pairs) is the LSTM input projection,
// ComplexDense (complex_progress.py:77-89), and the DFT / inverse-DFT of STFT / ISTFT.
//
// MFMA: v_mfma_f32_32x32x2_f32 (exact fp32).  The two k of one instruction are the two time
// taps (kt = 0,1) of one (cc, kf): lanes 0-31 read patch column j, lanes 32-63 column j+1 of
// the SAME LDS row, so the im2col expansion costs nothing and is bank-conflict free.
// Weights stream from L2 in pre-swizzled fragment order (one coalesced 256 B load per
// fragment, no LDS); the input patch (CCK planes x FR rows x JT+2 columns) is staged
// global -> registers -> LDS, double buffered, one barrier per K chunk.
#pragma once
#include "common.hpp"

#ifndef IDV_WAVES_PER_SIMD
#define IDV_WAVES_PER_SIMD 1
#endif

enum { IDV_CONV = 0, IDV_TCONV = 1, IDV_PW = 2 };

struct CgemmArgs {
    const float* x0;      // first source, planar [2][C0][Fin][Jp] (PW: K planes of stride Jp)
    const float* x1;      // optional second source (skip connection), planar [2][C1][Fin][Jp1]
    int C0, C1;           // complex channels taken from x0 / x1 (PW: C0 = K/2, C1 = 0)
    int Fin, Fout;        // input / output rows (PW: 1 / 1)
    int J, Jp, Tp;        // columns, row stride, columns per utterance
    int Jp1, x1_div;      // x1 row stride; x1 column j maps to utterance (b / x1_div)
    const float* wfrag;   // [Mtiles][KS][64] fragment-ordered weights
    const float* bias;    // [Mtiles*32]
    const float* slope;   // PReLU slope (device scalar) or nullptr
    float* out;           // planar [M planes][Fout][Jp] or, SWAP, row-major [pos][ldo]
    int M;                // valid rows
    int Mtiles;           // allocated 32-row tiles in wfrag (multiple of the block's tiles)
    int cplx_rows;        // 1: row m = 2*co + ro -> plane ro*Cout + co ; 0: plane = m
    int Cout;
    int tshift;           // -1: taps (x[t-1], x[t])   0: taps (x[t], x[t+1])
    int t_valid;          // outputs at tp in [1, t_valid] are kept, everything else is zero
    double* stats;        // train mode: [Cout][5] sums (r, i, rr, ii, ri) or nullptr
    int stats_rep;        // > 1: stats holds that many replicas [rep][Cout][5] (power of two), one chosen per workgroup
    int ldo;              // SWAP: row stride of out; rows are ordered (tp-1)*B + b
    int nB;               // SWAP: utterances (B)
    int jtiles, ftiles, mblocks;   // grid decomposition (filled by the launcher)
    int map_ft;                    // 1: an XCD takes ALL frequency tiles of its column blocks (they share halo rows in L2)
    // split-bf16 image sources / destination (cgemm_bf16.hip, cgemm_c1.hip); x0 / x1 then point at image data
    long long lo_off0, lo_off1;    // hi -> lo plane distance of the x0 / x1 image, in 16-byte slots
    void* out_img;                 // optional image destination (besides or instead of `out`)
    long long out_lo_off;          // its hi -> lo distance, in bf16 elements
};
// 16-byte slot, relative to the start of an image plane, that every producer of an image zeroes (both planes):
// consumers read it for frequency rows outside [0, Fin)
#define IDV_IMG_ZSLOT (-8)

typedef __bf16 idv_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned idv_pack_bf16(float a, float b) {      // round-to-nearest-even pair
    idv_bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, v);
}

template <int MODE, int FO_T>
struct CgemmGeom {
    static constexpr int KF = (MODE == IDV_PW) ? 1 : 5;
    static constexpr int FR = (MODE == IDV_CONV) ? 2 * FO_T + 3 : (MODE == IDV_TCONV ? FO_T + 2 : 1);
    static constexpr int ROWS = (MODE == IDV_TCONV) ? 2 * FO_T : FO_T;   // output row tiles per j chunk
};

// Column maps.  The columns j of a tile are VIRTUAL columns v in [0, a.J); a map says which input column of the planar layout a
// virtual column reads, which output position (utterance b, column tp) it is, and how a SWAP result is stored.
struct CgemmFlatCols {                       // v = b * Tp + tp: the planar layout itself (every launch of cgemm_kernel)
    static constexpr bool FLAT = true;
    __device__ __forceinline__ int in_col(const CgemmArgs&, int v) const { return v; }
    __device__ __forceinline__ void out_pos(const CgemmArgs& a, int v, int& b, int& tp) const {
        b = v / a.Tp;
        tp = v - b * a.Tp;
    }
    __device__ __forceinline__ void store(float* p, float y) const { *p = y; }
};
// PW + SWAP only: the columns of a TIME CHUNK, steps [t0, t0 + steps) of every utterance, utterance-major: v = b * steps + (t - t0)
// (lstm_proj_split.hpp).  The output rows (t * B + b) of a chunk are contiguous; they are stored write-through (sc1), for
// consumers inside the same launch (lstm_stack2_f32.hip).
struct CgemmTimeChunkCols {
    static constexpr bool FLAT = false;
    int t0, steps;
    __device__ __forceinline__ int in_col(const CgemmArgs& a, int v) const {
        const int b = v / steps;
        return b * a.Tp + 1 + t0 + (v - b * steps);
    }
    __device__ __forceinline__ void out_pos(const CgemmArgs&, int v, int& b, int& tp) const {
        b = v / steps;
        tp = 1 + t0 + (v - b * steps);
    }
    __device__ __forceinline__ void store(float* p, float y) const { __hip_atomic_store(p, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// One workgroup tile: column block jt, frequency tile ft, row-tile block mblk; smem: 2 patch buffers.  Called by every thread of
// a workgroup of WM * WN waves (it contains barriers); may be called again with the same smem once it has returned.
template <int MODE, int WM, int WN, int MT_W, int FO_T, int JC_W, int CCK, bool SWAP, bool STATS, bool VEC, class CM>
__device__ __forceinline__ void cgemm_tile(const CgemmArgs& a, float* smem, const int jt, const int ft, const int mblk, const CM cm) {
#define CGEMM_BODY_TILE_GIVEN
#include "cgemm_body.hpp"
#undef CGEMM_BODY_TILE_GIVEN
}

// WM x WN waves; each wave owns MT_W row tiles (32 rows) and ROWS*JC_W column tiles (32 cols).
template <int MODE, int WM, int WN, int MT_W, int FO_T, int JC_W, int CCK, bool SWAP, bool STATS, bool VEC>
__global__ __launch_bounds__(WM* WN * 64, IDV_WAVES_PER_SIMD) void cgemm_kernel(const CgemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using CM = CgemmFlatCols;
    const CM cm{};
#include "cgemm_body.hpp"
}
