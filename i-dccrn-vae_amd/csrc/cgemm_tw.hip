// cgemm_tw: the complex ConvTranspose2d contraction of cgemm_wino.hip (three real products per complex product, frequency taps in
// Winograd form) with the TIME taps in Winograd form too: F(2,2) over pairs of output columns.
//
// The decoder block's kernel has two time taps (model/complex_progress.py:222-279: kernel (5, 2), causal).  cgemm / cgemm_gauss /
// cgemm_wino apply them with ONE v_mfma_f32_32x32x2_f32 whose two k are the two taps:  out[j] = Wa x[j + s] + Wb x[j + 1 + s]
// (s = tshift).  For the column pair (2c, 2c + 1) with  a = x[2c + s], b = x[2c + 1 + s], d = x[2c + 2 + s]:
//     m1 = Wa (a - b)      m2 = (Wa + Wb) b      m3 = Wb (b - d)          out[2c] = m1 + m2       out[2c + 1] = m2 - m3
// -- three products for two columns instead of four: the two k of an MFMA become two INPUT CHANNELS, and a (32 channels x 32
// column pairs) tile costs 3 MFMAs per channel pair where the 2-tap form costs 4 (2 column tiles x 2 channels).  On top of
// cgemm_wino's 7 / 10 frequency products and the three Gauss products: 3/4 x 7/10 x 3/4 = 0.39 of the reference's real products.
// All transform factors are +-1 (and the 1/2 of the frequency taps): exact in fp32 up to the rounding of the sums.
//
// Tiles.  One accumulator tile per (frequency product r, Gauss plane g, time product tau): the even-row phase (PH 0) has 4 x 3 x 3
// = 36 tiles, the odd-row phase (PH 1) 3 x 3 x 3 = 27, for ONE tile of 32 complex output channels x 64 columns x one pair of input
// rows.  No two tiles share an operand (each has its own transformed taps and its own transformed input row), so the tiles are
// dealt to the four waves of a workgroup (tw_tile: even rows wave = r with its nine planes; odd rows waves 0 .. 2 = r with planes
// 0 .. 5 and 8, wave 3 the planes 6, 7 of all three r: 9 / 7 tiles per wave, two workgroups per CU) and the output transforms (time,
// Gauss, frequency) run in the epilogue on tiles exchanged through the LDS.
// Staging writes the RAW input rows, each as nine planes (s = r + i | r | i) x (a - b | b | b - d) of 32 column pairs, planes (2 p,
// 2 p + 1) interleaved per pair (one 8-byte read fetches the operands of two tiles); the FREQUENCY transform A + cb B of cgemm_wino
// happens at the operand read (two reads + one add).  Weights: cgemm_wino's fragments re-ordered by idv_pack_cconv_tw (lane =
// channel parity x 32 + co), per (channel pair, wave).  Design notes and measurements: DESIGN.md 3.1e.
//
// Odd row counts (every decoder layer of the model): the last even output row, out[2 (Fin - 1)] = W4 x[Fin - 2] + W2 x[Fin - 1], has no
// partner row.  It is not a row tile of its own: the even-row launch holds EDGE workgroups (cgemm_tw_map.hpp) that compute that row
// for TWO adjacent column blocks, wave w the raw-tap product (column block w >> 1, tap W4 | W2 = w & 1) on raw row Fin - 2 + (w & 1)
// -- the same K loop on other offsets and a third weight region, and out = P[2 c] + P[2 c + 1] in the epilogue.
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include "cgemm.hpp"
#include "conv_epilogue.hpp"
#include "cgemm_tw_map.hpp"
#include "cgemm_tw_stage.hpp"
#include "../../include/idccrn_hip.h"

namespace {

// LDS operand reads through address-space pointers: base register + compile-time offset in the read's immediate
typedef __attribute__((address_space(3))) float LdsF;
typedef float TwF2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) TwF2 LdsF2;

struct TwArgs {
    const float* x0;      // planar [2][C0][Fin][Jp]
    const float* x1;      // optional skip source, planar [2][C1][Fin][Jp] (same pitch)
    int C0, C1;
    int Fin, Fout;
    int J, Jp, Tp;
    const float* wfrag;   // [phase 0: cotiles][UP][4 waves x 9 slots][64], [phase 1: cotiles][UP][4 x 8][64], then the raw taps of the
                          // edge workgroups [cotiles][UP][4 waves x 9 slots][64] (waves 0, 2: W4; 1, 3: W2) (idv_pack_cconv_tw)
    int UP;               // channel pairs per co tile as packed (Cin rounded up to the pack granularity, / 2)
    const float* epi;     // as cgemm_gauss: [cotiles * 32][8]
    int has_fold;
    const float* slope;
    float* out;           // planar [2][Cout][Fout][Jp]
    int Cout, cotiles;
    int tshift, t_valid;
    double* stats;        // train mode: [Cout][5] sums (r, i, rr, ii, ri) of the outputs, or nullptr (as cgemm_gauss)
    int stats_rep;        // > 1: that many replicas [rep][Cout][5] (power of two), one chosen per workgroup
    const float* add;     // optional addend (see cgemm_gauss.hip)
    int add_div, add_Jp;
    TwGrid grid;          // block order (cgemm_tw_map.hpp); cgroups = cotiles / NCT workgroups per (column block, row pair)
    int stagger;          // NCT = 2, odd-row phase: waves 4 .. 7 stage one k-step later than their SIMD partners, waves 0 .. 3
};

constexpr int TW_PACK_CI = 8;      // pack granularity in complex input channels (cgemm_wino's WCIK)
// co tiles on different XCDs: dec0-3 at B = 64 34.7 -> 34.3 ms (dec0, eight co tiles: 9.81 -> 9.54) against one XCD per column block
constexpr int TW_XCD_SPLIT = 1;
// two co tiles per workgroup, odd-row phase: waves 4 .. 7 stage one k-step later than their SIMD partners (see the kernel's main loop)
constexpr int TW_PAIR_STAGGER = 1;

// frequency transforms: cgemm_wino.hip's tables (transformed row r = raw row ra + cb * raw row rb of d0..d3 = input rows m0 - 1 .. m0 + 2)
template <int PH> __device__ __forceinline__ int tw_ra(int r) {
    if (PH == 0) return r == 0 ? 0 : (r == 2 ? 2 : 1);
    return r == 0 ? 1 : 2;
}
template <int PH> __device__ __forceinline__ int tw_rb(int r) {
    if (PH == 0) return r == 2 ? 1 : (r == 3 ? 3 : 2);
    return r == 0 ? 2 : 3;
}
template <int PH> __device__ __forceinline__ float tw_cb(int r) {
    if (PH == 0) return r == 1 ? 1.f : -1.f;
    return r == 1 ? 0.f : -1.f;
}
template <int PH> constexpr int tw_nr() { return PH == 0 ? 4 : 3; }
template <int PH> constexpr int tw_nt() { return tw_nr<PH>() * 9; }            // tiles (r, g, tau): t = r * 9 + g * 3 + tau
template <int PH> constexpr int tw_ntp() { return PH == 0 ? 36 : 32; }         // weight slots per channel pair: 4 waves x 9 / 8
template <int PH> constexpr int tw_ntw() { return (tw_nt<PH>() + 3) / 4; }     // tiles per wave: 9 / 7
// tile k of wave w: t = r * 9 + plane, or -1 (the odd-row phase's 28th slot: zero taps, never read).  Tiles come as NPAIR pairs of
// planes (2 p, 2 p + 1) of ONE frequency product + one single tile (plane 8): even-row phase, wave = r: all nine planes of r.
// Odd-row phase: waves 0 .. 2 = r: planes 0 .. 5 and 8; wave 3: planes 6, 7 of r = 0, 1, 2.
__host__ __device__ inline int tw_tile(int ph, int w, int k) {
    if (ph == 0) return w * 9 + k;
    if (w < 3) return k < 6 ? w * 9 + k : w * 9 + 8;
    return k < 6 ? (k >> 1) * 9 + 6 + (k & 1) : -1;
}
template <int PH> constexpr int tw_wslots() { return PH == 0 ? 9 : 8; }        // packed weight slots per (channel pair, wave)

// LEFT: the time taps read (x[t-1], x[t]) (tshift = -1: the extra window column is on the left), else (x[t], x[t+1])
// NCT: co tiles per workgroup.  2: eight waves; waves 0 .. 3 run the program of co tile 2 p, waves 4 .. 7 the same program on co tile
// 2 p + 1 (tiles, weights, K order and epilogue of a co tile are those of NCT = 1: the results are bit-identical), and all 512 threads
// share ONE staging of the raw rows, which do not depend on the output channel: half the staging work and input fetch per MFMA.  One
// workgroup per CU, still two waves per SIMD.
template <int PH, int CIK, bool LEFT, bool STATS = false, int NCT = 1>
__global__ __launch_bounds__(256 * NCT, NCT == 1 ? 2 : 1) void cconv_tw_kernel(const TwArgs a) {
    constexpr int NR = tw_nr<PH>(), NT = tw_nt<PH>(), NTP = tw_ntp<PH>(), NTW = tw_ntw<PH>();
    constexpr int NRAW = PH == 0 ? 4 : 3, ROW0 = PH == 0 ? 0 : 1;       // raw patch rows d(ROW0) .. : input rows m0 - 1 + ROW0 ..
    constexpr int KS = CIK / 2;                  // MFMA k-steps (channel pairs) per chunk
    constexpr int RT = NRAW * 9 * 32;            // floats per channel in a patch buffer: per raw row 9 (Gauss, time) planes of 32 pairs
    constexpr int NE = CIK * RT;
    constexpr int NBUF = 2;
    constexpr int RDW = 2;                       // weight ring depth in k-steps
    // A wave's loads return in order, so the first wait for weights fetched AFTER a staging load also waits for the staging load.
    // Even-row phase with two co tiles: an item's loads go behind the weight loads of their k-step instead of in front of them, and
    // the wait that retires them comes a k-step later (10 -> 18 MFMAs after issue; dec0-3 at B = 64: -0.5 .. -0.8 ms on two cards
    // of three, nothing on the third).  Measured to gain nothing: the same in the other three forms (the odd-row phase again behind
    // its two 16-byte weight loads: 7 -> 14 / 9 MFMAs paired, 7 -> 10 .. 14 unpaired, no faster), and a ring of KS k-steps on top of
    // it here.
    constexpr bool STAGE_BEHIND_W = PH == 0 && NCT == 2;
    // The K loop's address forms (operand reads on per-lane LDS bases + compile-time offsets with the transform one MFMA ahead;
    // staging loads on a scalar base + 32-bit byte offset) in every form but the unpaired odd-row kernel, which keeps the forms it
    // had: its loop is laid out as three copies (28, 20 and 13 MFMAs: the waves with two, one and no second staging item) whose
    // staging-load distances tests/test_tw_odd_wvec_host.py keeps, and with either new form the compiler lays out one
    constexpr bool KBASE = !(PH == 1 && NCT == 1);
    constexpr int NITEM = CIK * NRAW * 16;       // staging items per chunk: (channel, raw row, 2 column pairs)
    constexpr int NTHR = 256 * NCT;
    constexpr int NLD = (NITEM + NTHR - 1) / NTHR;
    static_assert(NCT == 1 || NCT == 2, "one or two co tiles per workgroup");
    static_assert(KS % RDW == 0 && NLD <= 2, "weight ring slots are compile-time; at most two staging items per thread");
    static_assert(NLD + NCT - 1 < KS, "the staging k-steps (from 1 on, waves 4 .. 7 one later) end before the barrier's k-step");
    static_assert(NCT * NT * 4 * 64 <= NBUF * NE, "the epilogue exchange (one area per co tile) fits the patch buffers");

    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the wave's place in its co tile's program; which co tile of the workgroup
    const int w4 = NCT == 1 ? wave : wave & 3, cth = NCT == 1 ? 0 : wave >> 2;
    const int half = lane >> 5, l31 = lane & 31;

    // block order: cgemm_tw_map.hpp.  An EDGE workgroup (even-row phase, odd row count; block-uniform) computes the last even output
    // row of the column blocks jt, jt + 1
    TwTile tile;
    if (!tw_block_tile(a.grid, blockIdx.x, tile)) return;
    const bool edge = PH == 0 && tile.edge;
    const int jt = tile.jt, ft = tile.ft;
    int ct = tile.ct;
    ct = NCT * ct + cth;                          // (ct was the workgroup's group of NCT co tiles)
    const int j0 = jt * 64;
    const int m0 = 2 * ft;
    const int rbase = m0 - 1 + ROW0;

    const int Cin = a.C0 + a.C1;
    const int nchunk = (Cin + CIK - 1) / CIK;

    f32x16 acc[NTW];
#pragma unroll
    for (int k = 0; k < NTW; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
    // this wave's tiles (tw_tile): NPAIR pairs of planes + one single; slot j of the wave reads raw rows ra(r_j), rb(r_j) at plane pair
    // pj_j -- the frequency transform  A + cb B  happens at the operand read.  An edge workgroup's wave reads ONE raw slot, its own
    // (A = B, cb = 0).
    constexpr int NPAIR = (NTW - 1) / 2;
    constexpr bool UNI = PH == 0;             // every slot of the wave belongs to ONE frequency product: one row offset, constant plane offsets
    int offA[UNI ? 1 : NPAIR + 1], offB[UNI ? 1 : NPAIR + 1];
    float cbj[UNI ? 1 : NPAIR + 1];
    if (UNI) {
        cbj[0] = edge ? 0.f : tw_cb<PH>(w4);
        offA[0] = (edge ? w4 : tw_ra<PH>(w4) - ROW0) * 288;
        offB[0] = (edge ? w4 : tw_rb<PH>(w4) - ROW0) * 288; // (cb is never 0 in a full tile of this phase)
    } else {
#pragma unroll
        for (int j = 0; j <= NPAIR; ++j) {
            int t = tw_tile(PH, w4, j < NPAIR ? 2 * j : NTW - 1);
            t = t < 0 ? 0 : t;
            const int r = t / 9, plane = t - r * 9;
            cbj[j] = tw_cb<PH>(r);
            const int po = plane == 8 ? 256 : (plane >> 1) * 64;
            offA[j] = (tw_ra<PH>(r) - ROW0) * 288 + po;
            offB[j] = cbj[j] != 0.f ? (tw_rb<PH>(r) - ROW0) * 288 + po : offA[j];
        }
    }

    // ---- staging: one item = channel cl, raw row, column pairs 2 c8, 2 c8 + 1 (output columns j0 + 4 c8 .. + 3): window columns
    // w0..w4 = input columns jc + tshift .. jc + 4 + tshift, real and imaginary -> the 9 planes (s = r + i | r | i) x (a - b | b | b - d).
    // Edge workgroup: raw slot rl holds (column block jt + (rl >> 1), row Fin - 2 + (rl & 1)); a second column block past J is masked
    // like any column out of range.
    f32x4 v_r[NLD], v_i[NLD];
    float e_r[NLD], e_i[NLD];
    unsigned off_v[NLD], off_e[NLD], ldsoff[NLD];
    unsigned okmask[NLD];     // bits 0-4: window column valid; bit 5: row valid; bit 7: item exists
    int item_cl[NLD];
    bool interior[NLD];       // wave-uniform: every lane's item has its row and all five window columns inside the tensor
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        // the address function: cgemm_tw_stage.hpp.  BYTE offsets from the chunk's wave-uniform row bases: the loads take the scalar
        // base + 32-bit lane offset form, no 64-bit address arithmetic per lane (KBASE = false, the unpaired odd-row kernel: float
        // offsets, see the main loop)
        const TwStageItem it = tw_stage_item(tid + i * NTHR, NRAW, NITEM, LEFT, edge, a.Fin, a.J, a.Jp, j0, rbase, KBASE ? 4u : 1u);
        item_cl[i] = it.cl;
        off_v[i] = it.off_v;
        off_e[i] = it.off_e;
        okmask[i] = it.mask;
        interior[i] = __builtin_amdgcn_ballot_w64((it.mask & 0xbfu) == 0xbfu) == ~0ull;
        ldsoff[i] = it.ldsoff;
    }
    auto stage_load = [&](int chunk, int i) {
        const int ci0 = chunk * CIK;
        const bool from0 = ci0 < a.C0;
        const float* br = from0 ? a.x0 + (size_t)ci0 * a.Fin * a.Jp : a.x1 + (size_t)(ci0 - a.C0) * a.Fin * a.Jp;
        const float* bi = from0 ? br + (size_t)a.C0 * a.Fin * a.Jp : br + (size_t)a.C1 * a.Fin * a.Jp;
        const int cvalid = (from0 ? a.C0 : Cin) - ci0;
        const bool dead = item_cl[i] >= cvalid;
        const unsigned ov = dead ? 4u * TW_DUMMY : off_v[i], oe = dead ? 4u * TW_DUMMY : off_e[i];
        if constexpr (KBASE) {
            v_r[i] = *(const f32x4*)((const char*)br + ov);
            v_i[i] = *(const f32x4*)((const char*)bi + ov);
            e_r[i] = *(const float*)((const char*)br + oe);
            e_i[i] = *(const float*)((const char*)bi + oe);
        } else {
            v_r[i] = *(const f32x4*)(br + ov);
            v_i[i] = *(const f32x4*)(bi + ov);
            e_r[i] = br[oe];
            e_i[i] = bi[oe];
        }
    };
    // the store of an item in ten steps that the main loop deals out between MFMAs (step 0: masks and the window of five columns;
    // steps 1 .. 9: one (Gauss, time) plane each), so that the vector ALU work hides behind the matrix pipe
    float fr[5], fi[5];
    auto stage_window = [&](int chunk, int i) {
        const int ci0s = chunk * CIK;
        const int cvalid = (ci0s < a.C0 ? a.C0 : Cin) - ci0s;
        constexpr bool left = LEFT;
        if (interior[i] && cvalid >= CIK) {                   // (uniform) nothing to mask
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                fr[q] = left ? (q == 0 ? e_r[i] : v_r[i][q == 0 ? 0 : q - 1]) : (q == 4 ? e_r[i] : v_r[i][q == 4 ? 3 : q]);
                fi[q] = left ? (q == 0 ? e_i[i] : v_i[i][q == 0 ? 0 : q - 1]) : (q == 4 ? e_i[i] : v_i[i][q == 4 ? 3 : q]);
            }
            return;
        }
        unsigned m = okmask[i];
        if (item_cl[i] >= cvalid || !((m >> 5) & 1u)) m &= ~0x1fu;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            // window column q: the extra column is w0 (taps to the left) or w4; compile-time vector indices on either side
            const float xr = left ? (q == 0 ? e_r[i] : v_r[i][q == 0 ? 0 : q - 1]) : (q == 4 ? e_r[i] : v_r[i][q == 4 ? 3 : q]);
            const float xi = left ? (q == 0 ? e_i[i] : v_i[i][q == 0 ? 0 : q - 1]) : (q == 4 ? e_i[i] : v_i[i][q == 4 ? 3 : q]);
            const bool cok = (m >> q) & 1u;
            fr[q] = cok ? xr : 0.f;
            fi[q] = cok ? xi : 0.f;
        }
    };
    auto plane_val = [&](int gt, int pr) -> float {           // plane gt = g * 3 + tau of column pair pr (0 / 1) of the item
        const int g = gt / 3, tau = gt - g * 3;
        // pair 0: (a, b, d) = window columns 0, 1, 2; pair 1: 2, 3, 4
        const int q0 = 2 * pr;
        const float xa_ = g == 0 ? fr[q0] + fi[q0] : (g == 1 ? fr[q0] : fi[q0]);
        const float xb_ = g == 0 ? fr[q0 + 1] + fi[q0 + 1] : (g == 1 ? fr[q0 + 1] : fi[q0 + 1]);
        const float xd_ = g == 0 ? fr[q0 + 2] + fi[q0 + 2] : (g == 1 ? fr[q0 + 2] : fi[q0 + 2]);
        return tau == 0 ? xa_ - xb_ : (tau == 1 ? xb_ : xb_ - xd_);
    };
    // an item exists for every thread in the even-row phase (512 items); in the odd-row phase (384) the second item only in waves 0, 1
    // (NCT = 2: the one item in waves 0 .. 5)
    auto item_exists = [&](int i) -> bool { return NITEM >= (i + 1) * NTHR || wave * 64 + i * NTHR < NITEM; };
    // LDS layout of a raw row: planes (2 j, 2 j + 1) interleaved per column pair at [j][32 pairs][2], plane 8 at [256 + pair]:
    // a lane fetches the operands of two tiles with one 8-byte read, an item writes two planes x two pairs with one 16-byte write
    auto stage_plane2 = [&](float* dst, int i, int j) {
        if (!item_exists(i)) return;                          // (uniform)
        if (j < 4) {
            f32x4 o = {plane_val(2 * j, 0), plane_val(2 * j + 1, 0), plane_val(2 * j, 1), plane_val(2 * j + 1, 1)};
            *(f32x4*)(dst + ldsoff[i] + j * 64) = o;
        } else {
            *(float2*)(dst + ldsoff[i] - 2 * (int)(tid & 15) + 256) = make_float2(plane_val(8, 0), plane_val(8, 1));
        }
    };
    auto stage_store = [&](float* dst, int chunk, int i) {
        stage_window(chunk, i);
#pragma unroll
        for (int j = 0; j < 5; ++j) stage_plane2(dst, i, j);
    };

    // ---- weights in a ring of RDW k-steps: the wave's tiles of a channel pair are packed as groups of [64 lanes][4 tiles] (lane =
    // channel parity x 32 + co; idv_pack_cconv_tw): even-row phase two 16-byte loads + one 4-byte load ([64 lanes]) per k-step,
    // odd-row phase two 16-byte loads.  The odd-row phase's eighth slot (zero taps, no tile) has a register of its own in the ring:
    // see the main loop.
    constexpr int WS = tw_wslots<PH>();
    constexpr int NWR = PH == 0 ? NTW : 8;                    // weight registers per ring slot
    const size_t wregion = PH == 1 ? (size_t)a.cotiles * a.UP * tw_ntp<0>() : (edge ? (size_t)a.cotiles * a.UP * (tw_ntp<0>() + tw_ntp<1>()) : 0);
    const float* wbase = a.wfrag + (wregion + (size_t)ct * a.UP * NTP) * 64 + (size_t)w4 * WS * 64;
    const int total_ks = nchunk * KS;
    float a_w[RDW][NWR];
    auto load_w = [&](int g, float (&dst)[NWR]) {
        g = g < total_ks ? g : total_ks - 1;                  // (past the end of K: an unused re-fetch)
        const float* ws = wbase + (size_t)g * NTP * 64;
        const f32x4 w0 = *(const f32x4*)(ws + lane * 4), w1 = *(const f32x4*)(ws + 256 + lane * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dst[k] = w0[k];
            dst[4 + k] = w1[k];
        }
        if (NTW == 9) dst[NTW - 1] = ws[512 + lane];
    };
    float xa[NTW], xb[NTW];
    // The wave's operand addresses, formed ONCE per lane: the LDS address of its first k-step's operand in the buffer the loop reads
    // (buffer + this half-wave's channel + row / plane offset + the lane's column pair).  Even-row phase: one pair of bases for the
    // plane pairs (8-byte reads at 2 l31) and one for plane 8 (4-byte reads at l31); odd-row phase: one pair per slot.  The k-step and
    // the plane pair are compile-time offsets of the reads, and the bases move to the other buffer once per chunk (flip_bases).
    constexpr int NBASE = UNI ? 2 : NPAIR + 1;
    const LdsF* pA[NBASE];
    const LdsF* pB[NBASE];
    {
        const LdsF* s0 = (const LdsF*)smem + half * RT;
#pragma unroll
        for (int j = 0; j < NBASE; ++j) {
            const bool single = j == NBASE - 1;
            const int lp = single ? (UNI ? 256 : 0) + l31 : 2 * l31;
            pA[j] = s0 + offA[UNI ? 0 : j] + lp;
            pB[j] = s0 + offB[UNI ? 0 : j] + lp;
        }
    }
    // the largest base + compile-time offset stays inside the two patch buffers: second buffer, odd channel of the last k-step, last
    // raw row, plane 8, last pair
    static_assert(NE + (2 * (KS - 1) + 1) * RT + (NRAW - 1) * 288 + 256 + 31 < NBUF * NE, "operand reads stay inside the LDS allocation");
    static_assert(((2 * (KS - 1)) * RT + (NPAIR - 1) * 64) * 4 < 65536, "k-step and plane-pair offsets fit the LDS read's immediate");
    static_assert(NBUF == 2, "the bases alternate between two buffers");
    int flip = NE;                                // (uniform) to the other buffer: + NE, then - NE, ...
    auto flip_bases = [&]() {
#pragma unroll
        for (int j = 0; j < NBASE; ++j) {
            pA[j] += flip;
            pB[j] += flip;
        }
        flip = -flip;
    };
    // operands of tiles 2 j, 2 j + 1 (j < NPAIR: one 8-byte read per raw row) or of the single tile, at KOFF floats (compile time: the
    // k-step's channel pair) from the bases
    auto load_raw2 = [&](int koff, int j) {
        if (j < NPAIR) {
            const int po = koff + (UNI ? j * 64 : 0);
            const TwF2 pa_ = *(const LdsF2*)(pA[UNI ? 0 : j] + po), pb_ = *(const LdsF2*)(pB[UNI ? 0 : j] + po);
            xa[2 * j] = pa_.x; xa[2 * j + 1] = pa_.y;
            xb[2 * j] = pb_.x; xb[2 * j + 1] = pb_.y;
        } else {
            xa[NTW - 1] = pA[NBASE - 1][koff];
            xb[NTW - 1] = pB[NBASE - 1][koff];
        }
    };
    // KBASE = false (the unpaired odd-row kernel, see the main loop): the reads at base = buffer + channel of this half-wave
    auto load_raw2_p = [&](const float* base, int j) {
        if (j < NPAIR) {
            const int oa = UNI ? offA[0] + j * 64 : offA[UNI ? 0 : j], ob = UNI ? offB[0] + j * 64 : offB[UNI ? 0 : j];
            const float2 pa_ = *(const float2*)(base + oa + 2 * l31), pb_ = *(const float2*)(base + ob + 2 * l31);
            xa[2 * j] = pa_.x; xa[2 * j + 1] = pa_.y;
            xb[2 * j] = pb_.x; xb[2 * j + 1] = pb_.y;
        } else {
            xa[NTW - 1] = base[(UNI ? offA[0] + 256 : offA[UNI ? 0 : NPAIR]) + l31];
            xb[NTW - 1] = base[(UNI ? offB[0] + 256 : offB[UNI ? 0 : NPAIR]) + l31];
        }
    };
    auto load_raw_all = [&]() {
#pragma unroll
        for (int j = 0; j <= NPAIR; ++j) {
            if constexpr (KBASE) load_raw2(0, j);
            else load_raw2_p(smem + (size_t)half * RT, j);
        }
    };
    // the frequency transform of tile k's operand
    auto xform = [&](int k) -> float { return xa[k] + cbj[UNI ? 0 : (k >> 1 < NPAIR ? k >> 1 : NPAIR)] * xb[k]; };

#pragma unroll
    for (int i = 0; i < NLD; ++i) stage_load(0, i);
#pragma unroll
    for (int u = 0; u < RDW; ++u) load_w(u, a_w[u]);
#pragma unroll
    for (int i = 0; i < NLD; ++i) stage_store(smem, 0, i);
#pragma unroll
    for (int i = 0; i < NLD; ++i) stage_load(nchunk > 1 ? 1 : 0, i);
    __syncthreads();

    load_raw_all();
    // the transform runs ONE MFMA ahead of its product: a transform right in front of the MFMA that reads it costs the wait states of
    // the vector-ALU-write -> MFMA-read hazard at every second MFMA
    float bcur = KBASE ? xform(0) : 0.f;
    // the main loop; late_ (NCT = 2, odd-row phase only): the copy that stages one k-step later, for waves 4 .. 7, so that SIMD partners
    // do not stage at the same time.  A copy, not a branch on the wave inside the loop: the staging steps sit between the MFMAs, and
    // with a wave-uniform branch at each of them the paired kernels were SLOWER than the unpaired ones (dec0-3, B = 64: 36.4 against
    // 34.2 ms; in this form 33.0).  The even-row phase has no late copy: a second copy of its loop spills 60 - 72 bytes per lane.
    auto run = [&](auto late_) {
        constexpr bool LATE = decltype(late_)::value;
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            const float* P = smem + (chunk & 1) * NE;
            float* Pn = smem + ((chunk + 1) & 1) * NE;
            const int nxt = chunk + 1 < nchunk ? chunk + 1 : chunk, nxt2 = chunk + 2 < nchunk ? chunk + 2 : nchunk - 1;
#pragma unroll
            for (int ul = 0; ul < KS; ++ul) {
                // operands of the next k-step: of this chunk, or (last k-step, after the barrier below, which moves the bases) of the
                // next chunk
                const int bnext = ul + 1 < KS ? 2 * (ul + 1) * RT : 0;
                const float* bnext_p = ul + 1 < KS ? P + (size_t)(2 * (ul + 1) + half) * RT : Pn + (size_t)half * RT;
                auto load_next = [&](int j) {
                    if constexpr (KBASE) load_raw2(bnext, j);
                    else load_raw2_p(bnext_p, j);
                };
                // staging of chunk + 1 rides on k-steps 1 (item 0) and 2 (item 1): the item's registers were loaded one chunk ago, the
                // other buffer was last read in the previous chunk (a barrier since); the steps of the store are dealt out between MFMAs
                const int si = ul - 1 - (LATE ? 1 : 0);
                const bool staging = si >= 0 && si < NLD;
#pragma unroll
                for (int k = 0; k < NTW; ++k) {
                    // (tile 0 of the next k-step: its operands were read behind MFMA 1 of this one)
                    float bn = 0.f;
                    if constexpr (KBASE) {
                        bn = xform(k + 1 < NTW ? k + 1 : 0);
                        // (odd-row phase: without this the compiler sinks the transform back in front of its product; the even-row
                        // phase keeps it here by itself, and its unpaired kernel pays 15 more vector instructions per chunk for the
                        // statement)
                        if (PH == 1) asm volatile("" : "+v"(bn));
                        __builtin_amdgcn_sched_barrier(0);    // (in FRONT of MFMA k: behind it, it would sit right in front of MFMA k + 1)
                    } else {
                        bcur = xform(k);
                    }
                    // Odd-row phase: no wave reads the eighth slot's weights (seven tiles).  Left dead, that register is handed out again
                    // while the second group's 16-byte load is still in flight, and the write to it waits for ALL the wave's loads
                    // (vmcnt(0)) right behind the load's issue, in every k-step (that form measured 14.1 -> 17.8 ms on dec0-3 at B = 64).
                    // Read here, where the group's first MFMA waits for the load anyway, it stays the load's until it has landed.
                    if (PH == 1 && k == 4)
                        asm volatile("" ::"v"(a_w[ul % RDW][4]), "v"(a_w[ul % RDW][5]), "v"(a_w[ul % RDW][6]), "v"(a_w[ul % RDW][7]));
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_w[ul % RDW][k], bcur, acc[k], 0, 0, 0);
                    if constexpr (KBASE) bcur = bn;
                    if (ul == KS - 1 && k == 0) {
                        // every wave has stored chunk + 1 (k-steps 1, 2) and issued its last reads of P: after this barrier Pn is complete
                        // and P may be overwritten (from k-step 1 of the next chunk on)
                        __builtin_amdgcn_sched_barrier(0);
                        __syncthreads();
                        if constexpr (KBASE) flip_bases();    // the one address update of the chunk: every read from here on is of Pn
                    }
                    // the operand registers of the tiles done so far are free again
                    if ((k & 1) && (k >> 1) < NPAIR) load_next(k >> 1);
                    if (k == NTW - 1) load_next(NPAIR);
                    if (staging) {
                        // the store's steps between the MFMAs: window at 0, plane pairs at 1, 3, 5 and (7 or, with seven tiles, 6), plane 8 last
                        if (k == 0) stage_window(nxt, si);
                        if ((k & 1) && k < 6) stage_plane2(Pn, si, k >> 1);
                        if (k == (NTW == 9 ? 7 : 6)) stage_plane2(Pn, si, 3);
                        if (k == NTW - 1) stage_plane2(Pn, si, 4);
                        if (k == NTW - 1 && !STAGE_BEHIND_W) stage_load(nxt2, si);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                load_w(chunk * KS + ul + RDW, a_w[ul % RDW]);
                if (STAGE_BEHIND_W && staging) {
                    __builtin_amdgcn_sched_barrier(0);
                    stage_load(nxt2, si);
                }
            }
        }
    };
    if (NCT == 2 && PH == 1 && a.stagger && cth)
        run(std::integral_constant<bool, NCT == 2 && PH == 1>{});
    else
        run(std::false_type{});
    __syncthreads();                                          // all patch reads done: the buffers become the exchange area

    // ------------------------------------------------------------------ epilogue
    // four slices of four accumulator registers: every wave writes its tiles' slice, then thread (wave w, lane l) owns register
    // 4 s + w of lane l -- output channel co, column pair l31 -- reads ALL tiles there and runs the output transforms
    const float slope = a.slope ? *a.slope : 1.0f;
    const bool has_act = a.slope != nullptr;
    float* E = smem + cth * (NT * 4 * 64);                    // one exchange area per co tile
    // the pair's two output columns jA, jA + 1 of the thread's two outputs rt: the two rows of a full tile, or (edge workgroup) the
    // one row of the column blocks jt, jt + 1
    const int jAc[2] = {j0 + 2 * l31, j0 + 2 * l31 + (edge ? 64 : 0)};
    bool keep[2][2], inb[2][2];
    int ja[2][2];                                             // the addend's column: utterance b / add_div of its own buffer
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = jAc[c] + q;
            const int bj = j / a.Tp, tp = j - bj * a.Tp;
            inb[c][q] = j < a.J;
            keep[c][q] = inb[c][q] && tp >= 1 && tp <= a.t_valid;
            ja[c][q] = j - (bj - bj / a.add_div) * a.Tp;
        }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s > 0) __syncthreads();
#pragma unroll
        for (int k = 0; k < NTW; ++k) {
            const int t = tw_tile(PH, w4, k);
            if (t >= 0) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) E[(t * 4 + rr) * 64 + lane] = acc[k][4 * s + rr];
            }
        }
        __syncthreads();
        float v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) v[t] = E[(t * 4 + w4) * 64 + lane];
        // time, then Gauss: P[r][q][re / im]
        float pr[NR][2], pi[NR][2];
        tw_recombine<NR>(v, pr, pi);
        const int rg = 4 * s + w4;
        const int co = ct * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * half;
        const bool cok = co < a.Cout;
        const EpiRow e = epi_row(a.epi, co);
        float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const int fo = edge ? a.Fout - 1 : 2 * m0 + PH + 2 * rt;
            const int jA = jAc[rt];
            if (fo >= a.Fout) continue;
            float yr[2], yi[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float re, im;
                if (PH == 0) {
                    re = rt == 0 ? pr[0][q] + pr[1][q] + pr[2][q] : pr[1][q] - pr[2][q] - pr[NR - 1][q];
                    im = rt == 0 ? pi[0][q] + pi[1][q] + pi[2][q] : pi[1][q] - pi[2][q] - pi[NR - 1][q];
                    if (edge) {                               // the two raw-tap products of column block rt
                        re = pr[2 * rt][q] + pr[(2 * rt + 1) % NR][q];
                        im = pi[2 * rt][q] + pi[(2 * rt + 1) % NR][q];
                    }
                } else {
                    re = rt == 0 ? pr[0][q] + pr[1][q] : pr[1][q] - pr[2][q];
                    im = rt == 0 ? pi[0][q] + pi[1][q] : pi[1][q] - pi[2][q];
                }
                if (a.add && cok && inb[rt][q]) {
                    re += epi_addend(a.add, co, a.Fout, fo, a.add_Jp, ja[rt][q]);
                    im += epi_addend(a.add, a.Cout + co, a.Fout, fo, a.add_Jp, ja[rt][q]);
                }
                const EpiPoint y = epi_point(re, im, e.z, e.sr, e.si, a.has_fold, has_act, slope);
                yr[q] = keep[rt][q] ? y.r : 0.f;
                yi[q] = keep[rt][q] ? y.i : 0.f;
                if (STATS && keep[rt][q]) epi_stats_add(st, yr[q], yi[q]);
            }
            if (cok) {
                float* o_r = a.out + ((size_t)co * a.Fout + fo) * a.Jp + jA;
                float* o_i = a.out + ((size_t)(a.Cout + co) * a.Fout + fo) * a.Jp + jA;
                if (inb[rt][1]) {
                    *(float2*)o_r = make_float2(yr[0], yr[1]);
                    *(float2*)o_i = make_float2(yi[0], yi[1]);
                } else if (inb[rt][0]) {
                    o_r[0] = yr[0];
                    o_i[0] = yi[0];
                }
            }
        }
        if (STATS) {
            // the 32 lanes of a half-wave hold the 32 column pairs of ONE output channel
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                float tsum = st[q];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) tsum += __shfl_xor(tsum, o, 64);
                if (l31 == 0 && cok)
                    atomicAdd(&a.stats[((size_t)(a.stats_rep > 1 ? (blockIdx.x & (a.stats_rep - 1)) : 0) * a.Cout + co) * 5 + q], (double)tsum);
            }
        }
    }
}

// cgemm_wino's fragments [phase][ct][unit = ci * 3 + g][slot r (4)][lane = h * 32 + co] (h: the two time taps as the MFMA's two k,
// h = 0 multiplies column j + tshift) -> [phase][ct][pair u][tile t = r * 9 + g * 3 + tau (36 | 28 slots)][lane = parity * 32 + co]
// with the time-transformed taps  tau 0: W_h0,  tau 1: W_h0 + W_h1,  tau 2: W_h1.  A third region in the even-row phase's layout holds
// the RAW frequency taps of the edge workgroups in place of the frequency products r: waves 0, 2 the tap W4 (the even-row phase's
// slot r = 0), waves 1, 3 the tap W2 = slot r = 1 minus slot r = 2 ((W4 + W2 + W0) / 2 - (W4 - W2 + W0) / 2).
__global__ void pack_cconv_tw_kernel(const float* __restrict__ wino, int cotiles, int UN, int UP, int cin, float* __restrict__ out) {
    const long long n0 = (long long)cotiles * UP * tw_ntp<0>() * 64, n1 = (long long)cotiles * UP * tw_ntp<1>() * 64;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n0 + n1 + n0; idx += (long long)gridDim.x * blockDim.x) {
        const bool raw = idx >= n0 + n1;
        const int ph = idx >= n0 && !raw;
        const long long i = raw ? idx - n0 - n1 : (ph ? idx - n0 : idx);
        const int ntp = ph ? tw_ntp<1>() : tw_ntp<0>(), nt = ph ? tw_nt<1>() : tw_nt<0>();
        const int lane = (int)(i & 63);
        long long t_ = i >> 6;
        const int t = (int)(t_ % ntp); t_ /= ntp;
        const int u = (int)(t_ % UP);
        const int ct = (int)(t_ / UP);
        float val = 0.f;
        // per (channel pair u, wave w) WS = 9 / 8 slots: two groups of [64 lanes][4 tiles] (+ one of [64 lanes] in the even-row phase);
        // the odd-row phase's slot 7 (and wave 3's slot 6) hold zero taps
        const int ws_ = ph ? tw_wslots<1>() : tw_wslots<0>();
        const int pos = t * 64 + lane, w = pos / (ws_ * 64), q = pos % (ws_ * 64);
        const int k = q < 512 ? (q >> 8) * 4 + (q & 3) : 8;
        const int ln = q < 512 ? (q & 255) >> 2 : q - 512;
        const int tt = k < (ph ? 7 : 9) ? tw_tile(ph, w, k) : -1;
        const int ci = 2 * u + (ln >> 5), co = ln & 31;
        if (tt >= 0 && ci < cin) {                             // (channels past cin: zero taps, whatever the source holds there)
            const int r = tt / 9, g = (tt % 9) / 3, tau = tt % 3;
            const float* src = wino + ((((size_t)ph * cotiles + ct) * UN + (size_t)ci * 3 + g) * 4 + (raw ? 0 : r)) * 64;
            float w0 = src[co], w1 = src[32 + co];
            if (raw && (r & 1)) {
                w0 = src[64 + co] - src[128 + co];
                w1 = src[64 + 32 + co] - src[128 + 32 + co];
            }
            val = tau == 0 ? w0 : (tau == 1 ? w0 + w1 : w1);
        }
        out[idx] = val;
    }
}

template <int PH, int CIK, bool LEFT, bool STATS, int NCT>
int launch_tw_ph_l(const TwArgs& a, hipStream_t st) {
    constexpr int NE = CIK * (PH == 0 ? 4 : 3) * 9 * 32;
    constexpr size_t smem = 2 * NE * sizeof(float);
    static_assert(smem * (NCT == 1 ? 2 : 1) <= 160 * 1024, "the patch buffers of two workgroups (NCT = 2: of one) must fit the 160 KB of LDS");
    TwArgs b = a;
    if (b.cotiles % NCT) return IDV_EINVAL;                   // (NCT = 2: the caller checked that the co-tile count is even)
    b.grid = tw_grid(PH, a.Fin, a.J, b.cotiles / NCT, TW_XCD_SPLIT);
    b.stagger = TW_PAIR_STAGGER;
    const long long nblk = tw_grid_blocks(b.grid);
    if (nblk == 0) return IDV_OK;
    if (nblk > 0x7fffffffLL) return IDV_EINVAL;
    constexpr auto k = cconv_tw_kernel<PH, CIK, LEFT, STATS, NCT>;
    if (int rc = idv_dyn_smem_once<k>(smem)) return rc;
    hipLaunchKernelGGL(k, dim3((unsigned)nblk), dim3(256 * NCT), smem, st, b);
    if (NCT > 1) idv_tw_pair_note_launch();
    return idv_launch_status();
}

// one choice over (statistics, two co tiles per workgroup, side of the time taps).  Two co tiles per workgroup (idv_tw_pair bit PH)
// need an even number of co tiles.
template <int PH, int CIK>
int launch_tw_ph(const TwArgs& a, hipStream_t st) {
    const bool pair = a.cotiles % 2 == 0 && ((idv_tw_pair(-1) >> PH) & 1);
    switch ((a.stats ? 4 : 0) | (pair ? 2 : 0) | (a.tshift ? 1 : 0)) {
        case 0: return launch_tw_ph_l<PH, CIK, false, false, 1>(a, st);
        case 1: return launch_tw_ph_l<PH, CIK, true, false, 1>(a, st);
        case 2: return launch_tw_ph_l<PH, CIK, false, false, 2>(a, st);
        case 3: return launch_tw_ph_l<PH, CIK, true, false, 2>(a, st);
        case 4: return launch_tw_ph_l<PH, CIK, false, true, 1>(a, st);
        case 5: return launch_tw_ph_l<PH, CIK, true, true, 1>(a, st);
        case 6: return launch_tw_ph_l<PH, CIK, false, true, 2>(a, st);
        default: return launch_tw_ph_l<PH, CIK, true, true, 2>(a, st);
    }
}

}  // namespace

// ---- the switch of the paired form, for this file and cgemm_tw2.hip.  Bits: 1 = transposed form, even-row phase; 2 = transposed form,
// odd-row phase; 4 = conv form.  IDV_TW_PAIR in the environment is read once; idv_tw_pair(mask >= 0) sets it in-process.
namespace {
std::atomic<int>& tw_pair_mask() {
    static std::atomic<int> v{[] { const char* e = getenv("IDV_TW_PAIR"); return e ? atoi(e) & IDV_TW_PAIR_ALL : IDV_TW_PAIR_DEFAULT; }()};
    return v;
}
std::atomic<long long> tw_pair_launches{0};
}  // namespace
void idv_tw_pair_note_launch() { tw_pair_launches.fetch_add(1, std::memory_order_relaxed); }
extern "C" int idv_tw_pair(int mask) {
    if (mask < 0) return tw_pair_mask().load(std::memory_order_relaxed);
    return tw_pair_mask().exchange(mask & IDV_TW_PAIR_ALL, std::memory_order_relaxed);
}
extern "C" long long idv_tw_pair_launches(int reset) {
    return reset ? tw_pair_launches.exchange(0, std::memory_order_relaxed) : tw_pair_launches.load(std::memory_order_relaxed);
}

// 1 if idv_ctconv2d_tw_fwd serves the layer: a transposed conv that cgemm_gauss serves, with at least two input rows, at least one
// FULL tile of 32 complex output channels (a workgroup is one co tile x 64 columns, so unlike cgemm_wino's four-co-tile form the
// 32-channel layer dec4 is served: 6.13 -> see DESIGN.md 3.1e) and, with a second source, C0 a multiple of 8 (a K chunk of 8 channels
// never straddles the sources).  IDV_TW_MIN_COUT (experiments): narrowest output served.
extern "C" int idv_cconv_tw_supported(int C0, int C1, int Cout, int Fin) {
    static const int min_cout = [] { const char* e = getenv("IDV_TW_MIN_COUT"); return e ? atoi(e) : 32; }();
    if (Cout < min_cout || Fin < 2) return 0;
    if (!idv_cconv_gauss_supported(C0, C1, Cout)) return 0;
    return (C1 == 0 || C0 % 8 == 0) ? 1 : 0;
}

extern "C" long long idv_cconv_tw_wfrag_floats(int Cout, int cin_used) {
    const long long cotiles = (Cout + 31) / 32, cpad = (cin_used + TW_PACK_CI - 1) / TW_PACK_CI * TW_PACK_CI;
    return cotiles * (cpad / 2) * (36 + 32 + 36) * 64;        // even-row phase, odd-row phase, raw taps of the edge workgroups
}

// wino_frag: idv_pack_cconv_wino(transposed = 1) of the same weights; tw_frag: idv_cconv_tw_wfrag_floats floats
extern "C" int idv_pack_cconv_tw(const float* wino_frag, int Cout, int cin_used, float* tw_frag, void* stream) {
    if (!wino_frag || !tw_frag || Cout <= 0 || cin_used <= 0) return IDV_EINVAL;
    const int cotiles = (Cout + 31) / 32;
    const int cpad = (cin_used + TW_PACK_CI - 1) / TW_PACK_CI * TW_PACK_CI;
    const long long n = idv_cconv_tw_wfrag_floats(Cout, cin_used);
    const unsigned blocks = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(pack_cconv_tw_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, wino_frag, cotiles, cpad * 3, cpad / 2,
                       cin_used, tw_frag);
    return idv_launch_status();
}

// idv_cconv2d_wino_fwd (transposed = 1; statistics and addend as there) on the time-Winograd kernels: same result up to the rounding of
// the transforms.  wfrag from idv_pack_cconv_tw, epi / has_fold from idv_pack_cconv_gauss.  Requires 16-byte aligned sources, Jp % 4
// == 0 and, with a second source, the same pitch.  Reference: model/complex_progress.py:222-279 (+ :161-209 and pvae_module.py:82
// for the epilogue).
extern "C" int idv_ctconv2d_tw_fwd(const float* x0, int C0, const float* x1, int C1, const float* wfrag, const float* epi, int has_fold,
                                   const float* prelu_slope, float* out, double* stats, double* stats_work, int stats_rep, int tshift,
                                   int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out, const float* addend, int addend_div,
                                   int addend_Jp, void* stream) {
    if (!x0 || !wfrag || !epi || !out || C0 <= 0 || Cout <= 0 || Fin <= 0 || B <= 0 || Tp <= 1) return IDV_EINVAL;
    const EpiStatsTarget sums{stats, stats_work, stats_rep};
    if (!sums.ok()) return IDV_EINVAL;
    if (addend && (addend_div < 1 || B % addend_div || addend_Jp < (B / addend_div) * Tp)) return IDV_EINVAL;
    if (C1 > 0 && !x1) return IDV_EINVAL;
    if (tshift != 0 && tshift != -1) return IDV_EINVAL;
    if (!idv_cconv_tw_supported(C0, C1, Cout, Fin)) return IDV_EINVAL;
    if ((Jp & 3) || (reinterpret_cast<uintptr_t>(x0) & 15) || (C1 > 0 && (reinterpret_cast<uintptr_t>(x1) & 15)) ||
        (reinterpret_cast<uintptr_t>(out) & 7))
        return IDV_EINVAL;
    TwArgs a{};
    a.x0 = x0; a.x1 = x1; a.C0 = C0; a.C1 = C1;
    a.Fin = Fin; a.Fout = 2 * Fin - 1;
    a.J = B * Tp; a.Jp = Jp; a.Tp = Tp;
    a.wfrag = wfrag; a.UP = (C0 + C1 + TW_PACK_CI - 1) / TW_PACK_CI * TW_PACK_CI / 2;
    a.epi = epi; a.has_fold = has_fold; a.slope = prelu_slope; a.out = out;
    a.Cout = Cout; a.cotiles = (Cout + 31) / 32;
    a.tshift = tshift; a.t_valid = t_valid_out;
    a.add = addend; a.add_div = addend ? addend_div : 1; a.add_Jp = addend_Jp;
    if (Jp < a.J) return IDV_EINVAL;
    if ((long long)4 * 8 * Fin * (long long)Jp >= 0xffffffffLL) return IDV_EINVAL;   // (the staging's 32-bit byte offsets)
    hipStream_t st = (hipStream_t)stream;
    sums.set(a);
    int rc = 0;
    rc = launch_tw_ph<0, 8>(a, st);
    if (!rc) rc = launch_tw_ph<1, 8>(a, st);
    return sums.finish(rc, Cout, st);
}
