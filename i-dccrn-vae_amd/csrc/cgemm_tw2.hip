// cgemm_tw2: the complex Conv2d contraction (encoder block: kernel (5, 2), stride (2, 1); model/complex_progress.py:8-36) in the form of
// cgemm_tw.hip -- three real products per complex product (Gauss), the FREQUENCY taps in Winograd form (cgemm_wino.hip's conv form: 7
// products on the raw rows r0..r6 = input rows 2 fo - 2 .. 2 fo + 4 of a pair of output rows, into FOUR accumulators
//     A0 = (r0 - r4) W0 + (r1 - r3) W1          A1 = (r2 + r4) (W0 + W2 + W4)/2 + r3 (W1 + W3)
//     A2 = (r4 - r2) (W0 - W2 + W4)/2           A3 = (r2 - r6) W4 + (r3 - r5) W3
//     out[fo] = A0 + A1 + A2                    out[fo + 1] = A1 - A2 - A3 ),
// and the two TIME taps as F(2,2) over pairs of output columns (cgemm_tw.hip: three products (a - b) Wa, b (Wa + Wb), (b - d) Wb per
// column pair, the MFMA's two k = two input channels).  Per (channel pair, co tile, 64 columns, pair of output rows): 7 x 3 x 3 = 63
// MFMAs into 4 x 9 = 36 accumulator tiles -- 0.39 of the reference's real products.
//
// The 63 MFMAs do not divide by four waves along any one axis; the deal that balances them with nine accumulators per wave:
//     waves 0, 1, 2 = accumulator A0, A1, A3 (two products each) on planes 0 .. 6      -> 14 MFMAs
//                   + accumulator A2 (one product) on planes 2 w, 2 w + 1              ->  2 MFMAs       (16 per k-step)
//     wave 3        = A0, A1, A3 on planes 7, 8 (12 MFMAs) + A2 on planes 6, 7, 8 (3)                     (15 per k-step)
// Staging, LDS layout (raw rows, planes paired per column pair), weight ring and the epilogue exchange are cgemm_tw.hip's; the
// frequency transform A + cb B happens at the operand read.  Weights: cgemm_wino's conv fragments re-ordered by idv_pack_cconv_tw2.
//
// Odd row counts with Fin = 2 Fout - 1 (every encoder layer of the model): the last output row has no partner, and rows Fin, Fin + 1
// are padding, so  out[Fout - 1] = W0 x[Fin - 3] + W1 x[Fin - 2] + W2 x[Fin - 1].  It is not a row tile of its own: the launch holds
// EDGE workgroups (cgemm_tw_map.hpp) that compute that row for TWO adjacent column blocks with the raw taps.  Raw slot 3 c + t of the
// patch buffer holds row Fin - 3 + t of column block c; wave w works on column block w >> 1, an even wave on planes 0 .. 4 (15 MFMAs
// per k-step), an odd wave on planes 5 .. 8 (12), the three taps of a plane into ONE accumulator (at most five per wave).  Staging,
// barriers, weight ring and epilogue exchange are those of a full tile; the K loop is a further copy with other operand reads and a
// second weight region (the raw taps, time-transformed).
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include "cgemm.hpp"
#include "conv_epilogue.hpp"
#include "cgemm_tw_map.hpp"
#include "cgemm_tw_stage.hpp"
#include "../../include/idccrn_hip.h"

namespace {

// LDS operand reads through address-space pointers: base register + compile-time offset in the read's immediate (cgemm_tw.hip)
typedef __attribute__((address_space(3))) float LdsF;
typedef float TwF2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) TwF2 LdsF2;

typedef f32x4 f32x4_a4 __attribute__((aligned(4)));     // a 16-byte global load at any float

struct Tw2Args {
    const float* x0;      // planar [2][Cin][Fin][Jp]
    int Cin;
    int Fin, Fout;
    int J, Jp, Tp;
    const float* wfrag;   // [cotiles][UP][4 waves][4 groups][64 lanes][4 slots], then the raw taps of the edge workgroups in the same
                          // layout (idv_pack_cconv_tw2)
    int UP;               // channel pairs per co tile as packed
    const float* epi;     // as cgemm_gauss: [cotiles * 32][8]
    int has_fold;
    const float* slope;
    float* out;           // planar [2][Cout][Fout][Jp]
    int Cout, cotiles;
    int tshift, t_valid;
    double* stats;
    int stats_rep;
    TwGrid grid;          // block order (cgemm_tw_map.hpp); cgroups = cotiles / NCT workgroups per (column block, row pair)
    int stagger;          // NCT = 2: waves 4 .. 7 stage eight MFMA slots later than their SIMD partners, waves 0 .. 3
};

constexpr int TW2_PACK_CI = 8;     // pack granularity in complex input channels (cgemm_wino's WCIK)
// block order and staging stagger as cgemm_tw.hip measured them: co tiles on different XCDs; with two co tiles per workgroup waves 4 .. 7
// stage later than their SIMD partners
constexpr int TW2_XCD_SPLIT = 1;
constexpr int TW2_PAIR_STAGGER = 1;

// product q of the conv form: raw rows (ra, rb), factor cb, accumulator
__host__ __device__ constexpr int tw2_ra(int q) { return q == 0 ? 0 : (q == 1 ? 2 : (q == 2 ? 4 : (q == 3 ? 2 : (q == 4 ? 1 : 3)))); }
__host__ __device__ constexpr int tw2_rb(int q) { return q == 0 ? 4 : (q == 1 ? 4 : (q == 2 ? 2 : (q == 3 ? 6 : (q == 4 ? 3 : (q == 5 ? 3 : 5))))); }
__host__ __device__ constexpr float tw2_cb(int q) { return q == 1 ? 1.f : (q == 5 ? 0.f : -1.f); }
// the two products of accumulator a (a = 0, 1, 3) and the product of accumulator 2
__host__ __device__ constexpr int tw2_qx(int a) { return a == 0 ? 0 : (a == 1 ? 1 : 3); }
__host__ __device__ constexpr int tw2_qy(int a) { return a == 0 ? 4 : (a == 1 ? 5 : 6); }
__host__ __device__ constexpr int tw2_main_acc(int w) { return w == 2 ? 3 : w; }          // wave 0, 1, 2 -> A0, A1, A3
// MFMA slot k (0 .. 15) of wave w -> product q and plane, or q = -1 (wave 3's 16th slot)
__host__ __device__ inline void tw2_slot(int w, int k, int& q, int& plane) {
    if (w < 3) {
        if (k < 14) { q = (k & 1) ? tw2_qy(tw2_main_acc(w)) : tw2_qx(tw2_main_acc(w)); plane = k >> 1; }
        else { q = 2; plane = 2 * w + (k - 14); }
    } else {
        if (k < 12) { const int a = tw2_main_acc(k >> 2); q = (k & 1) ? tw2_qy(a) : tw2_qx(a); plane = 7 + ((k >> 1) & 1); }
        else if (k < 15) { q = 2; plane = 6 + (k - 12); }
        else { q = -1; plane = 0; }
    }
}
// accumulator i (0 .. 8) of wave w -> tile t = a * 9 + plane of the epilogue exchange
__host__ __device__ inline int tw2_acc_tile(int w, int i) {
    if (w < 3) return i < 7 ? tw2_main_acc(w) * 9 + i : 2 * 9 + 2 * w + (i - 7);
    return i < 6 ? tw2_main_acc(i >> 1) * 9 + 7 + (i & 1) : 2 * 9 + 6 + (i - 6);
}

// edge workgroup, wave w (odd = w & 1): MFMA slot k (0 .. 15) -> raw tap t and plane, false: no product in the slot.  Even waves:
// planes 0 .. 4, slot = tap * 5 + plane (slot 15 empty); odd waves: planes 5 .. 8, three products in each group of four slots.  The
// accumulator of a slot is its plane less the wave's first; its three taps follow one another in k.
__host__ __device__ inline bool tw2_eslot(bool odd, int k, int& t, int& plane) {
    if (odd) {
        const int m = (k >> 2) * 3 + (k & 3);
        t = m >> 2;
        plane = 5 + (m & 3);
        return (k & 3) != 3;
    }
    t = k / 5;
    plane = k % 5;
    return k < 15;
}
// accumulator i (0 .. 8) of edge wave w -> tile of the epilogue exchange: column block c = w >> 1's sums at c * 9 + plane, the
// accumulators without a product (zero) on the 18 tiles behind, so that every tile the epilogue reads is written
__host__ __device__ inline int tw2_edge_tile(int w, int i) {
    const int c = w >> 1;
    if (w & 1) return i < 4 ? c * 9 + 5 + i : 18 + c * 9 + i;
    return i < 5 ? c * 9 + i : 18 + c * 9 + (i - 5);
}

// offset of plane p inside a raw row of the patch buffer (planes (2 j, 2 j + 1) interleaved per column pair, plane 8 apart), lane part
__device__ __forceinline__ int tw2_poff(int p, int l31) { return p < 8 ? (p >> 1) * 64 + 2 * l31 + (p & 1) : 256 + l31; }

// NCT: co tiles per workgroup (cgemm_tw.hip).  2: eight waves, waves 0 .. 3 on co tile 2 p, waves 4 .. 7 the same program on co tile
// 2 p + 1, one staging of the raw rows for both.  The 448 items of a chunk go to 512 threads, one each; the 64 threads of wave 7 have
// none and stage a dead item (loads of a valid address, stores to a dump row behind the patch buffer), so that the staging is free of
// a per-wave branch (with one the register allocator spills three times what NCT = 1 does).
constexpr int tw2_smem_floats(int nct) {
    // NCT = 1: two patch buffers; NCT = 2: two patch buffers with a dump row each, or the two exchange areas of the epilogue (larger)
    return nct == 1 ? 2 * 4 * 7 * 288 : (2 * (4 * 7 * 288 + 288) > 2 * 36 * 4 * 64 ? 2 * (4 * 7 * 288 + 288) : 2 * 36 * 4 * 64);
}
template <bool LEFT, bool STATS, int NCT = 1>
__global__ __launch_bounds__(256 * NCT, NCT == 1 ? 2 : 1) void cconv_tw2_kernel(const Tw2Args a) {
    constexpr int NT = 36, NACC = 9, NSLOT = 16;
    constexpr int NRAW = 7, CIK = 4, KS = 2;
    constexpr int RT = NRAW * 288;               // floats per channel in a patch buffer
    constexpr int NE = CIK * RT;
    constexpr int NEB = NCT == 1 ? NE : NE + 288;    // buffer pitch (NCT = 2: + the dump row of the threads without an item)
    constexpr int NITEM = CIK * NRAW * 16;       // 448 staging items per chunk: (channel, raw row, 2 column pairs)
    constexpr int NTHR = 256 * NCT;
    constexpr int NLD = (NITEM + NTHR - 1) / NTHR;
    static_assert(NCT == 1 || NCT == 2, "one or two co tiles per workgroup");
    static_assert(2 * NEB <= tw2_smem_floats(NCT) && NCT * NT * 4 * 64 <= tw2_smem_floats(NCT),
                  "the patch buffers and the epilogue exchange (one area per co tile) fit the allocation");

    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the wave's place in its co tile's program; which co tile of the workgroup
    const int w4 = NCT == 1 ? wave : wave & 3, cth = NCT == 1 ? 0 : wave >> 2;
    const int half = lane >> 5, l31 = lane & 31;

    // block order: cgemm_tw_map.hpp.  An EDGE workgroup (block-uniform) computes the last output row of the column blocks jt, jt + 1
    TwTile tile;
    if (!tw_block_tile(a.grid, blockIdx.x, tile)) return;
    const bool edge = tile.edge;
    const int jt = tile.jt, ft = tile.ft;
    const int ct = NCT * tile.ct + cth;           // (tile.ct is the workgroup's group of NCT co tiles)
    const int j0 = jt * 64;
    const int m0 = 2 * ft;                        // first OUTPUT row of the pair
    const int rbase = 2 * m0 - 2;                 // raw row r0

    const int Cin = a.Cin;
    const int nchunk = (Cin + CIK - 1) / CIK;

    f32x16 acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    // ---- staging (cgemm_tw.hip): item = channel cl, raw row, column pairs 2 c8, 2 c8 + 1.  Edge workgroup: raw slot rl < 6 holds
    // (column block jt + rl / 3, row Fin - 3 + rl % 3), slot 6 nothing; a second column block past J is masked like any column out of
    // range
    f32x4 v_r[NLD], v_i[NLD];
    float e_r[NLD], e_i[NLD];
    unsigned off_v[NLD], ldsoff[NLD];
    unsigned okmask[NLD];     // bits 0-4: window column valid; bit 5: row valid
    bool interior[NLD];
    auto item_cl = [&](int i) -> int { return (tid + i * NTHR) / (16 * NRAW); };
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        // the address function: cgemm_tw_stage.hpp.  A BYTE offset from the chunk's wave-uniform row bases: scalar base + 32-bit lane
        // offset.  (NCT = 2, no item: channel CIK is dead in every chunk, and its row 0 is the dump row behind the buffer)
        const TwStageItem it = tw2_stage_item(tid + i * NTHR, NITEM, NCT == 2, LEFT, edge, a.Fin, a.J, a.Jp, j0, rbase);
        off_v[i] = it.off_v;
        okmask[i] = it.mask;
        interior[i] = __builtin_amdgcn_ballot_w64((it.mask & 0x3fu) == 0x3fu) == ~0ull;
        ldsoff[i] = it.ldsoff;
    }
    // the second item exists in waves 0 .. 2 only (448 items); NCT = 2: one item in every thread (wave 7: a dead one)
    auto item_exists = [&](int i) -> bool { return i == 0 || wave * 64 + 256 < NITEM; };
    auto stage_load = [&](int chunk, int i) {
        if (!item_exists(i)) return;
        const int ci0 = chunk * CIK;
        const float* br = a.x0 + (size_t)ci0 * a.Fin * a.Jp;
        const float* bi = br + (size_t)Cin * a.Fin * a.Jp;
        const bool dead = item_cl(i) >= Cin - ci0;
        const unsigned ov = dead ? 4u * TW2_DUMMY : off_v[i];
        // the five-column window as ONE vector (its first four columns) and one scalar (the fifth) on both tap sides; tap left: the
        // vector starts a float in front of the 16-byte slot.  (Loaded as the aligned slot and the column in front, the compiler
        // merges the two into this same pair of loads, re-assembles v / e from their components right behind the loads and waits
        // for them there: a global round trip per chunk in the slot that issues them.)
        const float* pr = (const float*)((const char*)br + ov) - (LEFT ? 1 : 0);
        const float* pi = (const float*)((const char*)bi + ov) - (LEFT ? 1 : 0);
        using Win = std::conditional_t<LEFT, f32x4_a4, f32x4>;
        v_r[i] = *(const Win*)pr;
        v_i[i] = *(const Win*)pi;
        e_r[i] = pr[4];
        e_i[i] = pi[4];
    };
    float fr[5], fi[5];
    auto stage_window = [&](int chunk, int i) {
        if (!item_exists(i)) return;
        const int cvalid = Cin - chunk * CIK;
        if (interior[i] && cvalid >= CIK) {
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                fr[q] = q == 4 ? e_r[i] : v_r[i][q == 4 ? 3 : q];
                fi[q] = q == 4 ? e_i[i] : v_i[i][q == 4 ? 3 : q];
            }
            return;
        }
        unsigned m = okmask[i];
        if (item_cl(i) >= cvalid || !((m >> 5) & 1u)) m &= ~0x1fu;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float xr = q == 4 ? e_r[i] : v_r[i][q == 4 ? 3 : q];
            const float xi = q == 4 ? e_i[i] : v_i[i][q == 4 ? 3 : q];
            const bool cok = (m >> q) & 1u;
            fr[q] = cok ? xr : 0.f;
            fi[q] = cok ? xi : 0.f;
        }
    };
    auto plane_val = [&](int gt, int pr) -> float {
        const int g = gt / 3, tau = gt - g * 3;
        const int q0 = 2 * pr;
        const float xa_ = g == 0 ? fr[q0] + fi[q0] : (g == 1 ? fr[q0] : fi[q0]);
        const float xb_ = g == 0 ? fr[q0 + 1] + fi[q0 + 1] : (g == 1 ? fr[q0 + 1] : fi[q0 + 1]);
        const float xd_ = g == 0 ? fr[q0 + 2] + fi[q0 + 2] : (g == 1 ? fr[q0 + 2] : fi[q0 + 2]);
        return tau == 0 ? xa_ - xb_ : (tau == 1 ? xb_ : xb_ - xd_);
    };
    auto stage_plane2 = [&](float* dst, int i, int j) {
        if (!item_exists(i)) return;
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

    // ---- weights: 16 slots per k-step as four 16-byte loads ([group][64 lanes][4 slots]).  ONE set of registers: group g of the next
    // k-step is fetched right after the four MFMAs that use group g of this one (two sets do not fit beside 144 accumulator, 32
    // operand and 20 staging registers)
    const float* wbase = a.wfrag + (((size_t)(edge ? a.cotiles : 0) + ct) * a.UP * 4 + w4) * 1024 + lane * 4;
    const int total_ks = nchunk * KS;
    float a_w[NSLOT];
    auto load_wg = [&](int g, int grp) {
        g = g < total_ks ? g : total_ks - 1;
        const f32x4 w4 = *(const f32x4*)(wbase + (size_t)g * 4096 + grp * 256);
#pragma unroll
        for (int k = 0; k < 4; ++k) a_w[grp * 4 + k] = w4[k];
    };

    // ---- operands.  Waves 0 .. 2: products x, y of the wave's main accumulator on planes 0 .. 6 and product 2 on the plane pair w:
    // six row offsets at run time, plane offsets constant.  Wave 3: every row constant.
    const int am = tw2_main_acc(w4 < 3 ? w4 : 0);
    const int qxm = tw2_qx(am), qym = tw2_qy(am);
    const int rxa = tw2_ra(qxm) * 288, rxb = tw2_rb(qxm) * 288, rya = tw2_ra(qym) * 288, ryb = tw2_rb(qym) * 288;
    const float cbx = tw2_cb(qxm), cby = tw2_cb(qym);
    const int r2a = tw2_ra(2) * 288 + w4 * 64, r2b = tw2_rb(2) * 288 + w4 * 64;     // (+ plane pair j = w of product 2)
    // operands in a rolling window of two groups of four slots: group g of a k-step is fetched while group g - 1 runs.
    // Role A (waves 0 .. 2): group g < 3 = product x planes (2 g, 2 g + 1) on slots 0, 2 and product y on slots 1, 3 (two 8-byte reads per
    // row each); group 3 = plane 6 of x, y (slots 0, 1) and product 2's plane pair (slots 2, 3).  Role B (wave 3): slots 4 g .. 4 g + 3 of
    // tw2_slot(3, .), one 4-byte read per row.
    float xa[2][4], xb[2][4];
    // The reads go through per-lane LDS BASES that a loop forms once (run(): the address of the wave's operand in k-step 0 of the
    // buffer being read); the k-step (koff floats), the plane and -- where it is constant -- the row are compile-time offsets of
    // the reads, and the bases move to the other buffer once per chunk.  Role A: five bases at 2 l31.  Row ya is the row behind xa in all
    // three waves, and the two 8-byte reads go out as ONE two-address read, whose two offsets are 8 bits of 8 bytes: xa / ya have a
    // base per k-step (pb[0], pb[2]), so that the pair needs no address add; rows xb, yb, 2a (2b a constant in front of it) one each.
    static_assert(tw2_ra(tw2_qy(tw2_main_acc(0))) == tw2_ra(tw2_qx(tw2_main_acc(0))) + 1 &&
                  tw2_ra(tw2_qy(tw2_main_acc(1))) == tw2_ra(tw2_qx(tw2_main_acc(1))) + 1 &&
                  tw2_ra(tw2_qy(tw2_main_acc(2))) == tw2_ra(tw2_qx(tw2_main_acc(2))) + 1, "row ya = row xa + 1");
    static_assert(KS == 2, "one xa / ya base per k-step");
    auto load_grp_a = [&](const LdsF* const* pb, int koff, int g, float (&oa)[4], float (&ob)[4]) {
        const LdsF* px = koff ? pb[2] + (koff - 2 * RT) : pb[0];
        if (g < 3) {
            const TwF2 xa_ = *(const LdsF2*)(px + g * 64), xb_ = *(const LdsF2*)(pb[1] + koff + g * 64);
            const TwF2 ya_ = *(const LdsF2*)(px + 288 + g * 64), yb_ = *(const LdsF2*)(pb[3] + koff + g * 64);
            oa[0] = xa_.x; oa[2] = xa_.y; ob[0] = xb_.x; ob[2] = xb_.y;
            oa[1] = ya_.x; oa[3] = ya_.y; ob[1] = yb_.x; ob[3] = yb_.y;
        } else {
            oa[0] = px[3 * 64]; ob[0] = pb[1][koff + 3 * 64];
            oa[1] = px[288 + 3 * 64]; ob[1] = pb[3][koff + 3 * 64];
            const TwF2 pa_ = *(const LdsF2*)(pb[4] + koff), pb_ = *(const LdsF2*)(pb[4] + koff + (tw2_rb(2) - tw2_ra(2)) * 288);
            oa[2] = pa_.x; oa[3] = pa_.y; ob[2] = pb_.x; ob[3] = pb_.y;
        }
    };
    // Role B (wave 3) reads 4 bytes per row at constant rows: base = buffer + channel of this half-wave, formed per k-step.  (On
    // per-lane bases like role A's the compiler pairs fewer of these reads into two-address reads, more LDS read instructions per
    // chunk; wave 3 keeps this form.)
    auto load_grp_b = [&](const float* base, int g, float (&oa)[4], float (&ob)[4]) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            int q, plane;
            tw2_slot(3, 4 * g + s4, q, plane);
            if (q < 0) continue;
            oa[s4] = base[tw2_ra(q) * 288 + tw2_poff(plane, l31)];
            ob[s4] = base[tw2_rb(q) * 288 + tw2_poff(plane, l31)];
        }
    };
    // Edge workgroup: the products of tw2_eslot, one 4-byte read each from raw slot 3 c + tap of the wave's column block c
    const int eoff = (w4 >> 1) * 3 * 288;
    // (two bases, the lane parts of tw2_poff: planes 0 .. 7 at 2 l31, plane 8 at l31; two neighbouring slots on the interleaved
    // planes (2 j, 2 j + 1) of one tap take ONE 8-byte read)
    auto load_grp_e = [&](auto odd_, const LdsF* const* pb, int koff, int g, float (&oa)[4]) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            int t, plane, t2 = -1, plane2 = -1;
            if (!tw2_eslot(decltype(odd_)::value, 4 * g + s4, t, plane)) continue;
            // slot s4 opens a pair with slot s4 + 1, or closes the pair slot s4 - 1 opened
            const bool two = s4 < 3 && tw2_eslot(decltype(odd_)::value, 4 * g + s4 + 1, t2, plane2) && t2 == t && !(plane & 1) &&
                             plane2 == plane + 1 && plane2 < 8;
            const bool second = s4 > 0 && tw2_eslot(decltype(odd_)::value, 4 * g + s4 - 1, t2, plane2) && t2 == t && (plane & 1) &&
                                plane2 == plane - 1 && plane < 8;
            if (second) continue;
            if (two) {
                const TwF2 v = *(const LdsF2*)(pb[0] + koff + t * 288 + (plane >> 1) * 64);
                oa[s4] = v.x;
                oa[s4 + 1] = v.y;
            } else {
                oa[s4] = pb[plane < 8 ? 0 : 1][koff + t * 288 + (plane < 8 ? (plane >> 1) * 64 + (plane & 1) : 256)];
            }
        }
    };
    // role A: the largest base + compile-time offset stays inside the two patch buffers (second buffer, odd channel of the last
    // k-step, raw row 6, plane pair 3, last pair), and the offsets fit the LDS read's immediate
    static_assert(NEB + (2 * (KS - 1) + 1) * RT + 6 * 288 + 3 * 64 + 2 * 31 + 1 < 2 * NEB, "operand reads stay inside the LDS allocation");
    static_assert((2 * (KS - 1) * RT + 6 * 288 + 256) * 4 < 65536, "k-step, row and plane offsets fit the LDS read's immediate");
    // edge waves: base = buffer + half-wave channel + eoff (column block 1: 3 raw slots) + lane part, immediate = k-step + tap t <= 2 +
    // plane; the largest is plane 8 of tap 2 of column block 1.  Wave 3 (load_grp_b, addresses formed per k-step from the buffer):
    // raw row <= 6, plane 8
    static_assert(NEB + (2 * (KS - 1) + 1) * RT + (3 + 2) * 288 + 256 + 31 < 2 * NEB, "edge-wave reads stay inside the LDS allocation");
    static_assert(NEB + (2 * (KS - 1) + 1) * RT + 6 * 288 + 256 + 31 < 2 * NEB, "wave 3's reads stay inside the LDS allocation");
    static_assert(tw2_rb(6) <= 6 && tw2_rb(3) <= 6 && tw2_ra(2) <= 6, "raw rows 0 .. 6");

    // chunk 0 into the first buffer, chunk 1 on its way, the first k-step's weights.  Every copy of the loop below begins with its own
    // copy of this: what a loop overwrites (staging registers, weights, operands) would otherwise have to survive, in the state this
    // prologue left, through every copy placed before the one that runs -- the register allocator sees the copies in a row -- and
    // with the edge copies that was 72 - 156 bytes of scratch per lane for NCT = 1; like this no instantiation spills
    auto prologue = [&]() {
#pragma unroll
        for (int i = 0; i < NLD; ++i) stage_load(0, i);
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) load_wg(0, grp);
#pragma unroll
        for (int i = 0; i < NLD; ++i) stage_store(smem, 0, i);
#pragma unroll
        for (int i = 0; i < NLD; ++i) stage_load(nchunk > 1 ? 1 : 0, i);
        __syncthreads();
    };

    // the main loop, once per wave role (the branch is outside the loop: straight-line loops, each with the workgroup's barriers).
    // Roles 0, 1: waves 0 .. 2 and wave 3 of a full tile; 2, 3: even and odd waves of an edge workgroup (all 16 slots are walked, for
    // the weight ring and the staging that ride on them; a slot without a product issues no MFMA)
    auto run = [&](auto role, auto late_) {
        constexpr int ROLE = decltype(role)::value;
        constexpr bool ROLE_B = ROLE == 1, EDGE = ROLE >= 2;
        using EdgeOdd = std::integral_constant<bool, ROLE == 3>;
        prologue();
        constexpr bool AHEAD = !EDGE && !ROLE_B;
        constexpr bool BASES = !ROLE_B;
        constexpr int NB = EDGE ? 2 : (BASES ? 5 : 1);
        const LdsF* pb[NB];
        if constexpr (EDGE) {
            pb[0] = (const LdsF*)smem + half * RT + eoff + 2 * l31;
            pb[1] = (const LdsF*)smem + half * RT + eoff + l31;
        } else if constexpr (BASES) {
            const int ro[5] = {rxa, rxb, rxa + 2 * RT, ryb, r2a};
#pragma unroll
            for (int j = 0; j < 5; ++j) pb[j] = (const LdsF*)smem + half * RT + ro[j] + 2 * l31;
        }
        int flip = NEB;                           // (uniform) to the other buffer: + NEB, then - NEB, ...
        const float* Pcur = smem;                 // (wave 3: the buffer being read)
        auto load_grp = [&](int koff, int g) {
            if constexpr (EDGE) load_grp_e(EdgeOdd{}, pb, koff, g, xa[g & 1]);
            else if constexpr (ROLE_B) load_grp_b(Pcur + (size_t)(koff / RT + half) * RT, g, xa[g & 1], xb[g & 1]);
            else load_grp_a(pb, koff, g, xa[g & 1], xb[g & 1]);
        };
        // frequency transform of slot k's operand (full tiles; the edge waves multiply raw rows)
        auto xform = [&](int k) -> float {
            float cb;
            if constexpr (ROLE_B) {
                int q, plane;
                tw2_slot(3, k, q, plane);
                cb = tw2_cb(q);
            } else {
                cb = k < 14 ? ((k & 1) ? cby : cbx) : -1.f;
            }
            return xa[(k >> 2) & 1][k & 3] + cb * xb[(k >> 2) & 1][k & 3];
        };
        constexpr int NK = ROLE_B ? NSLOT - 1 : NSLOT;
        load_grp(0, 0);
        // role A: the transform runs ONE MFMA ahead of its product (cgemm_tw.hip).  Wave 3 keeps it in front of its MFMA: ahead, the
        // compiler pairs fewer of its 4-byte reads (see load_grp_b), and its 15 slots per k-step are not the workgroup's pace.
        float bcur = 0.f;
        if constexpr (AHEAD) bcur = xform(0);
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            float* Pn = smem + ((chunk + 1) & 1) * NEB;
            if constexpr (ROLE_B) Pcur = smem + (chunk & 1) * NEB;
            const int nxt = chunk + 1 < nchunk ? chunk + 1 : chunk, nxt2 = chunk + 2 < nchunk ? chunk + 2 : nchunk - 1;
#pragma unroll
            for (int ul = 0; ul < KS; ++ul) {
                const bool staging = ul == 0;           // both items ride on k-step 0; the barrier sits in k-step 1
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int g = k >> 2, s4 = k & 3;
                    int ai;
                    bool product = true;
                    if (EDGE) {
                        int t, plane;
                        product = tw2_eslot(EdgeOdd::value, k, t, plane);
                        ai = plane - (EdgeOdd::value ? 5 : 0);
                    } else if (ROLE_B) {
                        ai = k < 12 ? k >> 1 : 6 + (k - 12);
                    } else {
                        ai = k < 14 ? k >> 1 : 7 + (k - 14);
                    }
                    // (slot 0 of the next k-step: its group was read behind slot 12 of this one)
                    float bn = 0.f;
                    if constexpr (AHEAD) {
                        bn = xform(k + 1 < NK ? k + 1 : 0);
                        asm volatile("" : "+v"(bn));          // (the transform is DONE here, not sunk to its product)
                        __builtin_amdgcn_sched_barrier(0);    // (in FRONT of MFMA k: behind it, it would sit right in front of MFMA k + 1)
                    }
                    // A role with empty slots (wave 3: slot 15; edge waves: slot 15, or every fourth) never reads those slots' weights.
                    // Left dead, their registers are handed out again while the group's 16-byte load is still in flight, and the write
                    // to one waits for ALL the wave's loads (vmcnt(0)) right behind the load's issue, in every k-step.  Read here, where
                    // the group's first MFMA waits for the load anyway, they stay the load's until it has landed.
                    if ((ROLE_B || EDGE) && s4 == 0) asm volatile("" ::"v"(a_w[k]), "v"(a_w[k + 1]), "v"(a_w[k + 2]), "v"(a_w[k + 3]));
                    if (s4 == 0) {
                        // the next group's operands (of this k-step, or group 0 of the next one: after the barrier in the last k-step)
                        if (!(ul == KS - 1 && g == 3)) load_grp(g < 3 ? 2 * ul * RT : 2 * (ul + 1) * RT, (g + 1) & 3);
                    }
                    if constexpr (EDGE) {
                        if (product) acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_w[k], xa[g & 1][s4], acc[ai], 0, 0, 0);
                    } else if constexpr (AHEAD) {
                        acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_w[k], bcur, acc[ai], 0, 0, 0);
                        bcur = bn;
                    } else {
                        acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_w[k], xform(k), acc[ai], 0, 0, 0);
                    }
                    if (ul == KS - 1 && k == 0) {
                        __builtin_amdgcn_sched_barrier(0);
                        __syncthreads();
                    }
                    if (ul == KS - 1 && k == 12) {
                        // (last k-step: group 0 of the next chunk comes from the other buffer, complete since the barrier above: the one
                        // address update of the chunk, every read from here on is of Pn)
                        if constexpr (BASES) {
#pragma unroll
                            for (int j = 0; j < NB; ++j) pb[j] += flip;
                            flip = -flip;
                        } else {
                            Pcur = Pn;
                        }
                        load_grp(0, 0);
                    }
                    // weights of the next k-step, group by group
                    if ((k & 3) == 3 || (ROLE_B && k == NSLOT - 2)) load_wg(chunk * KS + ul + 1, k >> 2);
                    if constexpr (NCT == 2) if (staging) {
                        // the one item: slots 0 .. 5 or (waves 4 .. 7 with a.stagger: not while the SIMD partner stages) slots 8 .. 13
                        constexpr bool late = decltype(late_)::value;
                        if (k <= 5 && !late) {
                            if (k == 0) stage_window(nxt, 0);
                            if (k >= 1) stage_plane2(Pn, 0, k - 1);
                            if (k == 5) stage_load(nxt2, 0);
                        }
                        if (k >= 8 && k <= 13 && late) {
                            if (k == 8) stage_window(nxt, 0);
                            if (k >= 9) stage_plane2(Pn, 0, k - 9);
                            if (k == 13) stage_load(nxt2, 0);
                        }
                    }
                    if constexpr (NCT == 1) if (staging) {
                        // item 0: window at slot 0, plane pairs at 1 .. 4, plane 8 at 5, reload at 5; item 1 (waves 0 .. 2): slots 8 .. 13
                        if (k == 0) stage_window(nxt, 0);
                        if (k >= 1 && k <= 5) stage_plane2(Pn, 0, k - 1);
                        if (k == 5) stage_load(nxt2, 0);
                        if (!ROLE_B) {
                            if (k == 8) stage_window(nxt, 1);
                            if (k >= 9 && k <= 13) stage_plane2(Pn, 1, k - 9);
                            if (k == 13) stage_load(nxt2, 1);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
    // (NCT = 2 with a.stagger: waves 4 .. 7 run the copies of the loops that stage eight slots later -- a copy, because a branch on the
    // wave inside the loop costs the register allocator 80 - 90 bytes of scratch per lane)
    using Late = std::integral_constant<bool, NCT == 2>;
    const bool late = NCT == 2 && a.stagger && cth;
    if (edge) {
        if (late) {
            if (w4 & 1)
                run(std::integral_constant<int, 3>{}, Late{});
            else
                run(std::integral_constant<int, 2>{}, Late{});
        } else if (w4 & 1)
            run(std::integral_constant<int, 3>{}, std::false_type{});
        else
            run(std::integral_constant<int, 2>{}, std::false_type{});
    } else if (late) {
        if (w4 < 3)
            run(std::integral_constant<int, 0>{}, Late{});
        else
            run(std::integral_constant<int, 1>{}, Late{});
    } else if (w4 < 3)
        run(std::integral_constant<int, 0>{}, std::false_type{});
    else
        run(std::integral_constant<int, 1>{}, std::false_type{});
    __syncthreads();                                          // all patch reads done: the buffers become the exchange area

    // ------------------------------------------------------------------ epilogue (cgemm_tw.hip's, 36 tiles)
    const float slope = a.slope ? *a.slope : 1.0f;
    const bool has_act = a.slope != nullptr;
    float* E = smem + cth * (NT * 4 * 64);                    // one exchange area per co tile
    // the pair's two output columns jA, jA + 1 of the thread's two outputs rt: the two rows of a full tile, or (edge workgroup) the
    // one row of the column blocks jt, jt + 1
    const int jAc[2] = {j0 + 2 * l31, j0 + 2 * l31 + (edge ? 64 : 0)};
    bool keep[2][2], inb[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = jAc[0] + q;
        const int tp = j % a.Tp;
        inb[0][q] = inb[1][q] = j < a.J;
        keep[0][q] = keep[1][q] = inb[0][q] && tp >= 1 && tp <= a.t_valid;
    }
    if (edge) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = jAc[1] + q;
            const int tp = j % a.Tp;
            inb[1][q] = j < a.J;
            keep[1][q] = inb[1][q] && tp >= 1 && tp <= a.t_valid;
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s > 0) __syncthreads();
#pragma unroll
        for (int k = 0; k < NACC; ++k) {
            const int t = edge ? tw2_edge_tile(w4, k) : tw2_acc_tile(w4, k);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) E[(t * 4 + rr) * 64 + lane] = acc[k][4 * s + rr];
        }
        __syncthreads();
        float v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) v[t] = E[(t * 4 + w4) * 64 + lane];
        float pr[4][2], pi[4][2];
        tw_recombine<4>(v, pr, pi);
        const int rg = 4 * s + w4;
        const int co = ct * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * half;
        const bool cok = co < a.Cout;
        const EpiRow e = epi_row(a.epi, co);
        float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const int fo = edge ? a.Fout - 1 : m0 + rt;
            const int jA = jAc[rt];
            if (fo >= a.Fout) continue;
            float yr[2], yi[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float re = rt == 0 ? pr[0][q] + pr[1][q] + pr[2][q] : pr[1][q] - pr[2][q] - pr[3][q];
                float im = rt == 0 ? pi[0][q] + pi[1][q] + pi[2][q] : pi[1][q] - pi[2][q] - pi[3][q];
                if (edge) {                                   // the taps are summed in the accumulators of column block rt
                    re = pr[rt][q];
                    im = pi[rt][q];
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

// cgemm_wino's conv fragments [ct][unit = ci * 3 + g][8 slots q][lane = h * 32 + co] -> [ct][pair u][wave][group][lane = parity * 32 +
// co][4 slots] with the time-transformed taps (tau 0: W_h0, tau 1: W_h0 + W_h1, tau 2: W_h1) of the slot's (product, plane).  A second
// region in the same layout holds the RAW frequency taps of the edge workgroups (tw2_eslot): tap 0 = W0 (slot q = 0), tap 1 = W1 (slot
// q = 4), tap 2 = W2 = slot 1 minus slot 2 ((W0 + W2 + W4) / 2 - (W0 - W2 + W4) / 2).
__global__ void pack_cconv_tw2_kernel(const float* __restrict__ wino, int cotiles, int UN, int UP, float* __restrict__ out) {
    const long long n = (long long)cotiles * UP * 4096;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < 2 * n; idx += (long long)gridDim.x * blockDim.x) {
        const bool raw = idx >= n;
        const long long i = raw ? idx - n : idx;
        const int kk = (int)(i & 3), ln = (int)((i >> 2) & 63), grp = (int)((i >> 8) & 3), w = (int)((i >> 10) & 3);
        const long long t_ = i >> 12;
        const int u = (int)(t_ % UP), ct = (int)(t_ / UP);
        int q, plane;
        if (raw) {
            int t;
            q = tw2_eslot(w & 1, grp * 4 + kk, t, plane) ? (t == 0 ? 0 : (t == 1 ? 4 : 1)) : -1;
        } else {
            tw2_slot(w, grp * 4 + kk, q, plane);
        }
        float val = 0.f;
        const int ci = 2 * u + (ln >> 5), co = ln & 31;
        if (q >= 0 && ci * 3 < UN) {
            const int g = plane / 3, tau = plane % 3;
            const float* src = wino + ((((size_t)ct * UN + (size_t)ci * 3 + g) * 8 + q)) * 64;
            float w0 = src[co], w1 = src[32 + co];
            if (raw && q == 1) {
                w0 -= src[64 + co];
                w1 -= src[64 + 32 + co];
            }
            val = tau == 0 ? w0 : (tau == 1 ? w0 + w1 : w1);
        }
        out[idx] = val;
    }
}

template <bool LEFT, bool STATS, int NCT>
int launch_tw2(const Tw2Args& a, hipStream_t st) {
    constexpr size_t smem = tw2_smem_floats(NCT) * sizeof(float);
    static_assert(smem * (NCT == 1 ? 2 : 1) <= 160 * 1024, "the patch buffers of two workgroups (NCT = 2: of one) must fit the 160 KB of LDS");
    Tw2Args b = a;
    if (b.cotiles % NCT) return IDV_EINVAL;                   // (NCT = 2: the caller checked that the co-tile count is even)
    b.grid = tw2_grid(a.Fin, a.Fout, a.J, b.cotiles / NCT, TW2_XCD_SPLIT);
    b.stagger = TW2_PAIR_STAGGER;
    const long long nblk = tw_grid_blocks(b.grid);
    if (nblk > 0x7fffffffLL) return IDV_EINVAL;
    constexpr auto k = cconv_tw2_kernel<LEFT, STATS, NCT>;
    if (int rc = idv_dyn_smem_once<k>(smem)) return rc;
    hipLaunchKernelGGL(k, dim3((unsigned)nblk), dim3(256 * NCT), smem, st, b);
    if (NCT > 1) idv_tw_pair_note_launch();
    return idv_launch_status();
}

}  // namespace

// 1 if idv_cconv2d_tw_fwd serves the layer: a conv cgemm_gauss serves (one source) with at least one full tile of 32 complex output
// channels, at least 64 input channels (measured at B = 64: enc1, 32 -> 64 channels, 2.63 -> 2.86 ms: eight K chunks do not amortise the
// epilogue exchange; enc2-5 19.6 -> 18.7 ms) and at least two output rows.  IDV_TW2_MIN_COUT / IDV_TW2_MIN_CIN (experiments).
extern "C" int idv_cconv_tw2_supported(int Cin, int Cout, int Fin) {
    static const int min_cout = [] { const char* e = getenv("IDV_TW2_MIN_COUT"); return e ? atoi(e) : 32; }();
    static const int min_cin = [] { const char* e = getenv("IDV_TW2_MIN_CIN"); return e ? atoi(e) : 64; }();
    if (Cout < min_cout || Cin < min_cin || (Fin - 1) / 2 + 1 < 2) return 0;
    return idv_cconv_gauss_supported(Cin, 0, Cout);
}

extern "C" long long idv_cconv_tw2_wfrag_floats(int Cout, int cin_used) {
    const long long cotiles = (Cout + 31) / 32, cpad = (cin_used + TW2_PACK_CI - 1) / TW2_PACK_CI * TW2_PACK_CI;
    return cotiles * (cpad / 2) * 2 * 4096;                   // the Winograd products, the raw taps of the edge workgroups
}

// wino_frag: idv_pack_cconv_wino(transposed = 0) of the same weights; tw_frag: idv_cconv_tw2_wfrag_floats floats
extern "C" int idv_pack_cconv_tw2(const float* wino_frag, int Cout, int cin_used, float* tw_frag, void* stream) {
    if (!wino_frag || !tw_frag || Cout <= 0 || cin_used <= 0) return IDV_EINVAL;
    const int cotiles = (Cout + 31) / 32;
    const int cpad = (cin_used + TW2_PACK_CI - 1) / TW2_PACK_CI * TW2_PACK_CI;
    const long long n = idv_cconv_tw2_wfrag_floats(Cout, cin_used);
    const unsigned blocks = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(pack_cconv_tw2_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, wino_frag, cotiles, cpad * 3, cpad / 2,
                       tw_frag);
    return idv_launch_status();
}

// idv_cconv2d_wino_fwd (transposed = 0, one source, no addend) on the time-Winograd conv kernel: same result up to the rounding of the
// transforms.  wfrag from idv_pack_cconv_tw2, epi / has_fold from idv_pack_cconv_gauss.  16-byte aligned source, Jp % 4 == 0.
// Reference: model/complex_progress.py:8-36 (+ :161-209 and pvae_module.py:58 for the epilogue).
extern "C" int idv_cconv2d_tw_fwd(const float* x0, int Cin, const float* wfrag, const float* epi, int has_fold, const float* prelu_slope,
                                  float* out, double* stats, double* stats_work, int stats_rep, int tshift, int Cout, int Fin, int B, int Tp,
                                  int Jp, int t_valid_out, void* stream) {
    if (!x0 || !wfrag || !epi || !out || Cin <= 0 || Cout <= 0 || Fin <= 0 || B <= 0 || Tp <= 1) return IDV_EINVAL;
    const EpiStatsTarget sums{stats, stats_work, stats_rep};
    if (!sums.ok()) return IDV_EINVAL;
    if (tshift != 0 && tshift != -1) return IDV_EINVAL;
    if (!idv_cconv_tw2_supported(Cin, Cout, Fin)) return IDV_EINVAL;
    if ((Jp & 3) || (reinterpret_cast<uintptr_t>(x0) & 15) || (reinterpret_cast<uintptr_t>(out) & 7)) return IDV_EINVAL;
    Tw2Args a{};
    a.x0 = x0; a.Cin = Cin;
    a.Fin = Fin; a.Fout = (Fin - 1) / 2 + 1;
    a.J = B * Tp; a.Jp = Jp; a.Tp = Tp;
    a.wfrag = wfrag; a.UP = (Cin + TW2_PACK_CI - 1) / TW2_PACK_CI * TW2_PACK_CI / 2;
    a.epi = epi; a.has_fold = has_fold; a.slope = prelu_slope; a.out = out;
    a.Cout = Cout; a.cotiles = (Cout + 31) / 32;
    a.tshift = tshift; a.t_valid = t_valid_out;
    if (Jp < a.J) return IDV_EINVAL;
    if ((long long)4 * 4 * Fin * (long long)Jp >= 0xffffffffLL) return IDV_EINVAL;   // (the staging's 32-bit byte offsets)
    hipStream_t st = (hipStream_t)stream;
    sums.set(a);
    int rc;
    // two co tiles per workgroup (idv_tw_pair bit IDV_TW_PAIR_CONV): an even number of co tiles
    const bool pair = a.cotiles % 2 == 0 && (idv_tw_pair(-1) & IDV_TW_PAIR_CONV);
    switch ((stats ? 4 : 0) | (pair ? 2 : 0) | (tshift ? 1 : 0)) {
        case 0: rc = launch_tw2<false, false, 1>(a, st); break;
        case 1: rc = launch_tw2<true, false, 1>(a, st); break;
        case 2: rc = launch_tw2<false, false, 2>(a, st); break;
        case 3: rc = launch_tw2<true, false, 2>(a, st); break;
        case 4: rc = launch_tw2<false, true, 1>(a, st); break;
        case 5: rc = launch_tw2<true, true, 1>(a, st); break;
        case 6: rc = launch_tw2<false, true, 2>(a, st); break;
        default: rc = launch_tw2<true, true, 2>(a, st); break;
    }
    return sums.finish(rc, Cout, st);
}
