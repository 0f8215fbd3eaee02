// Both layers of the DCCRN-CL bottleneck LSTM (H = 128, exact fp32; reference ComplexLSTM.forward, model/complex_progress.py:50-74:
// two nn.LSTM(num_layers = 2), each applied to the real and to the imaginary input) in ONE cooperative launch (evaluation, and
// the training forward: the activated gates and cell states idv_lstm_bptt reads are kept).
//
// lstm_coop_f32.hip runs a layer as 641 latency-bound steps of 3.3 us on 64 CUs and needs layer 0 finished before layer 1's
// input projection (a separate GEMM) and recurrence start: 2 x 2.1 ms + 0.6 ms per forward, 5 % of the fp32 headline step
// with 3/4 of the chip idle.  Here layer 1 runs ONE STEP BEHIND layer 0 on its own 4 CUs per (run, 16-sequence tile):
//   * layer-0 workgroups are those of lstm_coop_f32.hip; they additionally publish h0[t] with write-through (sc1) stores
//     (the rows of the [run][T*B][H] buffer the per-layer path writes anyway) and never wait for layer 1;
//   * a layer-1 workgroup keeps its W_ih slice next to its W_hh slice in registers (2 x 64 VGPRs per lane) and computes
//     W_ih h0[t+1] -- an input that layer 0 finished a step earlier -- while its siblings' h1[t] is still in flight, i.e. in
//     the hand-off latency the step is bound by; the hoisted layer-1 projection GEMM disappears.
// Synchronisation is the fence-free hand-off of lstm_pers.hip / lstm_coop_f32.hip (sc1 16-byte stores drained by every
// storing wave, one agent-scope atomic add per workgroup and counter replica behind the workgroup barrier, an sc1 poll,
// sc1 loads behind poll + barrier); all 8 x 4 x tiles workgroups must be resident (one per CU: 84 KB of LDS requested,
// idv_lstm_stack2_f32_supported checks the count against idv_coop_max_workgroups()); bounded spins, NaN poison and the sticky
// status word on time-out (coop.hpp).
//
// PROJ (idv_lstm_stack2_f32_proj): the layer-0 input projection G = W_ih0 x + b runs INSIDE the launch, on the CUs the
// recurrence leaves empty, instead of as two hoisted idv_pw_gemm calls in front of it.  W_ih0 ([8H][K]) does not fit in
// registers, so other workgroups contract it: the grid (one-dimensional then) is the 32 x tiles recurrence workgroups followed
// by P PRODUCER workgroups.  G is cut into time chunks of PROJ_CH steps and those into the workgroup tiles of idv_pw_gemm
// (cgemm_tile, the same K loop, hence the same bits); lstm_proj_split.hpp numbers the tiles and says who computes which:
//   * opening phase: every workgroup of the launch takes tiles of the first C0 chunks, grid-strided;
//   * then the recurrence workgroups load their weights and run as above, and the producers go on with the later chunks, in
//     order, never waiting for anybody (on an abort they simply finish);
//   * hand-off, the protocol above: a tile's rows of G are stored write-through (sc1), every wave drains its stores, the
//     workgroup meets and adds one arrival to the CHUNK's counter (counters 2 x groups + c behind the recurrence's); a layer-0
//     workgroup that enters a chunk polls that counter (bounded, abort flag) for the chunk's tile count and reads its rows of G
//     with sc1 loads, issued at the top of the step and used after the reduce.  Layer 1 is untouched.
// The training forward overwrites consumed rows of G with the activated gates: those rows are behind every producer.
#include <cstdlib>
#include "cgemm.hpp"
#include "coop.hpp"
#include "lstm_proj_split.hpp"
#include "../../include/idccrn_hip.h"

namespace idv_stack2 {

typedef int v4i __attribute__((ext_vector_type(4)));

struct Args {
    // PROJ: the projection's operands (idv_pw_gemm's: x planar [2 parts][K][Jp], fragments of W_ih0, bias) and its split
    const float* x;
    const float* wih0;
    const float* bih0;
    int K, Tp, Jp;
    unsigned g_bytes;
    ProjSplit ps;
    const float* g;           // layer-0 gate pre-activations (hoisted input projection), addressing as lstm.hip RecArgs
    long long g_run_z, g_run_s;
    int ldg;
    const float* whh0;        // idv_pack_lstm_hh fp32 fragments: [set][tile = ub*4 + gate][kk][lane]
    const float* wih1;        // W_ih of layer 1 ([4H][H] as well) in the same fragment order
    const float* whh1;
    const float* bias1;       // [2 sets][4H], gate-column order (idv_pack_lstm_ih): b_ih + b_hh of layer 1
    float* h0;                // [4 runs][T*B][H]: layer-0 output, read by the layer-1 workgroups
    unsigned h0_bytes;
    float* hout;              // [4 runs][T*B][H]: layer-1 output
    float* gsave1;            // training forward: activated gates of layer 1 [run][T*B][4H] (layer 0: over g, in place) ...
    float* csave0;            // ... and the cell states [4 runs][T*B][H] of both layers; all three NULL in evaluation
    float* csave1;
    float* hx;                // exchange [2 layers][2 parity][4 runs][Bpad][H] fp32
    unsigned hx_bytes;
    CoopSync cs;              // group = layer * 4 * tiles + run * tiles + tile
    int B, T, Bpad, tiles;
};

constexpr int H = 128, NSL = 4, UPW = 32;          // hidden size, workgroups per (layer, group), units per workgroup
constexpr int MAX_GROUPS = 64, MAX_REP = 8;
constexpr int SYNC_BYTES = idv_coop_sync_bytes(2 * MAX_GROUPS, MAX_REP);
constexpr int PROJ_CCK = 32;                                                   // planes per K chunk of the projection tile
constexpr int RED_FLOATS = 4 * 8 * 4 * 64;                                     // red[]; PROJ: the tile's two patch buffers behind it
constexpr int proj_sync_bytes(int T) { return idv_coop_sync_bytes(2 * MAX_GROUPS + (T + PROJ_CH - 1) / PROJ_CH, MAX_REP); }

// PROJ false: grid (2 NSL, 4 runs, tiles); true: (32 tiles + P), the recurrence workgroups first and in the same linear order
template <bool PROJ>
__global__ __launch_bounds__(256, 1) void lstm_stack2_f32_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float red[];                // [4 waves][8 tiles][4 r][64 lanes]
    __shared__ int abort_sh;
    __shared__ unsigned seen0_sh;                                              // layer 1: layer-0 arrivals last observed
    __shared__ __attribute__((aligned(16))) float stage[16][UPW];              // h_t of this workgroup: [row][unit]
    const __amdgpu_buffer_rsrc_t hxr = __builtin_amdgcn_make_buffer_rsrc((void*)a.hx, 0, a.hx_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t h0r = __builtin_amdgcn_make_buffer_rsrc((void*)a.h0, 0, a.h0_bytes, 0x00020000);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nrec = 2 * NSL * 4 * a.tiles;
    const bool producer = PROJ && (int)blockIdx.x >= nrec;
    const int rid = producer ? 0 : (int)blockIdx.x;                            // PROJ: x + 8 (y + 4 z) of the three-dimensional grid
    const int layer = PROJ ? (rid >> 2) & 1 : blockIdx.x >> 2, sl = blockIdx.x & 3;
    const int run = PROJ ? (rid >> 3) & 3 : blockIdx.y, tile = PROJ ? rid >> 5 : blockIdx.z;
    const int z = run >> 1, s = run & 1;
    const int col = lane & 15, rq = lane >> 4;
    const int b0 = tile * 16;
    unsigned* abortf = idv_coop_abort_flag(a.cs);
    const int groups = 4 * a.tiles, grp = run * a.tiles + tile;
    unsigned* cnt0 = idv_coop_counter(a.cs, 0 * groups + grp);          // layer-0 arrivals of this (run, tile)
    unsigned* cnt1 = idv_coop_counter(a.cs, 1 * groups + grp);
    unsigned* mine = layer ? cnt1 : cnt0;
    const size_t TB = (size_t)a.T * a.B, TBH = TB * H;
    // exchange regions: [layer][parity][run][Bpad][H]
    const unsigned hx_layer = (unsigned)layer * 2u * 4u * (unsigned)a.Bpad * (unsigned)H * 4u;
    const unsigned hx_par = 4u * (unsigned)a.Bpad * (unsigned)H * 4u;

    // PROJ: the tiles of G this workgroup computes -- opening phase (every workgroup), then, producers only, the later chunks
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc((void*)a.g, 0, PROJ ? a.g_bytes : 0u, 0x00020000);
    if constexpr (PROJ) {
        if (idv_coop_withheld(a.cs)) return;
        for (ProjWalk w = proj_walk(a.ps, (int)blockIdx.x, (int)gridDim.x);
             proj_walk_tile(a.ps, w, producer ? (int)blockIdx.x - nrec : -1); w.i += w.stride) {
            const ProjTile pt = proj_tile(a.ps, a.T, w.i);
            CgemmArgs ca{};
            ca.x0 = a.x + (size_t)pt.z * a.K * a.Jp;
            ca.C0 = a.K / 2;
            ca.Fin = 1; ca.Fout = 1;
            ca.J = pt.steps * a.B; ca.Jp = a.Jp; ca.Tp = a.Tp;
            ca.wfrag = a.wih0; ca.bias = a.bih0;
            ca.out = const_cast<float*>(a.g) + (size_t)pt.z * a.g_run_z;
            ca.M = 8 * H; ca.Mtiles = 8 * H / 32; ca.Cout = 8 * H;
            ca.t_valid = a.T; ca.ldo = a.ldg; ca.nB = a.B;
            // idv_pw_gemm's 4 x 1 form with 32 planes per K chunk instead of 8 (the same k order, hence the same bits): this
            // workgroup has the CU to itself, and a chunk of 8 planes (0.43 us of MFMA) is shorter than the latency of its
            // staging loads, which no second workgroup hides here: 133 us per tile against 102 us per tile and CU hoisted
            cgemm_tile<IDV_PW, 4, 1, 2, 1, 2, PROJ_CCK, true, false, false>(ca, red + RED_FLOATS, pt.grp, 0, pt.mb,
                                                                            CgemmTimeChunkCols{pt.t0, pt.steps});
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            idv_coop_arrive(a.cs, idv_coop_counter(a.cs, 2 * groups + pt.chunk), tid);
        }
        if (producer) return;
    }

    // W_hh slice (and, layer 1, the W_ih slice): this workgroup's 8 column tiles (unit blocks 2 sl, 2 sl + 1 x 4 gates), this
    // wave's 32 k, 8 consecutive k per lane (MFMA k-step j of lane (row, kq) is k = 32 w + 8 kq + j) -- as lstm_coop_f32.hip
    float breg[8][8], ireg[8][8];
    {
        const float* wb = (layer ? a.whh1 : a.whh0) + (size_t)s * 4 * H * H;
        const float* wi = a.wih1 + (size_t)s * 4 * H * H;
#pragma unroll
        for (int t8 = 0; t8 < 8; ++t8) {
            const int ctile = (2 * sl + (t8 >> 2)) * 4 + (t8 & 3);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * wave + 8 * rq + j;
                const size_t e = ((size_t)ctile * (H / 4) + (k >> 2)) * 64 + (k & 3) * 16 + col;
                breg[t8][j] = wb[e];
                ireg[t8][j] = layer ? wi[e] : 0.f;
            }
        }
    }
    // cell update split by row over the waves: wave w owns rows rq * 4 + w of both unit blocks (unit = 16 ub + lane & 15)
    const int myrow = rq * 4 + wave;
    const int brow = b0 + myrow;
    const bool rowok = brow < a.B;
    const int bclamp = rowok ? brow : a.B - 1;
    const int lrow = (b0 + col < a.B) ? b0 + col : a.B - 1;       // the row this lane supplies to the A operand (clamped)
    float creg[2] = {0.f, 0.f};
    float gb[2][4];                                                // layer 1: the constant part of the gate pre-activations
#pragma unroll
    for (int ub = 0; ub < 2; ++ub)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) gb[ub][gg] = layer ? a.bias1[(size_t)s * 4 * H + (2 * sl + ub) * 64 + 16 * gg + col] : 0.f;
    const float* g = a.g + z * a.g_run_z + s * a.g_run_s;
    // training forward: where this workgroup keeps its activated gates (row pitch gld) and cell states
    float* gsv = !a.csave0 ? nullptr : (layer ? a.gsave1 + (size_t)run * TB * 4 * H : const_cast<float*>(g));
    const int gld = layer ? 4 * H : a.ldg;
    float* csv = layer ? a.csave1 : a.csave0;

    bool aborted = false;
    if (tid == 0) { abort_sh = 0; seen0_sh = 0; }
    if (idv_coop_withheld(a.cs)) return;
    __syncthreads();

    // layer 1: the rows of h0[t] for the CURRENT step sit in registers (cur0, cur1) when the step starts; W_ih h0[t] is
    // contracted while the loads of h1[t-1] are in flight, so it costs no time of its own.  Layer 0 runs ahead (its step is
    // shorter): its arrival count is polled only when the cached one does not cover the step, and the rows of h0[t+1] are
    // requested EARLY -- before this step's own stores and arrive.
    auto input_known = [&](int tt) -> bool { return seen0_sh >= (unsigned)(tt + 1) * (unsigned)NSL; };       // uniform
    auto input_load = [&](int tt, f32x4& a0, f32x4& a1) {
        const unsigned off = (unsigned)((((size_t)run * TB + (size_t)tt * a.B + lrow) * H + 32 * wave + 8 * rq) * 4u);
        a0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(h0r, off, 0, 16));
        a1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(h0r, off + 16u, 0, 16));
    };
    auto input_late = [&](int tt, f32x4& a0, f32x4& a1) -> bool {            // poll layer 0, then load
        if (tid == 0) idv_coop_wait(idv_coop_replica(a.cs, cnt0, sl), (unsigned)(tt + 1) * (unsigned)NSL, abortf, &abort_sh, &seen0_sh);
        __syncthreads();
        if (abort_sh) return false;
        input_load(tt, a0, a1);
        return true;
    };
    f32x4 cur0 = {0.f, 0.f, 0.f, 0.f}, cur1 = {0.f, 0.f, 0.f, 0.f};
    if (layer && !input_late(0, cur0, cur1)) aborted = true;

    for (int t = 0; t < a.T && !aborted; ++t) {
        float gpre[2][4];
        if (layer == 0) {
            if constexpr (PROJ) {
                // a new chunk: all of its tiles must have arrived; then sc1 loads (the rows were stored inside this launch)
                if (t % PROJ_CH == 0) {
                    const int c = t / PROJ_CH;
                    if (tid == 0)
                        idv_coop_wait(idv_coop_replica(a.cs, idv_coop_counter(a.cs, 2 * groups + c), sl),
                                      (unsigned)proj_chunk_tiles(a.B, a.T, c), abortf, &abort_sh);
                    __syncthreads();
                    if (abort_sh) { aborted = true; break; }
                }
                const unsigned off = (unsigned)(((size_t)z * a.g_run_z + (size_t)s * a.g_run_s + ((size_t)t * a.B + bclamp) * a.ldg +
                                                 (2 * sl) * 64 + col) * 4u);
#pragma unroll
                for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                    for (int gg = 0; gg < 4; ++gg)
                        gpre[ub][gg] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(gr, off + (ub * 64 + 16 * gg) * 4u, 0, 16));
            } else {
                const float* gp = g + ((size_t)t * a.B + bclamp) * a.ldg + (2 * sl) * 64 + col;
#pragma unroll
                for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                    for (int gg = 0; gg < 4; ++gg) gpre[ub][gg] = gp[ub * 64 + 16 * gg];
            }
        } else {
#pragma unroll
            for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) gpre[ub][gg] = gb[ub][gg];
        }
        f32x4 acc[8];
#pragma unroll
        for (int t8 = 0; t8 < 8; ++t8)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t8][r] = 0.f;
        auto input_mfma = [&]() {                 // layer 1: acc += W_ih h0[t]
            float av[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                av[j] = cur0[j];
                av[4 + j] = cur1[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int t8 = 0; t8 < 8; ++t8)
                    acc[t8] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], ireg[t8][j], acc[t8], 0, 0, 0);
        };
        if (layer && t == 0) input_mfma();
        if (t > 0) {
            if (tid == 0)       // (layer 1: the view of layer 0's progress is refreshed while waiting for the siblings, if it waits)
                idv_coop_wait(idv_coop_replica(a.cs, mine, sl), (unsigned)t * (unsigned)NSL, abortf, &abort_sh, nullptr,
                              layer ? idv_coop_replica(a.cs, cnt0, sl) : nullptr, &seen0_sh);
            __syncthreads();                 // the polling wave joins after its match; every load below is sc1
            if (abort_sh) { aborted = true; break; }
            const unsigned par_r = hx_layer + (unsigned)((t - 1) & 1) * hx_par;
            const unsigned off = (((unsigned)run * a.Bpad + b0 + col) * (unsigned)H + 32 * wave + 8 * rq) * 4u;
            const f32x4 a0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(hxr, off, par_r, 16));
            const f32x4 a1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(hxr, off + 16u, par_r, 16));
            if (layer) input_mfma();         // under the latency of the two loads above
            float av[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                av[j] = a0[j];
                av[4 + j] = a1[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int t8 = 0; t8 < 8; ++t8)
                    acc[t8] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], breg[t8][j], acc[t8], 0, 0, 0);
        }
        // layer 1: the next step's input rows, if layer 0 is known to have published them (it usually is)
        const bool early = layer && t + 1 < a.T && input_known(t + 1);
        f32x4 nx0 = {0.f, 0.f, 0.f, 0.f}, nx1 = {0.f, 0.f, 0.f, 0.f};
        if (early) input_load(t + 1, nx0, nx1);
        // ---- reduce the 4 K-partials through LDS: [wave][tile][r][lane], conflict-free dword writes and reads
#pragma unroll
        for (int t8 = 0; t8 < 8; ++t8)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(((wave * 8 + t8) * 4 + r) << 6) + lane] = acc[t8][r];
        __syncthreads();
#pragma unroll
        for (int ub = 0; ub < 2; ++ub) {
            float gate[4];
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                float v = gpre[ub][gg];
#pragma unroll
                for (int w = 0; w < 4; ++w) v += red[(((w * 8 + ub * 4 + gg) * 4 + wave) << 6) + lane];
                gate[gg] = v;
            }
            const float ig = sigmoidf_(gate[0]), fg = sigmoidf_(gate[1]);
            const float gv = tanhf_(gate[2]), og = sigmoidf_(gate[3]);
            const float cn = fg * creg[ub] + ig * gv;
            creg[ub] = cn;
            stage[myrow][ub * 16 + col] = og * tanhf_(cn);
            if (gsv && rowok) {
                float* gp = gsv + ((size_t)t * a.B + brow) * gld + (2 * sl + ub) * 64 + col;
                gp[0] = ig; gp[16] = fg; gp[32] = gv; gp[48] = og;
                csv[(size_t)run * TBH + ((size_t)t * a.B + brow) * H + sl * UPW + ub * 16 + col] = cn;
            }
        }
        __syncthreads();
        if (tid < 128) {
            // 16 rows x 8 float4: write-through (sc1) to the exchange buffer; the sequence output plain (layer 1) or, layer 0,
            // write-through as well: the layer-1 workgroups of this (run, tile) read it
            const int row = tid >> 3, c4 = tid & 7;
            const v4i pk = *(const v4i*)&stage[row][c4 * 4];
            const unsigned par_w = hx_layer + (unsigned)(t & 1) * hx_par;
            const unsigned off = (((unsigned)run * a.Bpad + b0 + row) * (unsigned)H + sl * UPW + c4 * 4) * 4u;
            __builtin_amdgcn_raw_buffer_store_b128(pk, hxr, off, par_w, 16);       // aux 16 = sc1
            if (b0 + row < a.B) {
                const size_t e = (size_t)run * TBH + ((size_t)t * a.B + b0 + row) * H + sl * UPW + c4 * 4;
                if (layer) *(v4i*)&a.hout[e] = pk;
                else __builtin_amdgcn_raw_buffer_store_b128(pk, h0r, (unsigned)(e * 4u), 0, 16);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        idv_coop_arrive(a.cs, mine, tid);
        // layer 1: the next step's input rows, the late way, if they were not requested above
        if (layer && t + 1 < a.T) {
            if (!early && !input_late(t + 1, nx0, nx1)) aborted = true;
            cur0 = nx0; cur1 = nx1;
        }
    }
    if (aborted) {
        if (tid == 0) idv_coop_raise(a.cs.status);
        if (layer) {
            const float qnan = __builtin_nanf("");
            for (long long e = tid; e < (long long)a.T * 16 * UPW; e += 256) {
                const int u = (int)(e % UPW), br = (int)((e / UPW) & 15);
                const long long t = e / (UPW * 16);
                if (b0 + br < a.B) a.hout[(size_t)run * TBH + ((size_t)t * a.B + b0 + br) * H + sl * UPW + u] = qnan;
            }
        }
    }
}

}  // namespace idv_stack2


extern "C" int idv_lstm_stack2_f32_supported(int H, int B) {
    static const bool on = [] { const char* e = getenv("IDV_LSTM_STACK2"); return !e || e[0] != '0'; }();
    if (!on || H != 128 || B <= 0) return 0;
    const int tiles = (B + 15) / 16;
    return 4 * tiles <= idv_stack2::MAX_GROUPS && 2 * 4 * 4 * tiles <= idv_coop_max_workgroups();      // all resident, one per CU
}

extern "C" long long idv_lstm_stack2_f32_work_bytes(int H, int B) {
    const long long Bpad = (B + 15) / 16 * 16;
    return idv_stack2::SYNC_BYTES + 2LL * 2 * 4 * Bpad * H * 4;
}

// Both layers of the H = 128 complex LSTM in one cooperative launch.  g: layer-0 gate pre-activations as for
// idv_lstm_rec_coop_f32; whh0 / wih1_hh / whh1: idv_pack_lstm_hh fragments (W_ih of layer 1 is [4H][H] too); bias1: [2][4H] in
// gate-column order (idv_pack_lstm_ih of layer 1); h0, hout: [4 runs][T*B][H]; work: idv_lstm_stack2_f32_work_bytes bytes.
// Training forward: gsave1 ([run][T*B][4H]), csave0, csave1 ([4 runs][T*B][H]) all non-NULL -- the activated gates of layer 0
// replace its pre-activations in g, those of layer 1 go to gsave1 (the layouts idv_lstm_bptt reads); evaluation: all NULL.
extern "C" int idv_lstm_stack2_f32(const float* g, long long g_run_z, long long g_run_s, int ldg, const float* whh0, const float* wih1_hh,
                                   const float* whh1, const float* bias1, float* h0, float* hout, int H, int B, int T, void* work,
                                   float* gsave1, float* csave0, float* csave1, void* stream) {
    using namespace idv_stack2;
    if (!g || !whh0 || !wih1_hh || !whh1 || !bias1 || !h0 || !hout || !work || T <= 0 || !idv_lstm_stack2_f32_supported(H, B))
        return IDV_EINVAL;
    if ((gsave1 != nullptr) != (csave0 != nullptr) || (csave0 != nullptr) != (csave1 != nullptr)) return IDV_EINVAL;
    if ((reinterpret_cast<uintptr_t>(work) & 15) || (reinterpret_cast<uintptr_t>(h0) & 15) || (reinterpret_cast<uintptr_t>(hout) & 15))
        return IDV_EINVAL;
    const long long h0_bytes = 4LL * T * B * H * 4;
    if (h0_bytes >= 0xfffffe00LL) return IDV_EINVAL;          // 32-bit buffer offsets
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (B + 15) / 16;
    const long long Bpad = 16LL * tiles;
    Args a{};
    a.g = g; a.g_run_z = g_run_z; a.g_run_s = g_run_s; a.ldg = ldg;
    a.whh0 = whh0; a.wih1 = wih1_hh; a.whh1 = whh1; a.bias1 = bias1;
    a.h0 = h0; a.h0_bytes = (unsigned)h0_bytes; a.hout = hout;
    a.gsave1 = gsave1; a.csave0 = csave0; a.csave1 = csave1;
    a.hx = (float*)((char*)work + SYNC_BYTES);
    a.hx_bytes = (unsigned)(2LL * 2 * 4 * Bpad * H * 4);
    a.cs.nrep = 4;
    a.B = B; a.T = T; a.Bpad = (int)Bpad; a.tiles = tiles;
    const size_t smem = 84 * 1024;                   // > half a CU's LDS: one workgroup per CU (red[] needs 32 KB)
    return idv_coop_launch(lstm_stack2_f32_kernel<false>, dim3(2 * NSL, 4, tiles), smem, st, work, SYNC_BYTES, a);
}

// ---- the layer-0 projection inside the launch ----------------------------------------------------------------------------------
// 1: idv_lstm_stack2_f32_proj takes (H, B, T, K); *c0 / *P (may be NULL): chunks of the opening phase and producer workgroups.
// 0: no room for producers beside the recurrence (large B), every chunk in the opening phase (short T), a G beyond 32-bit
// buffer offsets, or IDV_LSTM_PROJ_OVERLAP=0 -- the projection stays hoisted (idv_pw_gemm in front of idv_lstm_stack2_f32).
// force_c0: -1 automatic; tests: 0 .. chunks (clamped), the opening phase (the chunk count: all of G in it, one idle producer).
extern "C" int idv_lstm_stack2_f32_proj_split(int H, int B, int T, int K, int force_c0, int* c0, int* P) {
    static const bool on = [] { const char* e = getenv("IDV_LSTM_PROJ_OVERLAP"); return !e || e[0] != '0'; }();
    if (c0) *c0 = 0;
    if (P) *P = 0;
    if (!on || T <= 0 || K <= 0 || (K & 1) || !idv_lstm_stack2_f32_supported(H, B)) return 0;
    if (64LL * T * B * H >= 0xfffffe00LL) return 0;
    const ProjSplit ps = proj_split(B, T, K, 2 * 4 * 4 * ((B + 15) / 16), idv_coop_max_workgroups(), force_c0);
    if (c0) *c0 = ps.c0;
    if (P) *P = ps.P;
    return ps.P > 0;
}

// sync words (with one counter per chunk of Tmax steps) + the exchange buffers
extern "C" long long idv_lstm_stack2_f32_proj_work_bytes(int H, int B, int Tmax) {
    const long long Bpad = (B + 15) / 16 * 16;
    return idv_stack2::proj_sync_bytes(Tmax < 1 ? 1 : Tmax) + 2LL * 2 * 4 * Bpad * H * 4;
}

// idv_lstm_stack2_f32 that computes G itself: x planar [2 parts][K planes][Jp] (column b Tp + 1 + t), wih0 / bih0: idv_pack_lstm_ih
// of layer 0 (both weight sets, M = 8H); g: [2 parts][T*B][8H], written and (training forward) overwritten with the activated
// gates exactly as by idv_pw_gemm + idv_lstm_stack2_f32; work: idv_lstm_stack2_f32_proj_work_bytes(H, B, Tmax >= T) bytes.
// IDV_EINVAL where idv_lstm_stack2_f32_proj_split says 0.
extern "C" int idv_lstm_stack2_f32_proj(const float* x, int K, int Tp, int Jp, const float* wih0, const float* bih0, float* g,
                                        const float* whh0, const float* wih1_hh, const float* whh1, const float* bias1, float* h0,
                                        float* hout, int H, int B, int T, void* work, float* gsave1, float* csave0, float* csave1,
                                        int force_c0, void* stream) {
    using namespace idv_stack2;
    if (!x || !wih0 || !bih0 || !g || !whh0 || !wih1_hh || !whh1 || !bias1 || !h0 || !hout || !work || T <= 0 || Tp < T + 1 ||
        (long long)Jp < (long long)B * Tp || !idv_lstm_stack2_f32_proj_split(H, B, T, K, force_c0, nullptr, nullptr))
        return IDV_EINVAL;
    if ((gsave1 != nullptr) != (csave0 != nullptr) || (csave0 != nullptr) != (csave1 != nullptr)) return IDV_EINVAL;
    if ((reinterpret_cast<uintptr_t>(work) & 15) || (reinterpret_cast<uintptr_t>(h0) & 15) || (reinterpret_cast<uintptr_t>(hout) & 15) ||
        (reinterpret_cast<uintptr_t>(g) & 3))
        return IDV_EINVAL;
    const long long TB = (long long)T * B;
    const int tiles = (B + 15) / 16;
    const long long Bpad = 16LL * tiles;
    const int sync_bytes = proj_sync_bytes(T);
    Args a{};
    a.x = x; a.wih0 = wih0; a.bih0 = bih0; a.K = K; a.Tp = Tp; a.Jp = Jp;
    a.g_bytes = (unsigned)(64LL * TB * H);
    a.ps = proj_split(B, T, K, 2 * NSL * 4 * tiles, idv_coop_max_workgroups(), force_c0);
    a.g = g; a.g_run_z = TB * 8 * H; a.g_run_s = 4LL * H; a.ldg = 8 * H;
    a.whh0 = whh0; a.wih1 = wih1_hh; a.whh1 = whh1; a.bias1 = bias1;
    a.h0 = h0; a.h0_bytes = (unsigned)(16LL * TB * H); a.hout = hout;
    a.gsave1 = gsave1; a.csave0 = csave0; a.csave1 = csave1;
    a.hx = (float*)((char*)work + sync_bytes);
    a.hx_bytes = (unsigned)(2LL * 2 * 4 * Bpad * H * 4);
    a.cs.nrep = 4;
    a.B = B; a.T = T; a.Bpad = (int)Bpad; a.tiles = tiles;
    const size_t smem = 84 * 1024;                   // one workgroup per CU: red[] 32 KB, the tile's patch buffers 4.2 KB behind it
    return idv_coop_launch(lstm_stack2_f32_kernel<true>, dim3(2 * NSL * 4 * tiles + a.ps.P), smem, (hipStream_t)stream, work,
                           sync_bytes, a);
}
