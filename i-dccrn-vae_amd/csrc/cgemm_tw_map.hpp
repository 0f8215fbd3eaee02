// The launch geometry of the time-Winograd transposed conv (cgemm_tw.hip): how many workgroups a row phase launches and which tile
// each of them computes.  Plain integer code for host and device alike, so that a host program can enumerate it
// (tests/test_tw_edge_host.py).
//
// A FULL tile is (column block jt of 64 columns, row tile ft: a pair of input rows, co-tile group ct).  With an odd number of input
// rows the even-row phase has one output row left over, out[2 (Fin - 1)]: Fin / 2 full row tiles and, per TWO adjacent column blocks
// (2 e, 2 e + 1) and co-tile group, one EDGE workgroup for that row.  Edge workgroups last as long as full ones, so they come FIRST
// in the grid, never in its last round.  Both regions are whole rounds of eight blocks: block ids equal mod 8 share an XCD, and with
// xcd_split the co-tile group ct stays on the XCDs = ct (mod cgroups) in either region.
//
// The conv form (cgemm_tw2.hip) has the same geometry over OUTPUT rows: a full row tile is a pair of output rows, and with an odd
// number of output rows whose last row has three real taps (Fin = 2 Fout - 1) that row, out[Fout - 1], goes to edge workgroups
// (tw2_grid).
//
// At the end, for the kernels only: the output recombination both forms' epilogues share (tw_recombine).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TW_HD __host__ __device__
#else
#define TW_HD
#endif

struct TwGrid {
    int jtiles;      // column blocks of 64 columns
    int ftiles;      // full row tiles per column block
    int etiles;      // edge tiles per co-tile group: pairs of column blocks (0: none)
    int cgroups;     // co-tile groups (workgroups per tile)
    int xcd_split;   // the co-tile groups of a column block on different XCDs (cgroups 2, 4 or 8)
};

struct TwTile {
    int jt, ft, ct;  // first column block, row tile (edge: 0), co-tile group
    bool edge;
};

// ph: row phase (0 even output rows, 1 odd)
TW_HD inline TwGrid tw_grid(int ph, int Fin, int J, int cgroups, int want_split) {
    TwGrid g;
    g.jtiles = (J + 63) / 64;
    g.ftiles = Fin / 2;
    g.etiles = (ph == 0 && (Fin & 1)) ? (g.jtiles + 1) / 2 : 0;
    g.cgroups = cgroups;
    g.xcd_split = (want_split && (cgroups == 2 || cgroups == 4 || cgroups == 8)) ? 1 : 0;
    return g;
}

// the conv form: Fout / 2 full row tiles and edge workgroups where Fout is odd and Fin = 2 Fout - 1.  An odd Fout with an even Fin
// keeps its half tile (ftiles = (Fout + 1) / 2): its last row has four real taps, more than an edge workgroup holds for two blocks.
TW_HD inline TwGrid tw2_grid(int Fin, int Fout, int J, int cgroups, int want_split) {
    TwGrid g;
    const bool edge = (Fout & 1) && Fin == 2 * Fout - 1;
    g.jtiles = (J + 63) / 64;
    g.ftiles = edge ? Fout / 2 : (Fout + 1) / 2;
    g.etiles = edge ? (g.jtiles + 1) / 2 : 0;
    g.cgroups = cgroups;
    g.xcd_split = (want_split && (cgroups == 2 || cgroups == 4 || cgroups == 8)) ? 1 : 0;
    return g;
}

// rounds of eight blocks that hold cols x rows x cgroups workgroups
TW_HD inline long long tw_rounds(const TwGrid& g, int cols, int rows) {
    if (g.xcd_split) {
        const int G = 8 / g.cgroups;
        return (long long)((cols + G - 1) / G) * rows;
    }
    return (long long)((cols + 7) / 8) * rows * g.cgroups;
}

TW_HD inline long long tw_grid_blocks(const TwGrid& g) { return 8 * (tw_rounds(g, g.etiles, 1) + tw_rounds(g, g.jtiles, g.ftiles)); }

// block bid -> its tile; false: a block of the padding of a round (no tile)
TW_HD inline bool tw_block_tile(const TwGrid& g, int bid, TwTile& t) {
    const int xcd = bid & 7;
    int slot = bid >> 3;
    const int erounds = (int)tw_rounds(g, g.etiles, 1);
    t.edge = slot < erounds;
    if (!t.edge) slot -= erounds;
    const int rows = t.edge ? 1 : g.ftiles, cols = t.edge ? g.etiles : g.jtiles;
    int col;
    if (g.xcd_split) {
        // 2 / 4 / 8 co-tile groups: group ct always on the XCDs = ct (mod cgroups), so that an XCD streams 1 / cgroups of the layer's
        // taps (2 - 5 MB: its L2 holds them) and the raw rows of a column block are read by cgroups XCDs instead of one
        const int G = 8 / g.cgroups;
        t.ct = xcd % g.cgroups;
        col = (slot / rows) * G + xcd / g.cgroups;
        t.ft = slot - (slot / rows) * rows;
    } else {
        // all (row tile, co-tile group) workgroups of a column block on ONE XCD: they read the same raw input rows
        const int per = g.cgroups * rows;
        col = (slot / per) * 8 + xcd;
        const int rem = slot - (slot / per) * per;
        t.ft = rem / g.cgroups;
        t.ct = rem - t.ft * g.cgroups;
    }
    t.jt = t.edge ? 2 * col : col;
    return col < cols;
}

#if defined(__HIPCC__)
// The inverse time and Gauss transforms of both forms' epilogues: per frequency product r the nine tiles v[r * 9 + g * 3 + tau] (Gauss
// product g, time product tau) -> the output column pair q of the Gauss products, y[g][q], -> real / imaginary part pr[r][q], pi[r][q].
// (The attribute spelled out: a host program that includes this header alone has no __forceinline__.)
template <int NR>
__device__ inline __attribute__((always_inline)) void tw_recombine(const float (&v)[NR * 9], float (&pr)[NR][2], float (&pi)[NR][2]) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        float y[3][2];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float m1 = v[r * 9 + g * 3], m2 = v[r * 9 + g * 3 + 1], m3 = v[r * 9 + g * 3 + 2];
            y[g][0] = m1 + m2;
            y[g][1] = m2 - m3;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            pr[r][q] = y[0][q] - y[2][q];
            pi[r][q] = y[0][q] + y[1][q];
        }
    }
}
#endif
