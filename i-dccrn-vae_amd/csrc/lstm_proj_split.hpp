// The layer-0 input projection of the H = 128 complex LSTM inside the cooperative launch of lstm_stack2_f32.hip: which tiles of
// G = W_ih0 x + b exist, in which order, and who computes them.  Plain integer code for host and device alike, so that a host
// program can enumerate it (tests/test_lstm_proj_split_host.py).
//
// G is cut along TIME: chunk c = steps [c CH, min(T, (c + 1) CH)).  The steps x B columns of a chunk are flattened utterance-major
// (v = b * steps + (t - c CH): the input columns b Tp + 1 + t of one utterance are contiguous) into groups of 64; a TILE is
// (chunk, group, input part z, block mb of 256 gate rows), the workgroup tile of idv_pw_gemm's 4 x 1 form.  Tiles are numbered
// chunk-major.  All W = recurrence + P workgroups of the launch take the tiles of the first C0 chunks grid-strided (the OPENING
// phase); then the recurrence starts and the P producer workgroups go on with the remaining tiles, strided by P: a producer's
// chunks never decrease, and it never waits.  A layer-0 recurrence workgroup that enters chunk c waits until the chunk's arrive
// counter holds proj_chunk_tiles(c) (one arrive per tile).
//
// C0 comes from a timeline built of the two measured constants below (proj_predict_ns): the opening phase lasts
// ceil(opening tiles / W) tile times (it is quantised: 240 workgroups take 1.9 chunks of B = 64 per round), chunk c >= C0 is
// complete ceil(tiles of [C0, c] / P) tile times later, and the recurrence enters a chunk when it has finished the one before AND
// the chunk is complete -- a late producer only makes the recurrence wait, it never makes it wrong, so the producers need not
// be ahead at every chunk and no safety margin is added to their time: the choice is the opening phase with the shortest
// predicted launch.  Ties within PROJ_TIE_PCT per cent go to the hoisted projection (C0 = every chunk, P = 0: no overlap is
// to be had, e.g. a single chunk) and then to the smallest C0.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROJ_HD __host__ __device__
#else
#define PROJ_HD
#endif

constexpr int PROJ_CH = 16;                 // steps per chunk: 64-byte input segments, ~62 us of recurrence
// measured on one MI355X at B = 64, T = 641, K = 1280 (tests/tools/lstm_proj_probe.py, profiles/lstm_overlap/README.md):
constexpr int PROJ_STEP_NS = 3900;          // one step of lstm_stack2_f32_kernel (2.504 ms / 641 steps in the kernel trace)
constexpr int PROJ_TILE_NS_PER_K = 96;      // one 256 x 64 tile inside the launch, per input plane: 123 us at K = 1280 (a workgroup
                                            // alone on its CU; idv_pw_gemm, several workgroups per CU: 100 us per tile and CU)
constexpr int PROJ_TIE_PCT = 1;

struct ProjSplit {
    int nchunks;        // ceil(T / CH)
    int gfull, glast;   // 64-column groups of a full chunk / of the last chunk
    int c0;             // chunks of the opening phase
    int P;              // producer workgroups (0: the projection stays hoisted)
    long long nopen;    // tiles of the opening phase
    long long ntiles;
};
struct ProjTile {
    int chunk, grp, z, mb;
    int t0, steps;      // first step and steps of the chunk
};

PROJ_HD inline int proj_chunk_steps(int T, int c) { return (c + 1) * PROJ_CH <= T ? PROJ_CH : T - c * PROJ_CH; }
PROJ_HD inline int proj_chunk_groups(int B, int T, int c) { return (proj_chunk_steps(T, c) * B + 63) / 64; }
PROJ_HD inline int proj_chunk_tiles(int B, int T, int c) { return 8 * proj_chunk_groups(B, T, c); }
// tiles in front of chunk c (c <= nchunks)
PROJ_HD inline long long proj_tiles_before(const ProjSplit& s, int c) {
    return c < s.nchunks ? 8LL * s.gfull * c : 8LL * s.gfull * (s.nchunks - 1) + 8LL * s.glast;
}

// producers beside `rec` recurrence workgroups for an opening phase of c0 chunks: what the remaining tiles need, within the bound
PROJ_HD inline int proj_producers(const ProjSplit& s, int c0, int rec, int bound) {
    const long long room = (long long)bound - rec, rest = s.ntiles - proj_tiles_before(s, c0);
    return room <= 0 ? 0 : (int)(rest < room ? rest : room);
}

// predicted duration of the launch with an opening phase of c0 chunks (c0 = chunks: everything in front of the recurrence, on
// `bound` workgroups)
PROJ_HD inline long long proj_predict_ns(const ProjSplit& s, int B, int T, int K, int rec, int bound, int c0) {
    const long long tile_ns = (long long)PROJ_TILE_NS_PER_K * K;
    const long long nopen = proj_tiles_before(s, c0);
    const int P = proj_producers(s, c0, rec, bound);
    const long long W = c0 < s.nchunks ? rec + P : (bound > rec ? bound : rec);
    const long long open = (nopen + W - 1) / W * tile_ns;
    long long t = open;
    for (int c = 0; c < s.nchunks; ++c) {
        if (c >= c0) {
            const long long ready = open + (proj_tiles_before(s, c + 1) - nopen + P - 1) / P * tile_ns;
            if (ready > t) t = ready;
        }
        t += (long long)proj_chunk_steps(T, c) * PROJ_STEP_NS;
    }
    return t;
}

// `rec`: recurrence workgroups of the launch, `bound`: workgroups that may be resident at once, K: input planes per part,
// force_c0: -1 automatic, else the opening phase (clamped to the chunk count; tests)
PROJ_HD inline ProjSplit proj_split(int B, int T, int K, int rec, int bound, int force_c0) {
    ProjSplit s;
    s.nchunks = (T + PROJ_CH - 1) / PROJ_CH;
    s.glast = proj_chunk_groups(B, T, s.nchunks - 1);
    s.gfull = s.nchunks > 1 ? (PROJ_CH * B + 63) / 64 : s.glast;
    s.ntiles = 8LL * s.gfull * (s.nchunks - 1) + 8LL * s.glast;
    s.c0 = s.nchunks;
    s.P = 0;
    s.nopen = s.ntiles;
    if (bound <= rec) return s;
    if (force_c0 >= 0) {
        s.c0 = force_c0 < s.nchunks ? force_c0 : s.nchunks;
        s.P = proj_producers(s, s.c0, rec, bound);
        if (s.P == 0) s.P = 1;          // everything in the opening phase: one (idle) producer, so that the forced path is the fused kernel
    } else {
        long long best = proj_predict_ns(s, B, T, K, rec, bound, 0);
        for (int c = 1; c < s.nchunks; ++c) {
            const long long p = proj_predict_ns(s, B, T, K, rec, bound, c);
            if (p < best) best = p;
        }
        const long long lim = best + best * PROJ_TIE_PCT / 100;
        if (proj_predict_ns(s, B, T, K, rec, bound, s.nchunks) > lim) {
            int c0 = 0;
            while (proj_predict_ns(s, B, T, K, rec, bound, c0) > lim) ++c0;
            s.c0 = c0;
            s.P = proj_producers(s, c0, rec, bound);
        }
    }
    s.nopen = proj_tiles_before(s, s.c0);
    return s;
}

// The tiles of one workgroup, in order: `for (ProjWalk w = proj_walk(s, wg, nwg); proj_walk_tile(s, w, pid); w.i += w.stride)`
// computes tile w.i.  wg: workgroup id in the launch of nwg = rec + P; pid: producer index wg - rec, or -1 in a recurrence
// workgroup (which leaves after the opening phase).
struct ProjWalk {
    long long i, stride, end;
};
PROJ_HD inline ProjWalk proj_walk(const ProjSplit& s, int wg, int nwg) {
    ProjWalk w;
    w.i = wg;
    w.stride = nwg;
    w.end = s.nopen;
    return w;
}
PROJ_HD inline bool proj_walk_tile(const ProjSplit& s, ProjWalk& w, int pid) {
    if (w.i >= w.end) {
        if (pid < 0 || w.end == s.ntiles) return false;
        w.i = s.nopen + pid;                  // the opening phase is over: the later chunks, strided by the producers
        w.stride = s.P;
        w.end = s.ntiles;
        if (w.i >= w.end) return false;
    }
    return true;
}

// tile i of the chunk-major order -> its coordinates: within a chunk the four row blocks of a (group, part) patch are adjacent
PROJ_HD inline ProjTile proj_tile(const ProjSplit& s, int T, long long i) {
    ProjTile t;
    const long long per = 8LL * s.gfull;
    t.chunk = (int)(i / per);
    if (t.chunk >= s.nchunks - 1) t.chunk = s.nchunks - 1;
    const int r = (int)(i - per * t.chunk);
    t.grp = r >> 3;
    t.z = (r >> 2) & 1;
    t.mb = r & 3;
    t.t0 = t.chunk * PROJ_CH;
    t.steps = proj_chunk_steps(T, t.chunk);
    return t;
}
