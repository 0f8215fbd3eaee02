// The staging address function of the time-Winograd kernels (cgemm_tw.hip, cgemm_tw2.hip): staging item e of a chunk -> the offsets its
// loads take from the chunk's row bases, the LDS offset of its stores and its validity mask.  Plain integer code for host and device
// alike, as cgemm_tw_map.hpp: the kernels and a host program (tests/test_tw_addr_host.py, which enumerates every item of every chunk
// against the tensors' and the allocation's bounds) share this one text.
//
// An item = (channel cl of the chunk, raw row slot rl, column pairs 2 c8, 2 c8 + 1): e = (cl * NRAW + rl) * 16 + c8.  Its loads: one
// 16-byte vector at off_v and the fifth window column (4 bytes) at off_e (transposed form) or at the vector's start + 16 (conv form,
// whose vector starts 4 bytes in front of off_v with the taps on the left), from the real and the imaginary row base of the chunk.
// Offsets are in units of `unit` bytes: 4 (byte offsets; 32 Fin Jp < 2^32 is the launchers' check) or 1 (float offsets).  A masked
// item (no such item, row outside the tensor) or, chosen per chunk by the kernel, a dead channel loads a dummy that lies inside the
// tensor whatever the shape: TW_DUMMY floats from the base.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TW_SHD __host__ __device__
#else
#define TW_SHD
#endif

struct TwStageItem {
    unsigned off_v, off_e;   // load offsets (off_e: transposed form only)
    unsigned ldsoff;         // floats from the patch buffer: the item's raw row slot and column pairs
    unsigned mask;           // bits 0-4: window column valid; bit 5: row valid; bit 7: item exists
    int cl;                  // channel of the chunk
};

constexpr unsigned TW_DUMMY = 0;    // transposed form: the first float of the chunk
constexpr unsigned TW2_DUMMY = 4;   // conv form: the second 16-byte slot (its vector may start one float in front)

// transposed form (cgemm_tw.hip): NRAW = 4 (even-row phase) | 3 raw rows rbase .. ; edge workgroup: raw slot rl holds (column block
// jt + (rl >> 1), row Fin - 2 + (rl & 1))
TW_SHD inline TwStageItem tw_stage_item(int e, int nraw, int nitem, bool left, bool edge, int Fin, int J, int Jp, int j0, int rbase,
                                        unsigned unit) {
    TwStageItem it;
    const int c8 = e & 15;
    const int rl = (e >> 4) % nraw, cl = e / (16 * nraw);
    it.cl = cl;
    const int f = edge ? Fin - 2 + (rl & 1) : rbase + rl;
    const int jc = j0 + (edge ? 64 * (rl >> 1) : 0) + 4 * c8;
    const int je = left ? jc - 1 : jc + 4;
    const bool exists = e < nitem;
    const bool okr = exists && f >= 0 && f < Fin;
    unsigned m = 0;
    for (int q = 0; q < 5; ++q) {
        const int c = jc + q + (left ? -1 : 0);
        if (c >= 0 && c < J) m |= 1u << q;
    }
    if (okr) m |= 1u << 5;
    if (exists) m |= 1u << 7;
    // addresses stay inside mapped memory whatever the masks say: vector slot clamped to the row, the extra column to [0, Jp)
    const int jcv = jc + 3 < Jp ? jc : 0;
    const int jev = (je >= 0 && je < Jp) ? je : 0;
    it.off_v = okr ? unit * (unsigned)((cl * Fin + f) * Jp + jcv) : unit * TW_DUMMY;
    it.off_e = okr ? unit * (unsigned)((cl * Fin + f) * Jp + jev) : unit * TW_DUMMY;
    if (jc + 3 >= Jp) m &= ~0x1fu;                            // (a column block past the row pitch: nothing valid)
    if (!(je >= 0 && je < Jp)) m &= left ? ~1u : ~(1u << 4);
    it.mask = m;
    it.ldsoff = (unsigned)((cl * nraw + rl) * 288 + 4 * c8);
    return it;
}

// conv form (cgemm_tw2.hip): seven raw rows rbase .. ; edge workgroup: raw slot rl < 6 holds (column block jt + rl / 3, row Fin - 3 +
// rl % 3), slot 6 nothing.  dump: two co tiles per workgroup, where the threads past the last item stage a dead item into the dump
// row behind the buffer (channel CIK, row slot 0).  Byte offsets always.
TW_SHD inline TwStageItem tw2_stage_item(int e, int nitem, bool dump, bool left, bool edge, int Fin, int J, int Jp, int j0, int rbase) {
    constexpr int nraw = 7;
    TwStageItem it;
    const int c8 = e & 15;
    const int cl = e / (16 * nraw), rl = (dump && e >= nitem) ? 0 : (e >> 4) % nraw;
    it.cl = cl;
    const int f = edge ? (rl < 6 ? Fin - 3 + rl % 3 : -1) : rbase + rl;
    const int jc = j0 + (edge && rl >= 3 ? 64 : 0) + 4 * c8;
    const int je = left ? jc - 1 : jc + 4;
    const bool exists = e < nitem;
    const bool okr = exists && f >= 0 && f < Fin;
    unsigned m = 0;
    for (int q = 0; q < 5; ++q) {
        const int c = jc + q + (left ? -1 : 0);
        if (c >= 0 && c < J) m |= 1u << q;
    }
    if (okr) m |= 1u << 5;
    // the extra column is loaded at the vector slot's offset - 1 / + 4: one float outside the row at the buffer's edges, inside the
    // slack every planar buffer has in front and behind (masked)
    const int jcv = jc + 3 < Jp ? jc : 0;
    it.off_v = okr ? 4u * (unsigned)((cl * Fin + f) * Jp + jcv) : 4u * TW2_DUMMY;
    it.off_e = 0;
    if (jc + 3 >= Jp) m &= ~0x1fu;
    if (!(je >= 0 && je < Jp)) m &= left ? ~1u : ~(1u << 4);
    it.mask = m;
    it.ldsoff = (unsigned)((cl * nraw + rl) * 288 + 4 * c8);
    return it;
}
