"""CPU test of the staging address function of the time-Winograd kernels (csrc/cgemm_tw_stage.hpp, the text csrc/cgemm_tw.hip and
csrc/cgemm_tw2.hip compile), built into a small stand-alone host program that enumerates every staging item of every chunk of every
tile and checks each address against its bounds:

  shapes     Fin 3 / 5 / 9; J = 64, 128, 129 columns at pitch Jp = J rounded up to 4; one source (12 channels: a ragged last chunk) and,
             transposed form, two sources (8 + 12 channels: the second one ragged); taps on either side; every full tile (column
             block, row pair) and every edge tile (pair of column blocks) of the shape; every thread slot of both workgroup sizes, the
             slots without an item included.
  global     the offset a lane loads from is the kernel's choice: the dummy for a dead channel (at or past the chunk's valid
             channels), else the item's.  Transposed form (both row phases; byte offsets, and the float offsets of the unpaired
             odd-row kernel): the 16-byte vector is 16-byte aligned and it and the 4-byte extra column lie inside the source's real
             plane from the chunk's base (so the imaginary loads lie inside the imaginary plane).  Conv form: the vector (from 4
             bytes in front of the offset with the taps on the left) and the float behind it lie inside the tensor but for the one
             float in front of or behind it that the kernel documents (the slack of a planar buffer) -- and that float is masked.
  masked     an item whose row lies outside the tensor, or that does not exist, loads the dummy; a valid window column lies inside
             [0, J) of a row inside the tensor.
  LDS        an existing item's stores (four 16-byte plane pairs, the 8-byte plane 8) lie inside its patch buffer of CIK x NRAW x 288
             floats (conv form with two co tiles: the thread slots past the last item inside the dump row behind it), 16- and
             8-byte aligned, and no two items of a chunk overlap."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dccrn-vae_amd", "csrc")
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <set>
#include "cgemm_tw_stage.hpp"

static long bad = 0, seen = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } ++bad; } } while (0)

// one chunk of one tile: items e = 0 .. nslots - 1 (thread slots; e >= nitem: no item)
static void chunk_tw(int ph, bool left, bool edge, int Fin, int J, int Jp, int j0, int rbase, long C, long ci0, int cvalid, unsigned unit,
                     int nslots) {
    const int nraw = ph == 0 ? 4 : 3, cik = 8, nitem = cik * nraw * 16, ne = cik * nraw * 288;
    const long plane = C * Fin * Jp * 4, base = ci0 * Fin * Jp * 4;            // bytes; the chunk's row base inside the real plane
    std::set<unsigned> used;
    for (int e = 0; e < nslots; ++e) {
        const TwStageItem it = tw_stage_item(e, nraw, nitem, left, edge, Fin, J, Jp, j0, rbase, unit);
        ++seen;
        const bool exists = e < nitem, dead = it.cl >= cvalid;
        CHECK(((it.mask >> 7) & 1u) == (unsigned)exists, "e %d", e);
        const long ov = (dead ? (long)unit * TW_DUMMY : (long)it.off_v) * (4 / unit), oe = (dead ? (long)unit * TW_DUMMY : (long)it.off_e) * (4 / unit);
        CHECK(ov % 16 == 0 && base + ov >= 0 && base + ov + 16 <= plane, "ph %d Fin %d J %d j0 %d rbase %d ci0 %ld e %d ov %ld plane %ld", ph, Fin, J, j0, rbase, ci0, e, ov, plane);
        CHECK(base + oe >= 0 && base + oe + 4 <= plane, "ph %d Fin %d J %d j0 %d e %d oe %ld", ph, Fin, J, j0, e, oe);
        const int rl = (e >> 4) % nraw, c8 = e & 15;
        const int f = edge ? Fin - 2 + (rl & 1) : rbase + rl, jc = j0 + (edge ? 64 * (rl >> 1) : 0) + 4 * c8;
        const bool rowok = exists && f >= 0 && f < Fin;
        CHECK(((it.mask >> 5) & 1u) == (unsigned)rowok, "row bit e %d", e);
        if (!rowok) CHECK(it.off_v == unit * TW_DUMMY && it.off_e == unit * TW_DUMMY, "masked item off the dummy e %d", e);
        for (int q = 0; q < 5; ++q)
            if ((it.mask >> q) & 1u) {
                const int c = jc + q - (left ? 1 : 0);
                CHECK(c >= 0 && c < J && c < Jp, "column bit q %d c %d", q, c);
                if (rowok && !dead) {       // the float the lane uses for that column is the tensor's (cl, f, c)
                    const long want = (((long)it.cl * Fin + f) * Jp + c) * 4;
                    const long got = (left ? (q == 0 ? oe : ov + 4 * (q - 1)) : (q == 4 ? oe : ov + 4 * q));
                    CHECK(got == want, "window column q %d: %ld for %ld", q, got, want);
                }
            }
        if (exists) {
            CHECK(it.ldsoff % 4 == 0 && it.ldsoff + 3 * 64 + 4 <= (unsigned)ne, "plane pairs e %d ldsoff %u", e, it.ldsoff);
            const unsigned p8 = it.ldsoff - 2 * c8 + 256;
            CHECK(p8 % 2 == 0 && p8 + 2 <= (unsigned)ne && p8 / 288 == it.ldsoff / 288, "plane 8 e %d", e);
            CHECK(used.insert(it.ldsoff).second, "two items on one LDS slot e %d", e);
        }
    }
}

static void chunk_tw2(bool left, bool edge, int Fin, int J, int Jp, int j0, int rbase, long C, long ci0, int cvalid, bool dump, int nslots) {
    const int nraw = 7, cik = 4, nitem = cik * nraw * 16, ne = cik * nraw * 288, neb = dump ? ne + 288 : ne;
    const long total = 2 * C * Fin * Jp * 4;
    std::set<unsigned> used;
    for (int e = 0; e < nslots; ++e) {
        const TwStageItem it = tw2_stage_item(e, nitem, dump, left, edge, Fin, J, Jp, j0, rbase);
        ++seen;
        const bool exists = e < nitem, dead = it.cl >= cvalid;
        const long ov = dead ? 4L * TW2_DUMMY : (long)it.off_v;
        const int rl = (dump && e >= nitem) ? 0 : (e >> 4) % nraw, c8 = e & 15;
        const int f = edge ? (rl < 6 ? Fin - 3 + rl % 3 : -1) : rbase + rl, jc = j0 + (edge && rl >= 3 ? 64 : 0) + 4 * c8;
        const bool rowok = exists && f >= 0 && f < Fin;
        CHECK(((it.mask >> 5) & 1u) == (unsigned)rowok, "row bit e %d", e);
        if (!rowok) CHECK(it.off_v == 4u * TW2_DUMMY, "masked item off the dummy e %d", e);
        for (int pl = 0; pl < 2; ++pl) {                      // real and imaginary row base of the chunk
            const long base = (pl * C + ci0) * Fin * Jp * 4;
            const long lo = base + ov - (left ? 4 : 0), hi = lo + 20;
            CHECK(ov % 16 == 0 && lo >= -4 && hi <= total + 4, "Fin %d J %d j0 %d rbase %d ci0 %ld e %d lo %ld hi %ld total %ld", Fin, J, j0, rbase, ci0, e, lo, hi, total);
            for (int q = 0; q < 5; ++q)
                if (((it.mask >> q) & 1u) && rowok && !dead) {
                    const int c = jc + q - (left ? 1 : 0);
                    const long at = lo + 4 * q, want = ((pl * C + ci0 + it.cl) * Fin + f) * (long)Jp * 4 + 4L * c;
                    CHECK(c >= 0 && c < J && at == want && at >= 0 && at + 4 <= total, "window column q %d c %d: %ld for %ld", q, c, at, want);
                }
        }
        // every thread slot stores (the slots past the last item into the dump row)
        if (exists || dump) {
            CHECK(it.ldsoff % 4 == 0 && it.ldsoff + 3 * 64 + 4 <= (unsigned)neb, "plane pairs e %d ldsoff %u", e, it.ldsoff);
            const unsigned p8 = it.ldsoff - 2 * c8 + 256;
            CHECK(p8 % 2 == 0 && p8 + 2 <= (unsigned)neb && p8 / 288 == it.ldsoff / 288, "plane 8 e %d", e);
            if (exists) CHECK(it.ldsoff + 288 - 4 * c8 <= (unsigned)ne, "an item inside the patch buffer e %d", e);
            else CHECK(it.ldsoff >= (unsigned)ne, "a slot without an item in the dump row e %d", e);
            if (exists) CHECK(used.insert(it.ldsoff).second, "two items on one LDS slot e %d", e);
        } else {
            CHECK(!dump && e >= nitem, "e %d", e);
        }
    }
}

int main() {
    const int fins[3] = {3, 5, 9}, js[3] = {64, 128, 129};
    for (int Fin : fins)
        for (int J : js) {
            const int Jp = (J + 3) / 4 * 4, jtiles = (J + 63) / 64;
            for (int left = 0; left < 2; ++left) {
                // ---- transposed form: sources (C0, C1) = (12, 0) and (8, 12); chunks of 8 channels, none straddles the sources
                for (int two = 0; two < 2; ++two) {
                    const long C0 = two ? 8 : 12, C1 = two ? 12 : 0, Cin = C0 + C1;
                    for (long ci0 = 0; ci0 < Cin; ci0 += 8) {
                        const bool from0 = ci0 < C0;
                        const long C = from0 ? C0 : C1, local = from0 ? ci0 : ci0 - C0;
                        const int cvalid = (int)((from0 ? C0 : Cin) - ci0);
                        for (int ph = 0; ph < 2; ++ph)
                            for (int nslots : {512, 1024})     // NLD x NTHR of one and of two co tiles per workgroup (NLD = 2)
                                for (int jt = 0; jt < jtiles; ++jt) {
                                    for (int ft = 0; ft <= Fin / 2; ++ft)
                                        for (unsigned unit : {4u, 1u})
                                            chunk_tw(ph, left, false, Fin, J, Jp, jt * 64, 2 * ft - 1 + ph, C, local, cvalid, unit, nslots);
                                    if (ph == 0 && (Fin & 1) && !(jt & 1)) chunk_tw(0, left, true, Fin, J, Jp, jt * 64, 0, C, local, cvalid, 4u, nslots);
                                }
                    }
                }
                // ---- conv form: 10 channels (chunks of 4: the last one ragged), Fout = (Fin + 1) / 2 output rows in pairs
                const long Cin = 10;
                const int Fout = (Fin + 1) / 2;
                for (long ci0 = 0; ci0 < Cin; ci0 += 4)
                    for (int dump = 0; dump < 2; ++dump)
                        for (int jt = 0; jt < jtiles; ++jt) {
                            for (int ft = 0; ft <= Fout / 2; ++ft)
                                chunk_tw2(left, false, Fin, J, Jp, jt * 64, 2 * (2 * ft) - 2, Cin, ci0, (int)(Cin - ci0), dump, 512);
                            if ((Fout & 1) && !(jt & 1)) chunk_tw2(left, true, Fin, J, Jp, jt * 64, 0, Cin, ci0, (int)(Cin - ci0), dump, 512);
                        }
            }
        }
    printf("items %ld bad %ld\n", seen, bad);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    if not os.path.exists(G.HIPCC):
        pytest.skip("no hipcc here")
    d = tmp_path_factory.mktemp("tw_addr")
    src, exe = d / "tw_addr_enum.hip", d / "tw_addr_enum"
    src.write_text(PROGRAM)
    # host code only: no device pass, nothing of the GPU runtime is used
    subprocess.run([G.HIPCC, "-O1", "-std=c++17", "--offload-host-only", "-I", CSRC, str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_every_staging_address_is_in_bounds(result):
    print(result.stdout[-3000:])
    last = result.stdout.strip().splitlines()[-1].split()
    assert result.returncode == 0 and last[0] == "items" and int(last[1]) > 100000 and int(last[3]) == 0, result.stdout[-3000:] + result.stderr


def test_the_kernels_compile_this_text():
    """Both kernels take their item from the header and keep no copy of the address arithmetic."""
    for name, fn in (("cgemm_tw.hip", "tw_stage_item("), ("cgemm_tw2.hip", "tw2_stage_item(")):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "cgemm_tw_stage.hpp"' in text and fn in text, name
        assert "* a.Jp + jcv" not in text, name
