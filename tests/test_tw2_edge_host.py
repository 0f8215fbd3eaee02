"""CPU test of the launch geometry of the time-Winograd conv form (csrc/cgemm_tw_map.hpp, tw2_grid): the block -> (column block, row
tile or edge, co-tile group) mapping that kernel and launch share, compiled into a small stand-alone host program and enumerated.

For every (Fin, jtiles, cgroups, block order), Fout = (Fin - 1) / 2 + 1 as the conv gives it, the program walks all blocks and checks
  * every full tile (jt, ft, ct) is hit exactly once, and no tile outside the ranges is produced;
  * where Fout is odd and Fin = 2 Fout - 1 there are Fout / 2 full row tiles and every edge tile (column pair e = jt / 2, ct) is hit
    exactly once, jt even;
  * every other row count yields no edge workgroup and exactly the former grid of (Fout + 1) / 2 row tiles -- an even Fout, and an
    odd Fout with an even Fin (Fin = 6, 10: the last row has four real taps and stays a half tile);
  * with xcd_split, co-tile group ct sits on the XCDs (block id mod 8) = ct (mod cgroups), edge and full alike;
  * edge blocks precede every full block (they last as long as full tiles and must not form the last round).
The workgroup counts of enc2 .. enc5 at B = 64 are compared with the counts the design states."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dccrn-vae_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FINS = (4, 5, 6, 7, 8, 9, 10, 11, 17, 33, 65)
JTILES = (1, 2, 3, 8, 9, 642)
CGROUPS = (1, 2, 3, 4, 5, 8)

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "cgemm_tw_map.hpp"

static int check(int Fin, int jtiles, int cgroups, int want_split) {
    const int Fout = (Fin - 1) / 2 + 1;
    const TwGrid g = tw2_grid(Fin, Fout, jtiles * 64 - 5, cgroups, want_split);
    int bad = 0;
    const bool has_edge = (Fout & 1) && Fin == 2 * Fout - 1;
    if (g.jtiles != jtiles || g.cgroups != cgroups) ++bad;
    if (g.ftiles != (has_edge ? Fout / 2 : (Fout + 1) / 2)) ++bad;
    if (g.etiles != (has_edge ? (jtiles + 1) / 2 : 0)) ++bad;
    if (g.xcd_split != ((want_split && (cgroups == 2 || cgroups == 4 || cgroups == 8)) ? 1 : 0)) ++bad;
    const long long nblk = tw_grid_blocks(g);
    std::vector<int> full((size_t)jtiles * g.ftiles * cgroups, 0), edge((size_t)(g.etiles ? g.etiles : 1) * cgroups, 0);
    long long nfull = 0, nedge = 0, none = 0, last_edge = -1, first_full = -1;
    for (long long bid = 0; bid < nblk; ++bid) {
        TwTile t;
        if (!tw_block_tile(g, (int)bid, t)) { ++none; continue; }
        if (t.ct < 0 || t.ct >= cgroups || t.jt < 0 || t.jt >= jtiles) { ++bad; continue; }
        if (g.xcd_split && (int)(bid & 7) % cgroups != t.ct) ++bad;
        if (t.edge) {
            if (!g.etiles || (t.jt & 1) || t.jt / 2 >= g.etiles) { ++bad; continue; }
            ++edge[(size_t)(t.jt / 2) * cgroups + t.ct];
            ++nedge;
            last_edge = bid;
        } else {
            if (t.ft < 0 || t.ft >= g.ftiles) { ++bad; continue; }
            ++full[((size_t)t.jt * g.ftiles + t.ft) * cgroups + t.ct];
            ++nfull;
            if (first_full < 0) first_full = bid;
        }
    }
    for (int v : full) if (v != 1) ++bad;
    if (g.etiles) { for (int v : edge) if (v != 1) ++bad; }
    if (!has_edge && nedge != 0) ++bad;
    if (nedge && nfull && last_edge > first_full) ++bad;
    printf("Fin %d Fout %d jtiles %d cgroups %d split %d : blocks %lld full %lld edge %lld empty %lld bad %d\n", Fin, Fout, jtiles, cgroups,
           g.xcd_split, nblk, nfull, nedge, none, bad);
    return bad;
}

int main() {
    const int J[] = {@JTILES@}, CG[] = {@CGROUPS@}, FIN[] = {@FINS@};
    int bad = 0;
    for (int fin : FIN)
        for (int j : J)
            for (int cg : CG)
                for (int split = 0; split < 2; ++split) bad += check(fin, j, cg, split);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail(f"{HIPCC} not found: the launch-geometry program cannot be built")
    d = tmp_path_factory.mktemp("tw2_edge")
    src, exe = d / "tw2_map_enum.hip", d / "tw2_map_enum"
    text = PROGRAM
    for name, values in (("@JTILES@", JTILES), ("@CGROUPS@", CGROUPS), ("@FINS@", FINS)):
        text = text.replace(name, ", ".join(map(str, values)))
    src.write_text(text)
    # host code only: no device pass, nothing of the GPU runtime is used
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-host-only", "-I", CSRC, str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    out = r.stdout.strip().splitlines()
    failed = [l for l in out if not l.endswith("bad 0")]
    assert r.returncode == 0 and not failed, "\n".join(failed[:20]) + r.stderr
    rows = {}
    for l in out:
        w = l.split()
        key = (int(w[1]), int(w[5]), int(w[7]), int(w[9]))          # Fin, jtiles, cgroups, split in effect
        rows[key] = dict(fout=int(w[3]), blocks=int(w[12]), full=int(w[14]), edge=int(w[16]), empty=int(w[18]))
    return rows


def _has_edge(fin):
    fout = (fin - 1) // 2 + 1
    return fout % 2 == 1 and fin == 2 * fout - 1


def test_every_tile_once_and_co_tile_groups_keep_their_xcds(lines):
    """(uniqueness, ranges, the XCD rule and edge-before-full are the program's `bad` count, asserted zero by the fixture)"""
    for fin in FINS:
        fout = (fin - 1) // 2 + 1
        for jt in JTILES:
            for cg in CGROUPS:
                for split in ((0, 1) if cg in (2, 4, 8) else (0,)):
                    r = lines[(fin, jt, cg, split)]
                    assert r["fout"] == fout
                    if _has_edge(fin):
                        assert r["full"] == jt * (fout // 2) * cg
                        assert r["edge"] == (jt + 1) // 2 * cg
                    else:
                        assert r["full"] == jt * ((fout + 1) // 2) * cg
                        assert r["edge"] == 0
                    assert r["blocks"] == r["full"] + r["edge"] + r["empty"]
    assert [f for f in FINS if _has_edge(f)] == [5, 9, 17, 33, 65]


def test_no_edge_row_counts_launch_the_former_grid(lines):
    """An even Fout (Fin = 4, 7, 8, 11) and an odd Fout with an even Fin (Fin = 6, 10) launch exactly the grid from before edge
    workgroups existed: whole rounds of eight blocks over (Fout + 1) / 2 row tiles, half tile included."""
    seen = set()
    for (fin, jt, cg, split), r in lines.items():
        if _has_edge(fin):
            continue
        seen.add(fin)
        ftiles = (r["fout"] + 1) // 2
        if split:
            G = 8 // cg
            want = (jt + G - 1) // G * ftiles * 8
        else:
            want = (jt + 7) // 8 * 8 * ftiles * cg
        assert r["edge"] == 0 and r["blocks"] == want, (fin, jt, cg, split)
    assert seen == {4, 6, 7, 8, 10, 11}


def test_encoder_workgroup_counts_at_batch_64(lines):
    """642 column blocks, paired co tiles: enc2 .. enc5 launch 21186, 10914, 11556 and 6420 workgroups (half tiles of their own made it
    21828, 11556, 12840 and 7704)."""
    for fin, cg, want, before in ((65, 2, 21186, 21828), (33, 2, 10914, 11556), (17, 4, 11556, 12840), (9, 4, 6420, 7704)):
        r = lines[(fin, 642, cg, 1)]
        assert r["full"] + r["edge"] == want, (fin, cg, r)
        assert 642 * ((r["fout"] + 1) // 2) * cg == before
