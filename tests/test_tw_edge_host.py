"""CPU test of the launch geometry of the time-Winograd transposed conv (csrc/cgemm_tw_map.hpp): the block -> (column block, row tile
or edge, co-tile group) mapping that kernel and launch share, compiled into a small stand-alone host program and enumerated.

For every (phase, Fin, jtiles, cgroups, block order) the program walks all blocks of the grid and checks that
  * every full tile (jt, ft, ct) is hit exactly once, and no tile outside the ranges is produced;
  * for an odd Fin in the even-row phase every edge tile (column pair e = jt / 2, ct) is hit exactly once, jt even;
  * an even Fin, and the odd-row phase, yield no edge workgroup at all and exactly the grid of full tiles;
  * with xcd_split, co-tile group ct sits on the XCDs (block id mod 8) = ct (mod cgroups), edge and full alike;
  * edge blocks precede every full block (they last as long as full tiles and must not form the last round).
It prints one line per configuration; the workgroup counts of the five decoder layers at B = 64 are compared with the counts the
design states."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dccrn-vae_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "cgemm_tw_map.hpp"

static int check(int ph, int Fin, int jtiles, int cgroups, int want_split) {
    const TwGrid g = tw_grid(ph, Fin, jtiles * 64 - 5, cgroups, want_split);
    int bad = 0;
    if (g.jtiles != jtiles || g.ftiles != Fin / 2 || g.cgroups != cgroups) ++bad;
    const bool odd_even_phase = ph == 0 && (Fin & 1);
    if (g.etiles != (odd_even_phase ? (jtiles + 1) / 2 : 0)) ++bad;
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
    if (!odd_even_phase && nedge != 0) ++bad;
    if (nedge && nfull && last_edge > first_full) ++bad;
    printf("ph %d Fin %d jtiles %d cgroups %d split %d : blocks %lld full %lld edge %lld empty %lld bad %d\n", ph, Fin, jtiles, cgroups,
           g.xcd_split, nblk, nfull, nedge, none, bad);
    return bad;
}

int main() {
    const int J[] = {1, 2, 3, 642}, CG[] = {1, 2, 4, 8, 3}, FIN[] = {2, 3, 5, 65, 4, 9, 17, 33};
    int bad = 0;
    for (int ph = 0; ph < 2; ++ph)
        for (int fin : FIN)
            for (int j : J)
                for (int cg : CG)
                    for (int split = 0; split < 2; ++split) bad += check(ph, fin, j, cg, split);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail(f"{HIPCC} not found: the launch-geometry program cannot be built")
    d = tmp_path_factory.mktemp("tw_edge")
    src, exe = d / "tw_map_enum.hip", d / "tw_map_enum"
    src.write_text(PROGRAM)
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
        key = (int(w[1]), int(w[3]), int(w[5]), int(w[7]), int(w[9]))
        rows[key] = dict(blocks=int(w[12]), full=int(w[14]), edge=int(w[16]), empty=int(w[18]))
    return rows


def test_every_tile_once_and_co_tile_groups_keep_their_xcds(lines):
    # the issue's cases are all there (the program adds cgroups 8 and 3 and the model's row counts)
    for ph in (0, 1):
        for fin in (2, 3, 5, 65):
            for jt in (1, 2, 3, 642):
                for cg in (1, 2, 4):
                    for split in ((0,) if cg == 1 else (0, 1)):
                        r = lines[(ph, fin, jt, cg, split)]
                        assert r["full"] == jt * (fin // 2) * cg
                        assert r["edge"] == ((jt + 1) // 2 * cg if ph == 0 and fin % 2 else 0)
                        assert r["blocks"] == r["full"] + r["edge"] + r["empty"]


def test_even_row_count_launches_no_edge_workgroup_and_the_former_grid(lines):
    for (ph, fin, jt, cg, split), r in lines.items():
        if fin % 2 == 0 or ph == 1:
            assert r["edge"] == 0
            # the grid before edge workgroups existed: whole rounds of eight blocks over the full tiles
            if split:
                G = 8 // cg
                want = (jt + G - 1) // G * (fin // 2) * 8
            else:
                want = (jt + 7) // 8 * 8 * (fin // 2) * cg
            assert r["blocks"] == want, (ph, fin, jt, cg, split)


def test_decoder_workgroup_counts_at_batch_64(lines):
    """Even-row phase, 642 column blocks: dec0 .. dec4 launch 6420, 5778, 10914, 10593 and 20865 workgroups (half tiles of their own
    would make it 7704, 6420, 11556, 10914 and 21186)."""
    for fin, cg, want in ((5, 4, 6420), (9, 2, 5778), (17, 2, 10914), (33, 1, 10593), (65, 1, 20865)):
        r = lines[(0, fin, 642, cg, 1 if cg > 1 else 0)]
        assert r["full"] + r["edge"] == want, (fin, cg, r)
