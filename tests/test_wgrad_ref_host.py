"""CPU tests behind the weight-gradient suite (tests/test_gpu_wgrad.py).

1. The float64 reference of the contraction (tests/wgrad_ref.py) against float64 autograd through the oracle's complex conv /
   transposed conv, on integer-valued inputs in [-3, 3]: both sides are exact, so the assertion is torch.equal.  That pins the tap
   order, the conjugation signs and the tshift convention before any kernel is involved.
2. The balanced split-K plan (make_plan_rounds, csrc/wgrad_common.hpp) compiled into a small stand-alone host program: 1 <= nsplit
   <= jtiles, the step ranges tile [0, steps_total) without gap, overlap or empty split, and no row count asks for more splits
   than Fs = 0, the bound the workspace is sized with.  The Python mirror of the plan (wgrad_ref.plan_rounds) must reproduce the
   program's output over a sweep and over every GPU case; at 256 compute units the cases named mid-tile must have split
   boundaries inside a column tile."""
import os
import subprocess

import pytest
import torch

import wgrad_ref as R
from oracle import idccrn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dccrn-vae_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).double()


# ----------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("transposed,cx,cout,cin_total,ci_off,fin,T,B", [
    (False, 3, 5, 3, 0, 9, 7, 2), (False, 2, 3, 6, 3, 5, 4, 3), (False, 4, 2, 4, 0, 1, 5, 2), (False, 1, 4, 1, 0, 17, 3, 1),
    (True, 3, 5, 3, 0, 5, 7, 2), (True, 2, 3, 6, 3, 4, 6, 3), (True, 4, 2, 4, 0, 1, 5, 2), (True, 5, 1, 7, 2, 2, 3, 1),
])
def test_reference_equals_oracle_autograd(transposed, cx, cout, cin_total, ci_off, fin, T, B, causal):
    g = torch.Generator().manual_seed(fin * 100 + T * 10 + ci_off + int(causal))
    x = ints(g, B, cin_total, fin, T, 2)
    wshape = (cin_total, cout, 5, 2) if transposed else (cout, cin_total, 5, 2)
    w_re, w_im = ints(g, *wshape).requires_grad_(True), ints(g, *wshape).requires_grad_(True)
    bias = torch.zeros(cout, dtype=torch.float64)
    if transposed:
        y = O.complex_conv_transpose2d(x, w_re, bias, w_im, bias, (2, 1), (2, 0), causal)
    else:
        y = O.complex_conv2d(x, w_re, bias, w_im, bias, (2, 1), (2, 1) if causal else (2, 0), causal)
    fout = 2 * fin - 1 if transposed else (fin - 1) // 2 + 1
    tout = T if causal else (T + 1 if transposed else T - 1)
    assert tuple(y.shape) == (B, cout, fout, tout, 2)
    dy = ints(g, *y.shape)
    (y * dy).sum().backward()
    got_re, got_im = R.conv_wgrad_ref(x[:, ci_off:ci_off + cx], dy, transposed, causal)
    sl = (slice(ci_off, ci_off + cx),) if transposed else (slice(None), slice(ci_off, ci_off + cx))
    assert got_re.dtype == torch.float64 and float(got_re.abs().max()) > 0
    assert torch.equal(got_re, w_re.grad[sl]) and torch.equal(got_im, w_im.grad[sl])


def test_pointwise_reference_and_gate_order():
    g = torch.Generator().manual_seed(5)
    H, M, K, J = 32, 256, 5, 9
    dout, x = ints(g, M, J), ints(g, K, J)
    plain = R.pw_wgrad_ref(dout, x, -1, 0, 0)
    want = torch.zeros(M, K, dtype=torch.float64)
    for j in range(1, J):
        want += dout[:, j:j + 1] * x[:, j - 1][None, :]
    assert torch.equal(plain, want)
    # gate order: colp = ((u / 16) * 4 + gate) * 16 + u % 16 -> gate * H + u, per set of 4 H rows; a permutation of the rows
    rows = [R.lstm_gate_row(m, H) for m in range(M)]
    assert sorted(rows) == list(range(M))
    for s in range(M // (4 * H)):
        for gate in range(4):
            for u in range(H):
                assert rows[s * 4 * H + ((u // 16) * 4 + gate) * 16 + u % 16] == s * 4 * H + gate * H + u
    mapped = R.pw_wgrad_ref(dout, x, -1, 1, H)
    assert torch.equal(mapped[rows], plain)


# ----------------------------------------------------------------------------- the split plan
PROGRAM = r"""
#include <cstdio>
#include "wgrad_common.hpp"

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    printf("cus %d\n", device_cus());
    int Sp, Lp, J, MS, ML, JT, np, occ, spt, allbad = 0;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d", &Sp, &Lp, &J, &MS, &ML, &JT, &np, &occ, &spt) == 9) {
        const Plan p = make_plan_rounds(Sp, Lp, J, MS, ML, JT, np, occ, spt), p0 = make_plan_rounds(Sp, Lp, J, MS, ML, JT, np, occ, 0);
        int bad = 0;
        if (p.nsplit < 1 || p.nsplit > p.jtiles || p.jtiles != (J + JT - 1) / JT) ++bad;
        if (p0.nsplit < 1 || p0.nsplit > p0.jtiles) ++bad;
        for (int fs = 1; fs <= 80; ++fs)
            if (make_plan_rounds(Sp, Lp, J, MS, ML, JT, np, occ, fs).nsplit > p0.nsplit) ++bad;      // Fs = 0 bounds the workspace
        printf("plan %d %d %d %d %d %d %d %d %d : nsplit %d jtiles %d nsplit0 %d bounds 0", Sp, Lp, J, MS, ML, JT, np, occ, spt, p.nsplit,
               p.jtiles, p0.nsplit);
        // the ranges as the kernels compute them
        const long long total = (long long)p.jtiles * spt;
        long long end = 0;
        for (int split = 0; split < p.nsplit; ++split) {
            const long long s0 = (long long)split * total / p.nsplit, s1 = (long long)(split + 1) * total / p.nsplit;
            if (s0 != end || s1 <= s0) ++bad;
            end = s1;
            printf(" %lld", s1);
        }
        if (end != total) ++bad;
        printf(" bad %d\n", bad);
        allbad += bad;
    }
    return allbad ? 1 : 0;
}
"""


def sweep():
    cases = []
    for MS, ML, JT, np_, occ in ((128, 32, 16, 1, 2), (128, 32, 16, 3, 2), (128, 32, 32, 3, 2), (128, 128, 32, 1, 1)):
        for Sp in (2, 80, 320, 1024):
            for Lp in (4, 48, 512):
                for J in (1, 93, 1284, 20544):
                    for spt in (1, 3, 5, 33):
                        cases.append((Sp, Lp, J, MS, ML, JT, np_, occ, spt))
    return cases + R.all_plan_args()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail(f"{HIPCC} not found: the split-plan program cannot be built")
    d = tmp_path_factory.mktemp("wgrad_plan")
    src, exe, inp = d / "wgrad_plan.hip", d / "wgrad_plan", d / "cases.txt"
    src.write_text(PROGRAM)
    inp.write_text("".join(" ".join(str(v) for v in c) + "\n" for c in sweep()))
    # host code only: the one runtime call is device_cus()'s query, which answers 256 where no device is visible
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-host-only", "-I", CSRC, str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if k not in ("IDV_WGRAD_ROUNDS", "IDV_WGRAD_WGS")}
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, env=env)
    out = r.stdout.strip().splitlines()
    failed = [l[:200] for l in out[1:] if not l.endswith("bad 0")]
    assert r.returncode == 0 and not failed, "\n".join(failed[:20]) + r.stderr
    cus = int(out[0].split()[1])
    rows = {}
    for l in out[1:]:
        w = l.split()
        assert w[0] == "plan" and w[10] == ":" and w[17] == "bounds" and w[-2] == "bad"
        rows[tuple(int(v) for v in w[1:10])] = dict(nsplit=int(w[12]), jtiles=int(w[14]), nsplit0=int(w[16]),
                                                    bounds=[int(v) for v in w[18:-2]])
    assert len(rows) == len(set(sweep()))
    return cus, rows


def test_plan_program_reports_the_compute_units(plans):
    cus, _ = plans
    if not torch.cuda.is_available():
        assert cus == 256                               # no device visible: the MI355X figure
    assert cus > 0


def test_plan_properties(plans):
    """Checked inside the program (its exit status); here once more on what it printed."""
    _, rows = plans
    for key, r in rows.items():
        spt = key[8]
        assert 1 <= r["nsplit"] <= r["jtiles"] and r["nsplit"] <= r["nsplit0"] <= r["jtiles"], key
        b = r["bounds"]
        assert len(b) == r["nsplit"] + 1 and b[0] == 0 and b[-1] == r["jtiles"] * spt, key
        assert all(b[i] < b[i + 1] for i in range(r["nsplit"])), key


def test_python_mirror_equals_the_program(plans):
    cus, rows = plans
    for key, r in rows.items():
        assert R.plan_rounds(*key, cus) == (r["nsplit"], r["jtiles"]), key
        assert R.plan_rounds(*key[:8], 0, cus) == (r["nsplit0"], r["jtiles"]), key
        assert R.split_bounds(r["nsplit"], r["jtiles"], key[8]) == r["bounds"], key


def test_mid_tile_cases_split_inside_a_column_tile_at_256_cus():
    for name, (entry, want) in R.MID_TILE.items():
        case = (R.FOUR_CASES if entry == "four" else R.GAUSS_CASES)[name]
        args = R.conv_plan_args(entry, case)
        ns, jt = R.plan_rounds(*args, 256)
        n = R.mid_tile_boundaries(R.split_bounds(ns, jt, args[8]), args[8])
        assert n >= 1 and n == want, (name, ns, jt, n)
    assert R.plan_rounds(*R.conv_plan_args("four", R.FOUR_CASES["A6"]), 256) == (28, 81)
    assert R.plan_rounds(*R.conv_plan_args("gauss", R.GAUSS_CASES["G4"]), 256) == (17, 19)
    assert R.plan_rounds(*R.conv_plan_args("gauss", R.GAUSS_CASES["G5"]), 256) == (17, 38)


def test_case_geometry_is_what_the_cases_are_for():
    """J, plane counts and kernel choice the case comments promise."""
    J = {k: R.conv_geometry(c)[6] for k, c in {**R.FOUR_CASES, **R.GAUSS_CASES, **R.BF16_CASES}.items()}
    assert (J["A1"], J["A2"], J["A3"], J["A6"], J["G1"], J["G4"]) == (66, 301, 93, 1284, 93, 600)
    assert J["B5"] % 4 == 0 and J["A3"] % 4 == 1
    for k in ("A1", "A2"):
        assert R.conv_plan_args("four", R.FOUR_CASES[k]) is None          # skinny kernel: two L planes
    for k, c in R.GAUSS_CASES.items():
        cs, cl, fs = R.conv_geometry(c)[:3]
        assert cs >= 128 and cl >= 32
        assert (fs >= R.WINO_MIN_ROWS) == (k in ("G1", "G3", "G3n", "G4", "G6")), k
