"""BSS-eval SDR / SIR / SAR with the noise as second source on the MI355X (csrc/bss.hip through inference.compute_bss / score_list)
against the float64 host reference tests/bss_ref.py.  The reference results are computed once per module and shared; every test is
a single pass over signals of at most 16385 samples."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# 4 x the worst deviation from the float64 definition (LU) measured over R.CASES on the MI355X (test_parity_with_the_float64_definition)
OUT_ULPS = 1.0                 # float32 ulps of a dB value.  Measured worst: 0 on all three (every case is the rounded float64 value): the floor, 1
ENERGY_REL = 1e-12             # measured worst: 1.76e-13 (sum (pall - p1)^2, L = 768, K = 512), 8.4e-14 (sum pall^2): 4 x lies under the floor, 1e-12
RESIDUAL = 1.36e-14            # max |G C - D| / x_ss[0].  Measured worst: 3.40e-15 (L = 1025, K = 512; the LU reference's own: 2.8e-15)
ENERGIES = ("target_energy", "error_energy", "interf_energy", "projection_energy", "artif_energy")


def _inf():
    return importlib.import_module("i-dccrn-vae_amd.inference")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _padded(rows, pitch, fill=float("nan")):
    """The rows in a [B, pitch] float32 device tensor with `fill` behind every row's end."""
    t = torch.full((len(rows), pitch), fill, dtype=torch.float32)
    for k, r in enumerate(rows):
        t[k, :len(r)] = torch.from_numpy(np.asarray(r, dtype=np.float32))
    return t.cuda()


@pytest.fixture(scope="module")
def ref():
    """Per case: the float32 signals (what the device sees) and the float64 definition's result.  Computed once, never changed."""
    table = []
    for index, (L, K, kind) in enumerate(R.CASES):
        s, v, y = R.case_signals(index)
        table.append(dict(L=L, K=K, s=s, v=v, y=y, want=R.bss(s, v, y, K)))
    return table


def _ulps(got, want):
    want32 = np.float32(want)
    if not np.isfinite(want32):
        return 0.0 if got == want32 else math.inf
    return abs(float(got) - float(want32)) / float(np.spacing(np.abs(want32)))


def _rel(got, want):
    if want == 0:
        return 0.0 if got == 0 else math.inf
    return abs(got - want) / want


def test_parity_with_the_float64_definition(ref):
    """All cases of one K in ONE padded batch with lengths=, rows at an odd pitch, NaN behind every row's end in all three inputs; the
    three dB values, the five sums and the joint residual max |G C - D| / x_ss[0] of the device's filters against tests/bss_ref.py
    (float64, LU).  The bounds are 4 x the worst deviation measured over R.CASES on the MI355X, with floors of one float32 ulp of the
    value for a dB value and 1e-12 relative for the sums.

    Measured on the MI355X, 17 cases, K = 16 / 64 / 512: SDR, SIR and SAR equal the rounded float64 value in every case
    (0 ulp, so the bound is the floor of 1 ulp); the five sums within 7.3e-14 (sum p1^2), 6.1e-16 (sum (y - p1)^2), 1.76e-13 (sum (pall -
    p1)^2), 8.4e-14 (sum pall^2) and 1.7e-15 (sum (y - pall)^2) relative (4 x the worst: 7.0e-13, under the floor of 1e-12, which is the
    bound); the joint residual at most 3.40e-15 (bound 1.36e-14) where the LU reference's own is at most 2.8e-15."""
    inf = _inf()
    worst = dict(sdr=0.0, sir=0.0, sar=0.0, residual=0.0, ref_residual=0.0, **{n: 0.0 for n in ENERGIES})
    for K in sorted({c["K"] for c in ref}):
        rows = [c for c in ref if c["K"] == K]
        lens = [c["L"] for c in rows]
        pitch = max(lens) + 3 + (max(lens) % 2)                              # odd, wider than the longest row
        assert pitch % 2 == 1
        est, cln, nse = (_padded([c[n] for c in rows], pitch) for n in "ysv")
        sdr, sir, sar, det = inf.compute_bss(est, cln, nse, filt_len=K, lengths=lens, details=True)
        for t in (sdr, sir, sar):
            assert t.dtype == torch.float32 and t.shape == (len(rows),)
        assert det["filters"].dtype == torch.float64 and det["filters"].shape == (len(rows), 2, K)
        for n in ENERGIES:
            assert det[n].dtype == torch.float64 and det[n].shape == (len(rows),)
        got = dict(sdr=sdr.cpu().numpy(), sir=sir.cpu().numpy(), sar=sar.cpu().numpy(), **{n: det[n].cpu().numpy() for n in ENERGIES})
        filt = det["filters"].cpu().numpy()
        for k, c in enumerate(rows):
            w = c["want"]
            fig = {n: _ulps(got[n][k], w[n]) for n in ("sdr", "sir", "sar")}
            fig.update({n: _rel(got[n][k], w[n]) for n in ENERGIES})
            fig.update(residual=R.residual(filt[k], w["lags"]), ref_residual=R.residual(w["filters"], w["lags"]))
            print(f"K {K:3d} L {c['L']:5d}  got {got['sdr'][k]!r} {got['sir'][k]!r} {got['sar'][k]!r}  want {w['sdr']!r} {w['sir']!r} "
                  f"{w['sar']!r}  " + "  ".join(f"{n} {v:.3g}" for n, v in fig.items()))
            for n, v in fig.items():
                worst[n] = max(worst[n], v)
    print("worst:", worst)
    assert max(worst["sdr"], worst["sir"], worst["sar"]) <= OUT_ULPS
    assert max(worst[n] for n in ENERGIES) <= ENERGY_REL
    assert worst["residual"] <= RESIDUAL


def test_sdr_column_is_compute_sdr(ref):
    """The SDR column and its two sums come from idv_sdr's own launches: the bits of compute_sdr, on every case."""
    inf = _inf()
    for K in sorted({c["K"] for c in ref}):
        rows = [c for c in ref if c["K"] == K]
        lens = [c["L"] for c in rows]
        est, cln, nse = (_padded([c[n] for c in rows], max(lens) + 1) for n in "ysv")
        sdr, _, _, det = inf.compute_bss(est, cln, nse, filt_len=K, lengths=lens, details=True)
        one, d1 = inf.compute_sdr(est, cln, filt_len=K, lengths=lens, details=True)
        assert torch.equal(sdr, one) and torch.isfinite(sdr).all()
        assert torch.equal(det["target_energy"], d1["target_energy"]) and torch.equal(det["error_energy"], d1["error_energy"])


def test_a_row_does_not_depend_on_its_batch(ref):
    """One row alone, in a batch of 3 and in a batch of 65 rows of mixed lengths, at other pitches and with other padding: the same bits
    in the three values, the filters and the five sums."""
    inf = _inf()
    c = next(c for c in ref if (c["L"], c["K"]) == (1025, 512))
    *alone, da = inf.compute_bss(_cuda(c["y"]), _cuda(c["s"]), _cuda(c["v"]), details=True)
    assert alone[1].shape == () and da["filters"].shape == (2, 512) and da["artif_energy"].shape == ()
    rng = np.random.default_rng(5)
    for B, at, pitch, fill in ((3, 1, 1100, 7.0), (65, 41, 4700, float("inf"))):
        lens = [int(v) for v in rng.integers(1, 4600 if B == 65 else 1000, B)]
        lens[at] = 1025
        sig = [[rng.standard_normal(n).astype(np.float32) for n in lens] for _ in range(3)]
        sig[0][at], sig[1][at], sig[2][at] = c["y"], c["s"], c["v"]
        *out, d = inf.compute_bss(_padded(sig[0], pitch, fill), _padded(sig[1], pitch + 2, -fill), _padded(sig[2], pitch + 5, fill),
                                  lengths=lens, details=True)
        for k in range(3):
            assert torch.equal(out[k][at], alone[k]), (B, k, out[k][at], alone[k])
        for name in ("filters",) + ENERGIES:
            assert torch.equal(d[name][at], da[name]), (B, name)
        assert not torch.isnan(out[0]).any()                                 # no neighbour's padding got in
        # rows of K samples or fewer are NaN by the definition; from 2 K on nothing is (between the two G is near singular)
        for lo, hi, nan in ((1, 512, True), (1024, 1 << 30, False)):
            pick = torch.tensor([lo <= n <= hi for n in lens])
            assert (torch.isnan(out[1]).cpu()[pick] == nan).all() and (torch.isnan(out[2]).cpu()[pick] == nan).all()


def test_special_rows(ref):
    """In one batch at filt_len = 64: a normal row, a silent reference, a silent interferer, a silent estimate, L = K, L = 1, v = 2 s and
    y = 0.5 s delayed by three samples with nothing of the interferer in it (the reference ends in silence, so the cut at the row's
    length takes nothing away)."""
    inf = _inf()
    K = 64
    c = next(c for c in ref if (c["L"], c["K"]) == (257, K))
    L = 1500
    s = R.reference(L, "lowpass", seed=77)
    s[-16:] = 0
    v = R.reference(L, "white", seed=78)
    y = R.mixture(s, v, 20, 1.0, seed=79)
    delayed = np.zeros(L, dtype=np.float32)
    delayed[3:] = 0.5 * s[:-3]
    zero = np.zeros(L, dtype=np.float32)
    two = (2 * s).astype(np.float32)
    rows = [(c["y"], c["s"], c["v"]), (y, zero, v), (y, s, zero), (zero, s, v), (y[:K], s[:K], v[:K]), (y[:1], s[:1], v[:1]),
            (y, s, two), (delayed, s, v)]
    lens = [len(r[0]) for r in rows]
    est, cln, nse = (_padded([r[k] for r in rows], L + 1) for k in range(3))
    sdr, sir, sar, d = inf.compute_bss(est, cln, nse, filt_len=K, lengths=lens, details=True)
    one = inf.compute_sdr(est, cln, filt_len=K, lengths=lens)
    *alone, da = inf.compute_bss(_cuda(c["y"]), _cuda(c["s"]), _cuda(c["v"]), filt_len=K, details=True)
    assert torch.equal(sdr[0], alone[0]) and torch.equal(sir[0], alone[1]) and torch.equal(sar[0], alone[2])
    for name in ("filters",) + ENERGIES:
        assert torch.equal(d[name][0], da[name]), name
    o = [t.cpu().tolist() for t in (sdr, sir, sar)]
    e = {n: d[n].cpu().tolist() for n in ENERGIES}
    print("special rows:", o, e)
    same = (one == sdr) | (torch.isnan(one) & torch.isnan(sdr))
    assert same.all()
    # a silent reference: three NaN, every sum NaN
    assert all(math.isnan(o[k][1]) for k in range(3)) and all(math.isnan(e[n][1]) for n in ENERGIES) and torch.isnan(d["filters"][1]).all()
    # a silent interferer, L = K, L = 1, v = 2 s: the SDR intact, SIR and SAR NaN, their three sums and the filters NaN
    for row in (2, 4, 5, 6):
        assert not math.isnan(o[0][row]) and math.isnan(o[1][row]) and math.isnan(o[2][row]), row
        assert not math.isnan(e["target_energy"][row]) and not math.isnan(e["error_energy"][row]), row
        assert all(math.isnan(e[n][row]) for n in ENERGIES[2:]) and torch.isnan(d["filters"][row]).all(), row
    assert math.isfinite(o[0][2]) and math.isfinite(o[0][6])
    # a silent estimate: every numerator is zero
    assert o[0][3] == o[1][3] == o[2][3] == -math.inf and e["target_energy"][3] == 0.0 and e["projection_energy"][3] == 0.0
    # an exactly filtered copy of the target alone: nothing leaks, nothing is left
    for k in range(3):
        assert o[k][7] == math.inf or o[k][7] > 120.0, (k, o[k][7])
    f = d["filters"][7].cpu().numpy()
    assert abs(f[0, 3] - 0.5) < 1e-9 and np.abs(np.delete(f[0], 3)).max() < 1e-9 and np.abs(f[1]).max() < 1e-9


def test_rationale_leakage_against_artifacts():
    """One mixture s + v and two estimates of s with the same SDR by construction: s plus 10 % of v (leakage) and s plus white noise of
    that energy (artifacts).  The SDR cannot tell them apart; SIR is more than 10 dB lower for the first, SAR for the second.  The
    signals are checked against the float64 definition on the host first."""
    inf = _inf()
    L, K = 8000, 64
    s = R.reference(L, "lowpass", seed=21)
    v = R.reference(L, "white", seed=22)
    leak = 0.1 * v.astype(np.float64)
    nz = np.random.default_rng(23).standard_normal(L)
    nz *= np.sqrt(np.sum(leak * leak) / np.sum(nz * nz))
    est = [(s + leak).astype(np.float32), (s + nz).astype(np.float32)]
    want = [R.bss(s, v, y, K) for y in est]
    assert abs(want[0]["sdr"] - want[1]["sdr"]) < 0.5
    assert want[1]["sir"] - want[0]["sir"] > 10 and want[0]["sar"] - want[1]["sar"] > 10
    sdr, sir, sar = inf.compute_bss(_cuda(np.stack(est)), _cuda(np.stack([s, s])), _cuda(np.stack([v, v])), filt_len=K)
    print("rationale: sdr", sdr.tolist(), "sir", sir.tolist(), "sar", sar.tolist(), "want", [(w["sdr"], w["sir"], w["sar"]) for w in want])
    assert abs(sdr[0].item() - sdr[1].item()) < 0.5
    assert sir[1].item() - sir[0].item() > 10 and sar[0].item() - sar[1].item() > 10
    for k in range(2):
        assert _ulps(sir[k].item(), want[k]["sir"]) <= OUT_ULPS and _ulps(sar[k].item(), want[k]["sar"]) <= OUT_ULPS


def test_score_list_with_interferers():
    """The caller's order with interferers=, triples of three different lengths (aligned to the shortest of the three), "sir" without
    interferers, and a call that was valid before."""
    inf = _inf()
    lens = ((1300, 1250, 1400), (4001, 4100, 4050), (2025, 2000, 2010), (1513, 1513, 1500), (2500, 2600, 2450))
    refs, nses, ests = [], [], []
    for k, (ne, nr, nv) in enumerate(lens):
        n = max(ne, nr, nv)
        s, v = R.reference(n, ("white", "lowpass")[k % 2], seed=50 + k), R.reference(n, ("lowpass", "white")[k % 2], seed=60 + k)
        y = R.mixture(s, v, (20, 0, 60)[k % 3], (1.0, 0.0, 0.1)[k % 3], seed=50 + k)
        ests.append(_cuda(y[:ne]))
        refs.append(_cuda(s[:nr]))
        nses.append(_cuda(v[:nv]))
    res = inf.score_list(ests, refs, metrics=("sisdr", "sdr", "sir", "sar"), max_batch=2, interferers=nses)
    assert set(res) == {"sisdr", "sdr", "sir", "sar"}
    for k, ns in enumerate(lens):
        n = min(ns)
        want = inf.compute_bss(ests[k][:n], refs[k][:n], nses[k][:n])
        for name, w in zip(("sdr", "sir", "sar"), want):
            assert res[name].dtype == torch.float32 and torch.equal(res[name][k], w.cpu()), (k, name)
        assert torch.equal(res["sisdr"][k], inf.compute_sisdr(ests[k][:n], refs[k][:n]).cpu()), k
    assert torch.isfinite(res["sir"]).all() and len(set(res["sir"].tolist())) == 5
    for name in ("sir", "sar"):
        with pytest.raises(ValueError, match="interferers"):
            inf.score_list(ests, refs, metrics=("sdr", name))
    with pytest.raises(ValueError, match="4 interferers"):
        inf.score_list(ests, refs, metrics=("sir",), interferers=nses[:4])
    old = inf.score_list(ests, refs, metrics=("sisdr", "sdr"), max_batch=2)
    for k, (ne, nr, _) in enumerate(lens):
        n = min(ne, nr)
        assert torch.equal(old["sdr"][k], inf.compute_sdr(ests[k][:n], refs[k][:n]).cpu()), k
        assert torch.equal(old["sisdr"][k], inf.compute_sisdr(ests[k][:n], refs[k][:n]).cpu()), k


@pytest.mark.parametrize("K", [16, 64])
def test_shorter_filters_and_scalar_results(ref, K):
    inf = _inf()
    c = max((c for c in ref if c["K"] == K), key=lambda c: c["L"])
    out = inf.compute_bss(_cuda(c["y"]), _cuda(c["s"]), _cuda(c["v"]), filt_len=K)
    assert len(out) == 3
    for t, name in zip(out, ("sdr", "sir", "sar")):
        assert t.shape == () and t.dtype == torch.float32
        assert _ulps(t.item(), c["want"][name]) <= OUT_ULPS, name
    both = inf.compute_bss(_cuda(c["y"])[None], _cuda(c["s"])[None], _cuda(c["v"])[None], filt_len=K)
    for k in range(3):
        assert both[k].shape == (1,) and torch.equal(both[k][0], out[k])
