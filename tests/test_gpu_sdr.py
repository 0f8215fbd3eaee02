"""BSS-eval SDR on the MI355X (csrc/sdr.hip through inference.compute_sdr / score_list) against the float64 host reference
tests/sdr_ref.py.  The reference results are computed once per module and shared; every test is a single pass over signals of at
most 16385 samples."""
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

import sdr_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# 4 x the worst deviation from the float64 definition measured over R.CASES on the MI355X (test_parity_with_the_float64_definition)
OUT_ULPS = 1.0                 # float32 ulps of the dB value.  Measured worst: 0 (every case is the rounded float64 value): the floor, 1
ENERGY_REL = 1e-12             # measured worst: 3.8e-14 (sum p^2, L = 511, K = 512), 4.6e-15 (sum e^2): 4 x lies under the floor, 1e-12
RESIDUAL = 9.7e-15             # max |G c - d| / r[0].  Measured worst: 2.42e-15 (L = 511, K = 512; the LU reference's own: 1.3e-15)


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
        s, y = R.case_signals(index)
        table.append(dict(L=L, K=K, s=s, y=y, want=R.sdr(s, y, K)))
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
    """All cases of one K in ONE padded batch with lengths=, rows at an odd pitch, NaN behind every row's end; out, the two energies and
    the normal-equation residual max |G c - d| / r[0] of the device's filter against tests/sdr_ref.py (float64, LU).  The bounds are
    4 x the worst deviation measured over R.CASES on the MI355X (the margin covers a reordered double sum on another input), with
    floors of one float32 ulp of the value for out and 1e-12 relative for the energies.

    Measured on the MI355X, 20 cases, K = 16 / 64 / 512: out equals the rounded float64 value in every case (0 ulp, so
    the bound is the floor of 1 ulp); sum p^2 within 3.8e-14 and sum e^2 within 4.6e-15 relative (4 x: 1.5e-13 and 1.9e-14, under the
    floor of 1e-12, which is the bound); the residual at most 2.42e-15 (bound 9.7e-15) where the LU reference's own is 1.3e-15.  The
    one-sample row is explained exactly on both sides: sum e^2 == 0 and +inf."""
    inf = _inf()
    worst = dict(out=0.0, target=0.0, error=0.0, residual=0.0, ref_residual=0.0)
    for K in sorted({c["K"] for c in ref}):
        rows = [c for c in ref if c["K"] == K]
        lens = [c["L"] for c in rows]
        pitch = max(lens) + 3 + (max(lens) % 2)                              # odd, wider than the longest row
        assert pitch % 2 == 1
        est, cln = _padded([c["y"] for c in rows], pitch), _padded([c["s"] for c in rows], pitch)
        out, det = inf.compute_sdr(est, cln, filt_len=K, lengths=lens, details=True)
        assert out.dtype == torch.float32 and out.shape == (len(rows),)
        assert det["filter"].dtype == torch.float64 and det["filter"].shape == (len(rows), K)
        assert det["target_energy"].dtype == torch.float64 and det["target_energy"].shape == det["error_energy"].shape == (len(rows),)
        out, filt = out.cpu().numpy(), det["filter"].cpu().numpy()
        tp, te = det["target_energy"].cpu().numpy(), det["error_energy"].cpu().numpy()
        for k, c in enumerate(rows):
            w = c["want"]
            fig = dict(out=_ulps(out[k], w["sdr"]), target=_rel(tp[k], w["target_energy"]), error=_rel(te[k], w["error_energy"]),
                       residual=R.residual(filt[k], w["r"], w["d"]), ref_residual=R.residual(w["filter"], w["r"], w["d"]))
            print(f"K {K:3d} L {c['L']:5d}  out {out[k]!r} want {w['sdr']!r}  " + "  ".join(f"{n} {v:.3g}" for n, v in fig.items()))
            for n, v in fig.items():
                worst[n] = max(worst[n], v)
    print("worst:", worst)
    assert worst["out"] <= OUT_ULPS
    assert worst["target"] <= ENERGY_REL and worst["error"] <= ENERGY_REL
    assert worst["residual"] <= RESIDUAL


def test_a_row_does_not_depend_on_its_batch(ref):
    """One row alone, in a batch of 3 and in a batch of 65 rows of mixed lengths, at other pitches and with other padding: the same bits
    in out and in all three detail tensors."""
    inf = _inf()
    c = next(c for c in ref if (c["L"], c["K"]) == (1025, 512))
    alone, da = inf.compute_sdr(_cuda(c["y"]), _cuda(c["s"]), details=True)
    assert alone.shape == () and da["filter"].shape == (512,) and da["target_energy"].shape == ()
    rng = np.random.default_rng(5)
    for B, at, pitch, fill in ((3, 1, 1100, 7.0), (65, 41, 4700, float("inf"))):
        lens = [int(v) for v in rng.integers(1, 4600 if B == 65 else 1000, B)]
        lens[at] = 1025
        est = [rng.standard_normal(n).astype(np.float32) for n in lens]
        cln = [rng.standard_normal(n).astype(np.float32) for n in lens]
        est[at], cln[at] = c["y"], c["s"]
        out, d = inf.compute_sdr(_padded(est, pitch, fill), _padded(cln, pitch + 2, -fill), lengths=lens, details=True)
        assert torch.equal(out[at], alone), (B, out[at], alone)
        for name in ("filter", "target_energy", "error_energy"):
            assert torch.equal(d[name][at], da[name]), (B, name)
        assert not torch.isnan(out).any()                                    # no neighbour's NaN padding got in


def test_special_rows(ref):
    """A normal row, a silent estimate (-inf), a silent reference (NaN) and est = 0.5 ref delayed by 7 samples in one batch.  The delayed
    row's reference ends in silence, so the cut at the row's length takes nothing away: it is explained exactly, +inf or beyond 120 dB,
    which the quadratic forms c'd and sum est^2 - c'd would not reach.  The normal row's bits are those it has alone."""
    inf = _inf()
    c = next(c for c in ref if (c["L"], c["K"]) == (1023, 512))
    L = 3000
    s = R.reference(L, "lowpass", seed=77)
    s[-16:] = 0
    delayed = np.zeros(L, dtype=np.float32)
    delayed[7:] = 0.5 * s[:-7]
    zero = np.zeros(L, dtype=np.float32)
    est = _padded([c["y"], zero, s, delayed], L + 1)
    cln = _padded([c["s"], s, zero, s], L + 1)
    out, d = inf.compute_sdr(est, cln, lengths=[1023, L, L, L], details=True)
    alone, da = inf.compute_sdr(_cuda(c["y"]), _cuda(c["s"]), details=True)
    assert torch.equal(out[0], alone) and torch.equal(d["filter"][0], da["filter"])
    assert torch.equal(d["target_energy"][0], da["target_energy"]) and torch.equal(d["error_energy"][0], da["error_energy"])
    o = out.cpu().tolist()
    print("special rows:", o, d["target_energy"].cpu().tolist(), d["error_energy"].cpu().tolist())
    assert o[1] == -math.inf and d["target_energy"][1].item() == 0.0
    assert math.isnan(o[2]) and torch.isnan(d["filter"][2]).all() and math.isnan(d["error_energy"][2].item())
    assert o[3] == math.inf or o[3] > 120.0
    f = d["filter"][3].cpu().numpy()
    assert abs(f[7] - 0.5) < 1e-9 and np.abs(np.delete(f, 7)).max() < 1e-9


def test_rationale_reverberant_estimate_against_the_dry_reference(ref):
    """The estimate is dataset.reverb.reverb of the reference under a 200-tap response whose first tap is at 37: an exactly filtered
    copy up to one float32 rounding per sample (the reference ends in silence longer than the response, so the cut at its length
    takes nothing away).  compute_sdr is above 100 dB where compute_sisdr is below 0 dB."""
    inf = _inf()
    reverb = importlib.import_module("i-dccrn-vae_amd.dataset.reverb")
    c = next(c for c in ref if c["L"] == 4001)
    s = c["s"].copy()
    s[-256:] = 0
    rng = np.random.default_rng(9)
    h = np.zeros(200, dtype=np.float32)
    h[37:] = (rng.standard_normal(163) * np.exp(-np.arange(163) / 40.0)).astype(np.float32)
    h[37] = 1.0
    x = _cuda(s)
    y = reverb.reverb(x[None], _cuda(h)[None])[0]
    sdr, sisdr = inf.compute_sdr(y, x).item(), inf.compute_sisdr(y, x).item()
    print("rationale: sdr", sdr, "sisdr", sisdr)
    assert sdr > 100.0 and sisdr < 0.0


def test_score_list_in_the_callers_order(ref):
    inf = _inf()
    lens = (300, 4001, 1025, 513, 2500)
    refs = [_cuda(R.reference(n, ("white", "lowpass")[k % 2], seed=50 + k)) for k, n in enumerate(lens)]
    ests = [_cuda(R.estimate(r.cpu().numpy(), (20, 0, 60)[k % 3], seed=50 + k)) for k, r in enumerate(refs)]
    res = inf.score_list(ests, refs, metrics=("sisdr", "sdr"), max_batch=2)
    assert set(res) == {"sisdr", "sdr"} and res["sdr"].shape == (5,) and res["sdr"].dtype == torch.float32
    for k in range(5):
        assert torch.equal(res["sdr"][k], inf.compute_sdr(ests[k], refs[k]).cpu()), k
        assert torch.equal(res["sisdr"][k], inf.compute_sisdr(ests[k], refs[k]).cpu()), k
    assert torch.isfinite(res["sdr"]).all() and len(set(res["sdr"].tolist())) == 5


@pytest.mark.parametrize("K", [16, 64])
def test_shorter_filters_and_scalar_result(ref, K):
    inf = _inf()
    c = max((c for c in ref if c["K"] == K), key=lambda c: c["L"])
    out = inf.compute_sdr(_cuda(c["y"]), _cuda(c["s"]), filt_len=K)
    assert out.shape == () and out.dtype == torch.float32
    assert _ulps(out.item(), c["want"]["sdr"]) <= OUT_ULPS
    both = inf.compute_sdr(_cuda(c["y"])[None], _cuda(c["s"])[None], filt_len=K)
    assert both.shape == (1,) and torch.equal(both[0], out)
