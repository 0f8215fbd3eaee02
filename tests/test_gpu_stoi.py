"""STOI / ESTOI / RMSE scoring on the MI355X (csrc/stoi.hip through inference.compute_stoi / compute_estoi / compute_rmse /
score_list) against the float64 host reference tests/stoi_ref.py.  The reference scores are computed once per session and shared;
every test is a single pass over signals of at most 1.5 s."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stoi_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ONE_E5 = float(np.float32(1e-5))


def _inf():
    return importlib.import_module("i-dccrn-vae_amd.inference")


def _cuda(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda()


@pytest.fixture(scope="module")
def ref():
    """Per (case, snr): the float32 signals (what the device sees; both references score exactly these), and per metric the
    float64 and float32 reference results.  Computed once, never changed."""
    table = {}
    for name, gen, n in R.CASES:
        x = gen(n).astype(np.float32)
        for snr in R.SNRS:
            y = R.noisy(gen(n), snr).astype(np.float32)
            rec = {"x": x, "y": y}
            for ext in (False, True):
                rec[ext] = (R.stoi(x, y, 16000, ext), R.stoi(x, y, 16000, ext, dtype=np.float32))
            table[(name, snr)] = rec
    return table


@pytest.fixture(scope="module")
def dev(ref):
    """The device's score and counts of every (case, snr, metric), each utterance alone at B = 1."""
    inf = _inf()
    out = {}
    for key, rec in ref.items():
        for ext in (False, True):
            s, c = inf.compute_stoi(_cuda(rec["y"]), _cuda(rec["x"]), extended=ext, counts=True)
            assert s.shape == () and s.dtype == torch.float32 and c.shape == (3,)
            out[key + (ext,)] = (s.cpu(), tuple(c.cpu().tolist()))
    return out


def test_counts_match_the_reference(ref, dev):
    """(frames, kept frames, segments) equal the float64 reference's.  Condition: every case's mask margin is >= 0.5 dB, so that
    an fp32 energy cannot flip a frame."""
    for key, rec in ref.items():
        for ext in (False, True):
            (_, counts, margin), _ = rec[ext]
            assert margin >= 0.5, (key, margin)
            assert dev[key + (ext,)][1] == counts, (key, ext, dev[key + (ext,)][1], counts)
    assert ref[("one_segment", 0)][True][0][1] == (57, 31, 1) and ref[("range_edge", 0)][True][0][1][0] == 40


def test_values_within_four_float32_floors(ref, dev):
    """|device - float64 reference| <= 4 x the largest deviation of the float32 reference from the float64 one over these cases
    (8 cases x 3 SNRs x STOI / ESTOI); the factor 4 covers the device's other summation orders (MFMA accumulation, tree
    reductions), and the bound may never exceed 1e-4 (the evaluation scripts print two decimals).

    Measured on the MI355X: the float32 reference's largest deviation 1.45e-7, so the bound is 5.8e-7; the
    device's largest deviation 2.0e-7 (the 3.6 s case, ESTOI at 20 dB; 1.1e-7 on the seven short cases; its output is a float32)."""
    floor = max(abs(rec[ext][1][0] - rec[ext][0][0]) for rec in ref.values() for ext in (False, True))
    bound = 4 * floor
    worst = 0.0
    for key, rec in ref.items():
        for ext in (False, True):
            d = abs(float(dev[key + (ext,)][0]) - rec[ext][0][0])
            worst = max(worst, d)
            print("stoi", key, "estoi" if ext else "stoi", "ref", rec[ext][0][0], "device", float(dev[key + (ext,)][0]), "dev", d)
    print("float32 reference floor", floor, "bound", bound, "device worst", worst)
    assert 0 < bound <= 1e-4
    assert worst <= bound
    for snr in R.SNRS:
        for ext in (False, True):
            assert float(dev[("too_few", snr, ext)][0]) == ONE_E5


def test_rows_are_independent(ref, dev):
    """Cases 1, 2, 3 and 6 in one padded batch with NaN in the padding: every row is bit-identical to the utterance scored alone at
    B = 1, counts included; the too-few-frames row is exactly 1e-5.  Then the same rows behind the 3.6 s case: a wider batch and
    other launch grids, a row of several workgroups per stage, the same bits."""
    inf = _inf()
    names = ["compaction", "near_30", "too_few", "longer"]
    for names, snr in ((names, 0), (names, -5), (["many_blocks"] + names, 0)):
        recs = [ref[(nm, snr)] for nm in names]
        lens = [len(r["x"]) for r in recs]
        x = torch.full((len(names), max(lens) + 37), float("nan"))
        y = torch.full((len(names), max(lens) + 37), float("nan"))
        for b, r in enumerate(recs):
            x[b, :lens[b]] = torch.from_numpy(r["x"])
            y[b, :lens[b]] = torch.from_numpy(r["y"])
        for ext in (False, True):
            s, c = inf.compute_stoi(y.cuda(), x.cuda(), extended=ext, lengths=lens, counts=True)
            s, c = s.cpu(), c.cpu()
            assert torch.isfinite(s).all()
            for b, nm in enumerate(names):
                alone_s, alone_c = dev[(nm, snr, ext)]
                assert s[b].item() == alone_s.item() and torch.equal(s[b].view(torch.int32), alone_s.view(torch.int32)), (nm, snr, ext)
                assert tuple(c[b].tolist()) == alone_c
            assert s[names.index("too_few")].item() == ONE_E5
            # without counts, and with the two inputs padded to different widths
            s2 = inf.compute_stoi(y.cuda(), x[:, :max(lens)].cuda(), extended=ext, lengths=torch.tensor(lens))
            assert torch.equal(s2.cpu(), s)


def test_degenerate_rows(ref):
    """A zero estimate and a zero reference give finite values equal to the reference's, 0.0."""
    inf = _inf()
    x = ref[("compaction", 0)]["x"]
    z = np.zeros_like(x)
    for ext in (False, True):
        for a, b in ((x, z), (z, x), (z, z)):                                 # (reference, estimate)
            want = R.stoi(a, b, 16000, ext)[0]
            got = float(inf.compute_stoi(_cuda(b), _cuda(a), extended=ext))
            assert want == 0.0 and np.isfinite(got) and got == 0.0, (ext, got)


def test_10khz_input_skips_the_resampler(ref):
    """fs=10000 on a pre-resampled signal: the later stages alone, against the float64 reference on the same 10 kHz signals."""
    inf = _inf()
    floor = max(abs(rec[ext][1][0] - rec[ext][0][0]) for rec in ref.values() for ext in (False, True))
    for name in ("compaction", "range_edge", "range_next"):
        rec = ref[(name, 0)]
        x10, y10 = R.resample(rec["x"]).astype(np.float32), R.resample(rec["y"]).astype(np.float32)
        for ext in (False, True):
            want, counts, margin = R.stoi(x10, y10, 10000, ext)
            assert margin >= 0.5 and counts == rec[ext][0][1]
            s, c = inf.compute_stoi(_cuda(y10), _cuda(x10), fs=10000, extended=ext, counts=True)
            print("10 kHz", name, ext, want, float(s))
            assert tuple(c.cpu().tolist()) == counts
            assert abs(float(s) - want) <= 4 * floor


def test_rmse(ref):
    inf = _inf()
    names = ["compaction", "near_30", "longer"]
    recs = [ref[(nm, 0)] for nm in names]
    lens = [len(r["x"]) for r in recs]
    for r in recs:                                                            # alone, no lengths
        want = R.rmse(r["y"], r["x"])
        got = float(inf.compute_rmse(_cuda(r["y"]), _cuda(r["x"])))
        assert abs(got - want) <= 1e-6 * want, (got, want)
    x = torch.full((3, max(lens)), float("nan"))
    y = torch.full((3, max(lens)), float("nan"))
    for b, r in enumerate(recs):
        x[b, :lens[b]] = torch.from_numpy(r["x"])
        y[b, :lens[b]] = torch.from_numpy(r["y"])
    got = inf.compute_rmse(y.cuda(), x.cuda(), lengths=lens).cpu()
    for b, r in enumerate(recs):
        want = R.rmse(r["y"], r["x"])
        assert abs(float(got[b]) - want) <= 1e-6 * want
    n = min(lens)                                                             # a full batch without lengths
    got = inf.compute_rmse(y[:, :n].cuda(), x[:, :n].cuda()).cpu()
    for b, r in enumerate(recs):
        want = R.rmse(r["y"][:n], r["x"][:n])
        assert abs(float(got[b]) - want) <= 1e-6 * want


def test_score_list(ref, dev):
    """The six table cases (and the one-segment one) in shuffled order: the caller's order comes back, and every value equals the
    per-utterance call bit for bit.  The estimates are a few samples longer than the references: pairs are scored over min(len)."""
    inf = _inf()
    order = [3, 6, 0, 5, 2, 4, 1]
    recs = [ref[(R.CASES[k][0], 0)] for k in order]
    est = [torch.cat([_cuda(r["y"]), torch.ones(k, device="cuda")]) for k, r in enumerate(recs)]
    refs = [_cuda(r["x"]) for r in recs]
    metrics = ("sisdr", "estoi", "stoi", "rmse")
    got = inf.score_list(est, refs, metrics=metrics, max_batch=3)
    assert sorted(got) == sorted(metrics)
    for m in metrics:
        assert got[m].shape == (7,) and got[m].dtype == torch.float32 and not got[m].is_cuda
    for k, r in enumerate(recs):
        e, x = _cuda(r["y"]), _cuda(r["x"])
        name = R.CASES[order[k]][0]
        assert got["estoi"][k].item() == dev[(name, 0, True)][0].item()
        assert got["stoi"][k].item() == dev[(name, 0, False)][0].item()
        assert got["sisdr"][k].item() == inf.compute_sisdr(e, x).item()
        assert got["rmse"][k].item() == inf.compute_rmse(e, x).item()
    assert sorted(inf.score_list(est, refs)) == ["estoi", "sisdr"]
