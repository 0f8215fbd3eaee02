"""CPU tests of mixture synthesis: the host reference tests/mix_ref.py (the yardstick of tests/test_gpu_mix.py) and the
conditions under which the GPU tests compare decisions exactly, draw_batch, and the host-side guards of dataset/mix.py; no GPU and no
library load."""
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

import mix_ref as R  # noqa: E402

MIX = importlib.import_module("i-dccrn-vae_amd.dataset.mix")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")

MARGIN = 1e-6


@pytest.fixture(scope="module")
def table():
    """Every case of the GPU tests: (row index, snr, level, segmental) -> the reference's result."""
    rows = R.cases()
    return rows, {(k, snr, lev, seg): R.mix(c, v, o, snr, lev, seg) for k, (c, v, o) in enumerate(rows) for snr, lev, seg in R.grid()}


def test_cases_are_what_the_gpu_tests_assume():
    rows = R.cases()
    assert [len(c) for c, _, _ in rows] == R.LENGTHS and max(R.LENGTHS) == 16385 and len(R.grid()) == 32
    for k, (c, v, o) in enumerate(rows):
        n = len(c)
        assert len(v) == [n, max(1, n // 3), n + 7, 1][k % 4] and o == [0, len(v) // 2, len(v) - 1, 0][k % 4] and 0 <= o < len(v)
        for x in (c, v):                                        # PCM16 values: k / 32768 with |k| <= 0.8 * 32767
            q = x.astype(np.float64) * 32768
            assert x.dtype == np.float32 and np.array_equal(q, np.round(q)) and np.abs(q).max() <= 26214
    # sums of squares of such rows are integers below 2^53 times 2^-30
    assert 16385 * 26214 ** 2 < 2 ** 53
    assert np.array_equal(R.cyclic(np.arange(5), 12, 3), [3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4])


def test_reference_by_hand():
    """Two samples each, plain mode: every step written out."""
    c, v = np.array([0.5, -0.25]), np.array([0.125, -0.25])
    r = R.mix(c, v, 0, 6.0, -20.0)
    t = 10 ** (-25 / 20)
    c2 = c / np.sqrt(np.mean(c ** 2)) * t
    v3 = v / np.sqrt(np.mean(v ** 2)) * t / 10 ** (6 / 20)
    y = c2 + v3
    s = 10 ** (-20 / 20) / np.sqrt(np.mean(y ** 2))
    assert np.allclose(r["noisy_f64"], y * s, rtol=1e-12, atol=0) and np.allclose(r["clean_f64"], c2 * s, rtol=1e-12, atol=0)
    assert not r["clipped"] and r["active"] == 2 and abs(r["level_db"] + 20.0) < 1e-9
    assert np.allclose(r["g_clean"] * c, r["clean_f64"], rtol=1e-13, atol=0) and np.allclose(r["g_noise"] * v, r["noise_f64"], rtol=1e-13, atol=0)
    # the same row at a level it cannot hold: scaled to the clip threshold
    r = R.mix(c, v, 0, 6.0, 0.0)
    assert r["clipped"] and abs(np.abs(r["noisy_f64"]).max() - 0.99) < 1e-12 and r["level_db"] < 0
    # the noise read from offset 1 of a one-sample-longer row is the same noise
    r1, r2 = R.mix(c, np.array([9.0, 0.125, -0.25]), 1, 6.0), R.mix(c, v, 0, 6.0)
    assert np.array_equal(r1["noisy"], r2["noisy"])
    # segmental: the silent second window does not count, so the SNR holds over the first window alone
    c = np.concatenate([np.full(1600, 0.25), np.full(800, 0.5)])
    v = np.concatenate([np.tile([0.125, -0.125], 800), np.zeros(800)])
    r = R.mix(c, v, 0, 10.0, segmental=True)
    assert r["active"] == 1600 and r["window_db"][1] == 10 * np.log10(R.EPS)
    assert abs(10 * np.log10(np.sum(r["clean_f64"][:1600] ** 2) / np.sum(r["noise_f64"][:1600] ** 2)) - 10.0) < 1e-9


def test_reference_properties(table):
    """Realised SNR over the row in plain mode, realised level where the row is not clipped, the peak at the threshold where it is;
    the gains reproduce the outputs; everything finite."""
    rows, tab = table
    for (k, snr, lev, seg), r in tab.items():
        c, _, _ = rows[k]
        assert all(np.isfinite(r[f]).all() for f in ("noisy", "clean_out", "noise_out", "g_clean", "g_noise", "level_db")), (k, snr, lev, seg)
        if not seg and c.any() and r["v"].any():
            got = 10 * np.log10(np.sum(r["clean_f64"] ** 2) / np.sum(r["noise_f64"] ** 2))
            assert abs(got - snr) < 1e-9, (k, snr, lev, got)
        if r["clipped"]:
            assert np.abs(r["noisy_f64"]).max() <= 0.99 and np.abs(r["noisy"]).max() <= np.float32(0.99)
            assert r["level_db"] < lev
        elif r["noisy_f64"].any():
            assert abs(r["level_db"] - lev) < 1e-9, (k, snr, lev, seg)
        assert np.allclose(r["g_clean"] * c.astype(np.float64), r["clean_f64"], rtol=1e-12, atol=0)
        assert np.allclose(r["g_noise"] * r["v"].astype(np.float64), r["noise_f64"], rtol=1e-12, atol=0)
        assert r["active"] == len(c) if not seg else 0 <= r["active"] <= len(c)


def test_conditions_of_the_gpu_tests(table):
    """What makes the exact comparisons of tests/test_gpu_mix.py statements about the kernels and not about a pow or a log10: every
    case stands at least 1e-6 from the clip threshold in max|y| and every window at least 1e-6 dB from thresh_db, in the reference
    alone.  Measured on these 768 cases: 150 clip, the nearest stands 0.00279 from 0.99, the nearest window 1.14 dB from -50 dB, 64
    segmental cases have some but not all samples active.  And no case is ill-conditioned: where clean and scaled noise cancel (one
    sample each, opposite signs, 0 dB) rms(y) is rounding noise in the reference as on the device and no gain can be compared; the
    factor ``cancel`` by which a rounding of either signal is amplified in rms(y) is at most 1.68 here, 1000 is demanded."""
    rows, tab = table
    assert len(tab) == 24 * 4 * 4 * 2
    clip_margin = min(R.clip_margin(r) for r in tab.values())
    window_margin = min(R.window_margin_db(r) for r in tab.values())
    clipped = sum(r["clipped"] for r in tab.values())
    partial = sum(1 for (k, _, _, seg), r in tab.items() if seg and 0 < r["active"] < len(rows[k][0]))
    print(f"mix: {clipped} of {len(tab)} cases clip, nearest {clip_margin:.4g} from the threshold; nearest window {window_margin:.4g} dB "
          f"from thresh_db; {partial} segmental cases partly active")
    assert clip_margin >= MARGIN and window_margin >= MARGIN
    assert 0 < clipped < len(tab) and partial >= 1
    assert (clipped, partial) == (150, 64) and abs(clip_margin - 0.00279) < 1e-5 and abs(window_margin - 1.14) < 1e-2
    assert max(r["cancel"] for r in tab.values()) <= 1000.0
    # the float32 rows and the degenerate rows of the GPU tests keep the same margins
    for c, v, o in R.float_cases():
        for seg in (False, True):
            r = R.mix(c, v, o, 5.0, -25.0, seg)
            assert R.clip_margin(r) >= MARGIN and R.window_margin_db(r) >= MARGIN and r["cancel"] <= 1000.0


def test_degenerate_rows_are_finite():
    z, one = np.zeros(100, dtype=np.float32), R.clean_row(100, 0)
    for c, v in ((z, one), (one, z), (z, z), (one[:1], one), (one, one[:1]), (one[:1], one[:1])):
        for seg in (False, True):
            r = R.mix(c, v, 0, 5.0, -25.0, seg)
            assert all(np.isfinite(r[f]).all() for f in ("noisy", "clean_out", "noise_out", "g_clean", "g_noise", "level_db"))
            if not v.any():
                assert np.array_equal(r["noisy"], r["clean_out"]) and r["active"] == (0 if seg else len(c))
            if not c.any():
                assert not r["noisy"].any()


def test_draw_batch():
    cl, nl = [70000, 64000, 500, 200000], [1, 16000, 480000]
    a = MIX.draw_batch(3, 123, cl, nl, 64, 64000)
    assert a == MIX.draw_batch(3, 123, cl, nl, 64, 64000)                      # a function of its arguments
    assert a != MIX.draw_batch(4, 123, cl, nl, 64, 64000) and a != MIX.draw_batch(3, 124, cl, nl, 64, 64000)
    # no state: batch 3 after other batches, or after none, is the same
    for k in (0, 7, 2):
        MIX.draw_batch(k, 123, cl, nl, 64, 64000)
    assert a == MIX.draw_batch(3, 123, cl, nl, 64, 64000)
    seen_c, seen_n, levels = set(), set(), set()
    for k in range(20):
        d = MIX.draw_batch(k, 9, cl, nl, 64, 64000)
        assert all(len(f) == 64 for f in d)
        for b in range(64):
            n, m = cl[d.clean_id[b]], nl[d.noise_id[b]]
            assert d.lens[b] == min(n, 64000) and 0 <= d.clean_start[b] <= n - d.lens[b] and 0 <= d.noise_offset[b] < m
            assert (d.clean_start[b] == 0) if n <= 64000 else True
            assert -5.0 <= d.snr_db[b] <= 20.0 and d.level_db[b] == int(d.level_db[b]) and -35 <= d.level_db[b] < -15
            assert isinstance(d.lens[b], int) and isinstance(d.clean_start[b], int) and isinstance(d.noise_offset[b], int)
        seen_c |= set(d.clean_id)
        seen_n |= set(d.noise_id)
        levels |= set(d.level_db)
    assert seen_c == {0, 1, 2, 3} and seen_n == {0, 1, 2} and levels == set(float(v) for v in range(-35, -15))
    d = MIX.draw_batch(0, 1, cl, nl, 8, 1000, snr_db=(0.0, 1.0), level_db=(-20, -19))
    assert all(0.0 <= s <= 1.0 for s in d.snr_db) and set(d.level_db) == {-20.0} and set(d.lens) <= {1000, 500}
    for kw in (dict(k=-1), dict(k=1.0), dict(seed=True), dict(batch=0), dict(samples=0), dict(clean_lengths=[]), dict(noise_lengths=[0]),
               dict(clean_lengths=[1.5]), dict(snr_db=(5.0, 5.0)), dict(snr_db=(0.0, float("inf"))), dict(snr_db=5.0),
               dict(level_db=(-20.5, -10)), dict(level_db=(-10, -20))):
        args = dict(k=0, seed=1, clean_lengths=cl, noise_lengths=nl, batch=4, samples=100)
        args.update(kw)
        with pytest.raises(ValueError, match="draw_batch"):
            MIX.draw_batch(**args)


def test_guards_raise_before_gpu_work():
    c, v = torch.zeros(3, 500), torch.zeros(3, 200)
    bad = [(dict(snr_db=float("nan")), "snr_db"), (dict(snr_db=[0.0, 1.0]), "2 values of snr_db"), (dict(snr_db="5"), "snr_db"),
           (dict(snr_db=[0.0, 1.0, float("inf")]), "snr_db\\[2\\]"), (dict(level_db=True), "level_db"), (dict(level_db=[-25.0] * 4), "level_db"),
           (dict(target_db=float("inf")), "target_db"), (dict(thresh_db=None), "thresh_db"), (dict(clip=0.0), "clip"), (dict(clip=1.5), "clip"),
           (dict(clip=float("nan")), "clip"), (dict(win=0), "win"), (dict(win=1602), "win"), (dict(win=1600.0), "win"),
           (dict(win=(1 << 27) + 4), "win"), (dict(segmental=1), "segmental"),
           (dict(lengths=[500, 10]), "2 lengths for a batch of 3"), (dict(lengths=[501, 10, 10]), "exceeds"), (dict(lengths=[500, 0, 10]), "positive"),
           (dict(lengths=torch.tensor([1.0, 2.0, 3.0])), "integer"), (dict(noise_lengths=[200, 201, 1]), "exceeds"),
           (dict(noise_lengths=[200, 0, 1]), "positive"), (dict(noise_offsets=[0, 0, 200]), "noise_offsets\\[2\\]"),
           (dict(noise_offsets=[0, -1, 0]), "noise_offsets\\[1\\]"), (dict(noise_offsets=[0, 0]), "2 noise_offsets"),
           (dict(noise_offsets=[0, 0.5, 0]), "integers"), (dict(noise_offsets=5), "noise_offsets"),
           (dict(noise_lengths=[200, 50, 1], noise_offsets=[0, 50, 0]), "noise_offsets\\[1\\]")]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            MIX.snr_mix(c, v, **dict(dict(snr_db=5.0), **kw))
    for cc, vv, what in ((c[0], v, "\\[B, L\\]"), (c, v[:2], "2 noise rows"), (c.double(), v, "float32"), (c, v.half(), "float32"),
                         (c[:, :0], v, "2\\^27"), (c, v[:, :0], "2\\^27"), (c[:0], v[:0], "65535"), ("x", v, "\\[B, L\\]"),
                         (torch.zeros(1, 1).expand(1, (1 << 27) + 1), v[:1], "2\\^27")):
        with pytest.raises(ValueError, match=what):
            MIX.snr_mix(cc, vv, 5.0)
    # all value guards passed: the CPU tensors are refused before any launch
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        MIX.snr_mix(c, v, [0.0, 5.0, 10.0], -20.0, lengths=[500, 1, 77], noise_lengths=[200, 50, 1], noise_offsets=[199, 0, 0], segmental=True)
    x = torch.zeros(100)
    for sig, kw, what in (([], {}, "non-empty"), (x, {}, "non-empty"), ([x, x.double()], {}, "signal 1"), ([x, x[:0]], {}, "signal 1"),
                          ([x.view(10, 10)], {}, "signal 0"), ([np.zeros(5)], {}, "signal 0"), ([x], dict(device="cpu"), "not a GPU"),
                          ([torch.zeros(1).expand((1 << 27) + 1)], {}, "2\\^27")):
        with pytest.raises(ValueError, match="SignalPool.*" + what):
            MIX.SignalPool(sig, **kw)
    with pytest.raises(ValueError, match="SignalPool objects"):
        MIX.DynamicMixtures([x], [x], 4)
