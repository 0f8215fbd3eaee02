"""CPU tests of reverberation: the host definition tests/reverb_ref.py (the yardstick of tests/test_gpu_reverb.py)
against scipy, the conditions under which the GPU tests demand equal bits, draw_reverb, the peaks of a RirPool and the host-side guards
of dataset/reverb.py and of the new arguments of dataset/mix.py; no GPU and no library load."""
import importlib
import os
import sys

import numpy as np
import pytest
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import reverb_ref as R  # noqa: E402

MIX = importlib.import_module("i-dccrn-vae_amd.dataset.mix")
RV = importlib.import_module("i-dccrn-vae_amd.dataset.reverb")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")


def test_cases_are_what_the_gpu_tests_assume():
    rows = R.cases()
    assert [(len(x), len(h)) for x, h in rows] == R.SHAPES
    assert R.SHAPES == [(1, 1), (5, 16), (63, 17), (64, 15), (257, 33), (1025, 255), (1601, 1024), (3201, 4097), (4097, 257), (8193, 8192),
                        (16385, 4097), (100, 4097), (12000, 16384)]
    for x, h in rows:
        assert x.dtype == np.float32 and h.dtype == np.float32 and np.isfinite(x).all() and np.isfinite(h).all()
        assert (x * 32768 == np.round(x * 32768)).all() and np.abs(x).max() <= 0.8             # PCM16
        assert not np.signbit(x[x == 0]).any()                                                # no negative zero
        assert np.abs(h).max() >= 1.0 and h[min(len(h) // 8, 40)] == 1.0                       # the unit peak behind the pre-delay


def test_definition_against_scipy():
    """Within 2^-53 log2(n + K) ||x|| ||h|| of scipy.signal.fftconvolve(x, h)[:n], the function the synthesizer calls."""
    worst = 0.0
    for x, h in R.cases():
        n, K = len(x), len(h)
        y, S = R.reverb(x, h)
        want = scipy.signal.fftconvolve(x.astype(np.float64), h.astype(np.float64), "full")[:n]
        tol = 2.0 ** -53 * np.log2(n + K) * np.linalg.norm(x.astype(np.float64)) * np.linalg.norm(h.astype(np.float64))
        err = float(np.abs(y - want).max())
        assert y.shape == (n,) and S.shape == (n,) and (S >= np.abs(y) * (1 - 1e-12)).all()
        assert err <= tol, (n, K, err, tol)
        worst = max(worst, err / tol)
    print(f"definition against fftconvolve: worst ratio to the bound {worst:.3f}")


def test_definition_by_hand_and_taps():
    y, S = R.reverb([1.0, 2.0, -3.0], [0.5, 0.25, 4.0])
    assert y.tolist() == [0.5, 1.25, 3.0] and S.tolist() == [0.5, 1.25, 6.0]
    assert R.reverb([1.0, 2.0, -3.0], [0.5, 0.25, 4.0], taps=2)[0].tolist() == [0.5, 1.25, -1.0]
    assert R.reverb([1.0, 2.0, -3.0], [0.5, 0.25, 4.0], history=[7.0, 1.0])[0].tolist() == [0.5 + 0.25 + 28.0, 1.0 + 0.25 + 4.0, -1.5 + 0.5 + 4.0]


def test_history_equals_convolving_the_recording_and_cutting():
    rng = np.random.default_rng(3)
    rec = R.speech_row(3000, 50)
    for K in (1, 2, 16, 17, 300):
        h = R.rir_row(K, 60 + K)
        whole, whole_S = R.reverb(rec, h)
        for s0, n in ((0, 100), (1, 100), (15, 64), (K - 1, 500), (K + 100, 257), (3000 - 40, 40)):
            for H in {min(s0, K - 1), s0}:                             # the K - 1 samples that can matter, or all of them
                y, S = R.reverb(rec[s0:s0 + n], h, history=rec[s0 - H:s0])
                # the same K terms, in whatever order np.convolve adds them for these operand lengths: two sums, K 2^-53 S each
                tol = 2.0 * K * 2.0 ** -53 * whole_S[s0:s0 + n]
                assert (np.abs(y - whole[s0:s0 + n]) <= tol).all() and (np.abs(S - whole_S[s0:s0 + n]) <= tol).all(), (K, s0, n, H)
        taps = int(rng.integers(1, K + 1))
        assert np.array_equal(R.reverb(rec, h, taps=taps)[0], R.reverb(rec, h[:taps])[0])
    # exactly, where every sum is exact: integer samples and taps
    rec_i, h_i = np.round(rec.astype(np.float64) * 32768), np.arange(1.0, 18.0)
    whole = R.reverb(rec_i, h_i)[0]
    for s0, n in ((0, 100), (1, 100), (15, 64), (16, 500), (117, 257), (3000 - 40, 40)):
        assert np.array_equal(R.reverb(rec_i[s0:s0 + n], h_i, history=rec_i[s0 - min(s0, 16):s0])[0], whole[s0:s0 + n])
        if s0 > 3:                                                             # too short a history is not the recording
            assert not np.array_equal(R.reverb(rec_i[s0:s0 + n], h_i, history=rec_i[s0 - 3:s0])[0], whole[s0:s0 + n])


def test_dyadic_set_is_exact_in_any_order():
    """Every product an integer multiple of 2^-23 and every S[i] 2^23 below 2^53: any summation order in double is exact."""
    rows = R.dyadic_cases()
    assert [(len(x), len(h)) for x, h in rows] == [s for s in R.SHAPES if s[1] <= 4097] and len(rows) == 11
    for x, h in rows:
        assert len(h) <= 4097 and np.abs(h).max() < 1.0 and (h * 256 == np.round(h * 256)).all() and np.abs(h).max() > 0
        assert (x * 32768 == np.round(x * 32768)).all()
        xi, hi = np.round(x.astype(np.float64) * 32768), np.round(h.astype(np.float64) * 256)    # x = xi 2^-15, h = hi 2^-8: products hi xi 2^-23
        assert np.array_equal(xi * 2.0 ** -15, x.astype(np.float64)) and np.array_equal(hi * 2.0 ** -8, h.astype(np.float64))
        y, S = R.reverb(x, h)
        assert float(S.max()) * 2.0 ** 23 < 2.0 ** 53
        assert np.array_equal(y * 2.0 ** 23, np.round(y * 2.0 ** 23))
        assert np.array_equal(y, np.convolve(xi, hi)[:len(x)] * 2.0 ** -23)                      # the integer convolution, exact


def test_draw_reverb():
    a = RV.draw_reverb(3, 123, 5, 8)
    assert a == [-1, 4, 4, -1, 1, 4, 3, -1] and RV.draw_reverb(0, 7, 5, 8, 0.25) == [-1, -1, -1, -1, -1, -1, 3, -1]
    for k in (0, 9, 2):                                                  # no state
        RV.draw_reverb(k, 123, 5, 8)
    assert a == RV.draw_reverb(3, 123, 5, 8)
    assert a != RV.draw_reverb(4, 123, 5, 8) and a != RV.draw_reverb(3, 124, 5, 8)
    assert RV.draw_reverb(3, 123, 5, 64, 0.0) == [-1] * 64
    full = RV.draw_reverb(3, 123, 5, 64, 1.0)
    assert all(0 <= r < 5 for r in full) and set(full) == {0, 1, 2, 3, 4}
    # p decides wet or dry only: the response of a wet row is the same at every p
    assert all(r in (-1, f) for r, f in zip(RV.draw_reverb(3, 123, 5, 64, 0.5), full))
    wet = sum(r >= 0 for k in range(50) for r in RV.draw_reverb(k, 1, 3, 64, 0.5))
    assert 0.45 < wet / 3200 < 0.55
    for kw in (dict(k=-1), dict(k=1.5), dict(seed=True), dict(n_rirs=0), dict(batch=0), dict(p=-0.1), dict(p=1.5), dict(p="1"),
               dict(p=float("nan"))):
        with pytest.raises(ValueError, match="draw_reverb"):
            RV.draw_reverb(**dict(dict(k=0, seed=1, n_rirs=3, batch=4), **kw))


def test_draw_batch_returns_what_it_returned_before():
    """Literal values of the commit before draw_reverb existed: its generator is its own."""
    cl, nl = [70000, 64000, 500, 200000], [1, 16000, 480000]
    RV.draw_reverb(3, 123, 5, 8)
    assert tuple(MIX.draw_batch(3, 123, cl, nl, 3, 64000)) == (
        [3, 0, 0], [108583, 5714, 5169], [64000, 64000, 64000], [2, 2, 2], [81110, 477646, 342199],
        [16.461939934176783, 12.446826832732924, -3.3877054823073998], [-18.0, -20.0, -23.0])
    assert tuple(MIX.draw_batch(0, 7, cl, nl, 3, 64000)) == (
        [2, 3, 3], [0, 70058, 86], [500, 64000, 64000], [1, 2, 0], [13510, 278246, 0],
        [-2.3044040007580104, 19.937130925008734, 14.674685727454307], [-21.0, -19.0, -20.0])


def test_peaks_and_early_taps():
    h0 = np.array([0.0, 0.1, -1.0, 0.5, 1.0, 0.2], dtype=np.float32)          # a tie of |h|: the first wins
    h1 = torch.tensor([0.1, 0.2, 0.3, -0.9])                                   # the peak is the last sample
    h2 = np.zeros(2000, dtype=np.float32)
    h2[7] = -2.0
    h3 = np.array([3.0], dtype=np.float32)
    peaks = RV.rir_peaks([h0, h1, h2, h3])
    assert peaks == [2, 3, 7, 0]
    lens = [6, 4, 2000, 1]
    assert RV.early_taps(lens, peaks, 50.0, 16000) == [6, 4, 808, 1]           # 7 + 1 + 800
    assert RV.early_taps(lens, peaks, 0.0, 16000) == [3, 4, 8, 1]              # the direct sound alone
    assert RV.early_taps(lens, peaks, 0.1, 16000) == [5, 4, 10, 1]             # round(1.6) = 2
    assert RV.early_taps(lens, peaks, 50.0, 8000) == [6, 4, 408, 1]
    for kw in (dict(ms=-1.0), dict(ms=float("nan")), dict(ms="5"), dict(fs=0), dict(fs=16000.0)):
        with pytest.raises(ValueError, match="early_taps"):
            RV.early_taps(lens, peaks, **kw)


def test_guards_raise_before_gpu_work():
    x, h = torch.zeros(3, 500), torch.zeros(3, 40)
    bad = [((x[0], h), {}, "x must be a \\[B, L\\]"), ((x, h[0]), {}, "rir must be a \\[B, K\\]"), (("x", h), {}, "x must be"),
           ((x.double(), h), {}, "float32"), ((x, h.half()), {}, "float32"), ((x[:0], h[:0]), {}, "65535"), ((x[:, :0], h), {}, "2\\^27"),
           ((x, h[:, :0]), {}, "taps"), ((x, torch.zeros(1, 1).expand(3, (1 << 16) + 1)), {}, "65536"), ((x, h[:2]), {}, "2 impulse responses"),
           ((torch.zeros(1, 1).expand(1, (1 << 27) + 1), h[:1]), {}, "2\\^27"),
           ((x, h), dict(lengths=[500, 10]), "2 lengths"), ((x, h), dict(lengths=[501, 1, 1]), "exceeds"), ((x, h), dict(lengths=[5, 0, 1]), "positive"),
           ((x, h), dict(rir_lengths=[40, 41, 1]), "rir_lengths\\[1\\]"), ((x, h), dict(rir_lengths=[40, 0, 1]), "rir_lengths\\[1\\]"),
           ((x, h), dict(rir_lengths=[40, 1]), "2 values of rir_lengths"), ((x, h), dict(rir_lengths=[40.0, 1, 1]), "integers"),
           ((x, h), dict(taps=0), "taps\\[0\\]"), ((x, h), dict(taps=41), "taps\\[0\\]"), ((x, h), dict(taps=[1, 2]), "2 values of taps"),
           ((x, h), dict(taps=[1, True, 2]), "integers"), ((x, h), dict(taps="4"), "taps must be"), ((x, h), dict(taps=2.0), "taps must be"),
           ((x, h), dict(taps=torch.tensor([1.0, 2.0, 3.0])), "taps must be"),
           ((x, h), dict(rir_lengths=[40, 10, 40], taps=[40, 11, 1]), "taps\\[1\\]")]
    for args, kw, what in bad:
        with pytest.raises(ValueError, match=what):
            RV.reverb(*args, **kw)
    # all value guards passed: the CPU tensors are refused before any launch
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        RV.reverb(x, h[:1], lengths=[500, 1, 77], rir_lengths=[40, 40, 3], taps=[1, 40, 3])
    r = torch.zeros(100)
    for sig, kw, what in (([r], dict(fs=0), "fs"), ([r], dict(fs=16000.0), "fs"), ([r, torch.zeros(1).expand((1 << 16) + 1)], {}, "response 1.*65536"),
                          ([np.zeros((1 << 16) + 1, dtype=np.float32)], {}, "response 0")):
        with pytest.raises(ValueError, match="RirPool.*" + what):
            RV.RirPool(sig, **kw)
    for sig, kw, what in (([], {}, "non-empty"), ([r.double()], {}, "signal 0"), ([r], dict(device="cpu"), "not a GPU")):
        with pytest.raises(ValueError, match="SignalPool.*" + what):
            RV.RirPool(sig, **kw)
    d = MIX.Draw([0], [0], [10], [0], [0], [5.0], [-25.0])
    with pytest.raises(ValueError, match="reverb_draw: clean_pool must be a SignalPool and rir_pool a RirPool"):
        RV.reverb_draw([r], [r], d, [-1], 100)
    with pytest.raises(ValueError, match="SignalPool objects"):
        MIX.mix_draw([r], [r], d, 100, clean=x)


def test_dynamic_mixtures_checks_its_new_arguments():
    """The new arguments are checked whether or not a pool is given: nothing is accepted and ignored."""
    for kw, what in ((dict(p_reverb=1.5), "p_reverb"), (dict(p_reverb=-0.1), "p_reverb"), (dict(p_reverb="0.5"), "p_reverb"),
                     (dict(p_reverb=True), "p_reverb"), (dict(target="dry"), "target"), (dict(target=None), "target"),
                     (dict(early_ms=-1.0), "early_ms"), (dict(early_ms=float("inf")), "early_ms"), (dict(early_ms="50"), "early_ms"),
                     (dict(rir_pool=[torch.zeros(4)]), "rir_pool must be a RirPool"), (dict(rir_pool=0), "rir_pool must be a RirPool")):
        with pytest.raises(ValueError, match="DynamicMixtures: " + what):
            MIX.DynamicMixtures(None, None, 4, **kw)
    with pytest.raises(TypeError):
        MIX.DynamicMixtures(None, None, 4, reverb=True)
    with pytest.raises(ValueError, match="SignalPool objects"):                # as before
        MIX.DynamicMixtures(None, None, 4, rir_pool=None, p_reverb=1.0, target="early", early_ms=0.0)
