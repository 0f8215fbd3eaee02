"""CPU tests of the BSS-eval SDR metric: the host reference tests/sdr_ref.py (it is the yardstick of tests/test_gpu_sdr.py, so its
cases must be ones for which the float64 definition itself is unambiguous) and the host-side guards of inference.compute_sdr /
score_list; no GPU needed."""
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

INF = importlib.import_module("i-dccrn-vae_amd.inference")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")


def test_cases_name_the_shapes_of_the_issue():
    want = {16: [1, 5, 15, 16, 17, 31, 33], 64: [63, 64, 65, 255, 257, 4001], 512: [300, 511, 512, 513, 1023, 1025, 16385]}
    got = {}
    for L, K, kind in R.CASES:
        assert kind in ("white", "lowpass")
        got.setdefault(K, []).append(L)
    assert got == want
    assert {R.case_snr(k) for k in range(len(R.CASES))} == {0, 20, 60}
    a, b = R.case_signals(5), R.case_signals(5)
    assert a[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])       # seeded


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_reference_is_unambiguous_on_every_case(index):
    """LU and Levinson agree within 1e-9 dB on the float64 definition and cond(G) <= 1e8: what keeps the GPU test honest."""
    L, K, kind = R.CASES[index]
    s, y = R.case_signals(index)
    lu, lev = R.sdr(s, y, K), R.sdr(s, y, K, solver="levinson")
    assert R.condition(lu["r"]) <= 1e8
    assert lu["sdr"] == lev["sdr"] or abs(lu["sdr"] - lev["sdr"]) <= 1e-9, (lu["sdr"], lev["sdr"])
    assert not math.isnan(lu["sdr"]) and lu["target_energy"] > 0
    assert R.residual(lu["filter"], lu["r"], lu["d"]) < 1e-13


def test_reference_behaviour():
    s = R.reference(4000, "lowpass", seed=3)
    # an exactly filtered copy (the reference ends in silence, so the cut at its length takes nothing of the channel's tail away):
    # the filter is found, nothing is left
    s[-8:] = 0
    y = np.convolve(s.astype(np.float64), R.CHANNEL)[:4000]
    a = R.sdr(s, y, 64)
    assert np.abs(a["filter"][:9] - R.CHANNEL).max() < 1e-9 and np.abs(a["filter"][9:]).max() < 1e-9
    assert a["sdr"] > 80 and R.sisdr(y, s) < 0                               # the delay alone sinks SI-SDR
    # the direct lag sums are the FFT form of the package
    n = 1 << 14
    sf = np.fft.rfft(np.asarray(s, dtype=np.float64), n)
    assert np.abs(np.fft.irfft(sf * np.conj(sf), n)[:64] - a["r"]).max() <= 1e-14 * a["r"][0]
    assert np.abs(np.fft.irfft(np.conj(sf) * np.fft.rfft(y, n), n)[:64] - a["d"]).max() <= 1e-14 * a["r"][0]
    # the special rows
    z = np.zeros(4000)
    assert math.isnan(R.sdr(z, s, 64)["sdr"]) and R.sdr(s, z, 64)["sdr"] == -np.inf
    one = R.sdr(s[:1], 0.5 * s[:1], 16)
    assert one["sdr"] == np.inf or one["sdr"] > 250                          # K taps explain one sample exactly
    with pytest.raises(ValueError):
        R.sdr(s, y[:-1], 64)


def test_rationale_of_the_issue():
    """A 40-tap channel that delays by 7 samples plus noise at -20 dB: SI-SDR is far below 0 dB, the 512-tap SDR is near +20 dB."""
    rng = np.random.default_rng(7)
    s = R.reference(16000, "lowpass", seed=11).astype(np.float64)
    h = np.zeros(40)
    h[7:] = rng.standard_normal(33) * np.exp(-np.arange(33) / 6.0)
    y = np.convolve(s, h)[:16000]
    nz = rng.standard_normal(16000)
    y = y + nz * np.sqrt(np.sum(y * y) / np.sum(nz * nz) / 100.0)
    assert R.sisdr(y, s) < -5 and 17 < R.sdr(s, y, 512)["sdr"] < 22


def test_filt_len_guards():
    e, r = torch.zeros(2, 2000), torch.zeros(2, 2000)
    for bad in (0, 8, 24, 520, 1024, True, 512.0, -16, None, "512"):
        with pytest.raises(ValueError, match="filt_len"):
            INF.compute_sdr(e, r, filt_len=bad)
    for good in (16, 64, 496, 512):
        with pytest.raises(LIB.IdvError, match="no CPU fallback"):           # every value guard passed
            INF.compute_sdr(e, r, filt_len=good)


def test_guards_raise_before_gpu_work():
    e, r = torch.zeros(3, 2000), torch.zeros(3, 2000)
    ok = [2000, 1500, 300]
    fn = INF.compute_sdr
    with pytest.raises(ValueError, match="must be tensors"):
        fn(e.numpy(), r)
    with pytest.raises(ValueError, match="expected"):
        fn(e[None], r[None])
    with pytest.raises(ValueError, match="batch size"):
        fn(e, r[:2], lengths=ok)
    with pytest.raises(ValueError, match="differ"):
        fn(e, r[:, :1999])
    with pytest.raises(ValueError, match="empty"):
        fn(e[:, :0], r[:, :0])
    with pytest.raises(ValueError, match="2 lengths for a batch of 3"):
        fn(e, r, lengths=ok[:2])
    with pytest.raises(ValueError, match="exceeds"):
        fn(e, r, lengths=[2001, 1500, 300])
    with pytest.raises(ValueError, match="exceeds"):
        fn(e, r[:, :1999], lengths=ok)                                       # beyond the shorter row
    with pytest.raises(ValueError, match="positive"):
        fn(e, r, lengths=[2000, 0, 300])
    with pytest.raises(ValueError, match="integers"):
        fn(e, r, lengths=[2000.0, 1500, 300])
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="CPU integer tensor"):
            fn(e, r, lengths=torch.tensor(ok).cuda())
    # all value guards passed: the CPU tensors are refused before any launch
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        fn(e, r, lengths=ok)
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        fn(e[0], r[0], details=True)
    doc = INF.compute_sdr.__doc__
    assert "ESTIMATE FIRST" in doc and "bss_eval_sources" in doc and "arbitrary finite number" in doc


def test_score_list_knows_the_name():
    sig = [torch.zeros(400), torch.zeros(300)]
    assert "sdr" in INF.METRICS and '"sdr"' in INF.score_list.__doc__
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        INF.score_list(sig, sig, metrics=("sdr",))
    with pytest.raises(ValueError, match="metric 'pesq'"):
        INF.score_list(sig, sig, metrics=("sdr", "pesq"))


def test_sdr_ref_matches_mir_eval():
    """The pin for a machine that has the package: the reference restates bss_eval_sources for one source."""
    mir_eval = pytest.importorskip("mir_eval")
    for index, (L, K, kind) in enumerate(R.CASES):
        if K != 512:
            continue                                                         # the package's own filter length
        s, y = R.case_signals(index)
        want = mir_eval.separation.bss_eval_sources(s[None].astype(np.float64), y[None].astype(np.float64))[0][0]
        got = R.sdr(s, y, K)["sdr"]
        assert abs(got - want) < 1e-6, (L, got, want)
