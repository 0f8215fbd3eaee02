"""CPU tests of the STOI / ESTOI / RMSE scoring family: the additive C ABI, the host reference tests/stoi_ref.py (its tables and
its behaviour -- it is the yardstick of tests/test_gpu_stoi.py) and the host-side guards of inference.compute_stoi / compute_estoi /
compute_rmse / score_list; no GPU needed."""
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

INF = importlib.import_module("i-dccrn-vae_amd.inference")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_stoi", "idv_stoi_work_bytes", "idv_rmse_ragged"):
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_stoi_work_bytes"] == ("long long", ["int", "int", "int"])
    assert protos["idv_stoi"] == ("int", ["ptr", "long long", "ptr", "long long", "ptr", "int", "int", "int", "int", "ptr", "long long",
                                          "ptr", "ptr", "ptr"])
    assert protos["idv_rmse_ragged"] == ("int", ["ptr", "long long", "ptr", "long long", "ptr", "int", "ptr", "ptr", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries
    # the size query needs no device: sized for the no-frame-dropped case, monotone, and refusing what idv_stoi refuses
    wb = lib.idv_stoi_work_bytes
    assert wb(1, 16000, 16000) > 2 * 10000 * 4 and wb(4, 16000, 16000) > 3 * wb(1, 16000, 16000)
    assert 0 < wb(1, 10000, 10000) < wb(1, 16000, 16000) < wb(1, 160000, 16000)
    assert wb(1, 16000, 8000) == -1 and wb(0, 16000, 16000) == -1 and wb(1, 0, 16000) == -1


def test_reference_tables():
    h = R.fir_taps()
    assert h.shape == (581,) and abs(h.sum() - 1.0) < 1e-14 and np.array_equal(h, h[::-1])
    assert R.band_edges() == (R.BAND_LO, R.BAND_HI)
    assert R.BAND_LO[1:] == R.BAND_HI[:-1] and R.BAND_LO[0] == 7 and R.BAND_HI[-1] == 219
    w = R.window()
    assert w.shape == (256,) and w[0] > 0 and not np.allclose(w, torch.hann_window(256, dtype=torch.float64).numpy())
    assert np.abs(w[:128] + w[128:] - 1).max() > 1e-3                        # overlap-add of the kept frames is not a copy
    x = np.random.default_rng(0).standard_normal(1000)
    got, want = R.resample_written_out(x), R.resample(x)
    assert got.shape == want.shape == (625,)
    assert np.abs(got - want).max() < 1e-12
    assert R.resample(np.zeros(8601)).shape == (5376,) and 5376 == 256 + 128 * 40


def test_reference_counts_of_the_shared_cases():
    """The counts the GPU test relies on; the margins keep an fp32 energy from flipping a frame."""
    want = {"compaction": (77, 37, 7), "near_30": (59, 33, 3), "too_few": (52, 26, 0), "range_edge": (40, 40, 10),
            "range_next": (41, 41, 11), "longer": (116, 59, 29), "one_segment": (57, 31, 1), "many_blocks": (282, 135, 105)}
    for name, gen, n in R.CASES:
        x = gen(n)
        score, counts, margin = R.stoi(x, R.noisy(x, 0), 16000, True)
        assert counts == want[name], (name, counts)
        assert margin >= 0.5, (name, margin)
        if name == "too_few":
            assert score == 1e-5


@pytest.mark.parametrize("extended", [False, True])
def test_reference_behaviour(extended):
    x = R.speech(16000)
    s, counts, _ = R.stoi(x, x, 16000, extended)
    assert abs(s - 1.0) < 1e-12 and counts == (77, 37, 7)
    s10, _, _ = R.stoi(R.resample(x), R.resample(x), 10000, extended)
    assert abs(s10 - 1.0) < 1e-12
    z = np.zeros(16000)
    for a, b in ((x, z), (z, x), (z, z)):                                     # (reference, estimate)
        s, _, _ = R.stoi(a, b, 16000, extended)
        assert s == 0.0 and np.isfinite(s)
    with pytest.raises(ValueError):
        R.stoi(x, x, 8000, extended)


def test_reference_estoi_falls_with_the_snr():
    x = R.speech(24000)
    scores = [R.stoi(x, R.noisy(x, snr), 16000, True)[0] for snr in (20, 5, 0, -5)]
    assert all(a > b for a, b in zip(scores, scores[1:])), scores
    assert 0 < scores[-1] and scores[0] < 1


def test_reference_float32_floor_is_small():
    """The float32 restatement stands within 1e-5 of the yardstick (the GPU test takes 4x its largest deviation as its bound)."""
    x = R.speech(16000)
    y = R.noisy(x, 0)
    for ext in (False, True):
        a, ca, _ = R.stoi(x, y, 16000, ext)
        b, cb, _ = R.stoi(x, y, 16000, ext, dtype=np.float32)
        assert ca == cb and abs(a - b) < 1e-5


def test_guards_raise_before_gpu_work():
    e, r = torch.zeros(3, 2000), torch.zeros(3, 2000)
    ok = [2000, 1500, 300]
    for fn in (INF.compute_stoi, INF.compute_estoi):
        for fs in (8000, 44100, 16000.5, True):
            with pytest.raises(ValueError, match="fs"):
                fn(e, r, fs=fs)
    for fn in (INF.compute_stoi, INF.compute_estoi, INF.compute_rmse):
        with pytest.raises(ValueError, match="batch size"):
            fn(e, r[:2], lengths=ok)
        with pytest.raises(ValueError, match="differ"):
            fn(e, r[:, :1999])
        with pytest.raises(ValueError, match="2 lengths for a batch of 3"):
            fn(e, r, lengths=ok[:2])
        with pytest.raises(ValueError, match="exceeds"):
            fn(e, r, lengths=[2001, 1500, 300])
        with pytest.raises(ValueError, match="exceeds"):
            fn(e, r[:, :1999], lengths=ok)                                   # beyond the shorter row
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
            fn(e[0], r[0])
    sig = [torch.zeros(400), torch.zeros(300)]
    with pytest.raises(ValueError, match="metric 'pesq'"):
        INF.score_list(sig, sig, metrics=("sisdr", "pesq"))
    with pytest.raises(ValueError, match="fs"):
        INF.score_list(sig, sig, fs=8000)
    with pytest.raises(ValueError, match="2 estimates for 1 references"):
        INF.score_list(sig, sig[:1])
    with pytest.raises(ValueError, match="max_batch"):
        INF.score_list(sig, sig, max_batch=0)
    with pytest.raises(ValueError, match="1-D"):
        INF.score_list([torch.zeros(2, 300)], [torch.zeros(300)])
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        INF.score_list(sig, sig)
    assert INF.compute_estoi.__doc__ and "ESTIMATE FIRST" in INF.compute_stoi.__doc__ and "clean, processed" in INF.compute_stoi.__doc__


def test_stoi_ref_matches_pystoi():
    """The pin for a machine that has the package: the reference restates pystoi.stoi(clean, processed, fs, extended)."""
    pystoi = pytest.importorskip("pystoi")
    for name, gen, n in R.CASES:
        x = gen(n)
        for snr in R.SNRS:
            y = R.noisy(x, snr)
            for ext in (False, True):
                want = pystoi.stoi(x, y, 16000, extended=ext)
                got = R.stoi(x, y, 16000, ext)[0]
                assert abs(got - want) < 1e-9, (name, snr, ext, got, want)
