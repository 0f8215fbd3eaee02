"""CPU tests of the streaming bookkeeping (streaming.StreamPlan) and of StreamingDCCRN's guards; no GPU needed."""
import importlib
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S = importlib.import_module("i-dccrn-vae_amd.streaming")
PM = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
from oracle import idccrn_oracle as O  # noqa: E402

N_FFT, HOP, WIN = 512, 100, 400


def _chunkings(L):
    rng = random.Random(L)
    out = {"whole": [L], "37": [37] * (L // 37) + [L % 37], "100": [100] * (L // 100) + [L % 100],
           "160": [160] * (L // 160) + [L % 160]}
    if L <= 2345:
        out["1"] = [1] * L
    rnd, left = [], L
    while left:
        n = min(left, rng.choice([0, 0, 1, 7, 50, 99, 100, 101, 333, 1000]))
        rnd.append(n)
        left -= n
    out["random"] = rnd
    return out


def _k(n):
    return 0 if n <= WIN // 2 else (n - WIN // 2) // HOP + 1


@pytest.mark.parametrize("L", [257, 300, 401, 2345, 64000])
def test_plan_counts_follow_the_contract(L):
    for name, sizes in _chunkings(L).items():
        pl = S.StreamPlan(N_FFT, HOP, WIN, cap=64)
        n = got = 0
        for m in sizes:
            chunks = pl.push(m)
            n += m
            got += sum(c.e1 - c.e0 for c in chunks)
            assert pl.k == _k(n), (name, n)
            assert got == max(0, HOP * _k(n) - WIN // 2), (name, n)
            assert all(0 < c.k <= 64 for c in chunks)
            if m == 0 or _k(n) == _k(n - m):
                assert chunks == []
        chunks = pl.flush()
        got += sum(c.e1 - c.e0 for c in chunks)
        assert got == HOP * (L // HOP), name
        assert pl.k == torch.stft(torch.zeros(1, L), N_FFT, HOP, WIN, torch.hann_window(WIN), return_complex=True).shape[-1]


def _emulate(x, sizes):
    """float64 replay of the schedule with an identity network: framing with the ring / mirrors, windowed overlap-add, carry,
    envelope and emission exactly as the chunk ranges of StreamPlan say."""
    B, L = x.shape
    w = torch.hann_window(WIN, periodic=True, dtype=torch.float64)
    half, left = N_FFT // 2, (N_FFT - WIN) // 2
    pl = S.StreamPlan(N_FFT, HOP, WIN, cap=5)
    carry = torch.zeros(B, pl.carry_cap, dtype=torch.float64)
    outs = []

    def run(chunks, n_avail, L_end):
        nonlocal carry
        for c in chunks:
            P = torch.arange(half + c.e0, c.p_end)
            v = torch.zeros(B, len(P), dtype=torch.float64)
            v[:, :c.carry_in] = carry[:, :c.carry_in]
            for t in range(c.t0, c.t0 + c.k):
                s = HOP * t + left - half + torch.arange(WIN)
                s = torch.where(s < 0, -s, s)
                if L_end is not None:
                    s = torch.where(s >= L_end, 2 * (L_end - 1) - s, s)
                assert int(s.max()) < n_avail
                fr = x[:, s] * w
                i = P - HOP * t - left
                ok = (i >= 0) & (i < WIN)
                v[:, ok] += fr[:, i[ok]] * w[i[ok]]
            T = pl.total_frames(L_end) if L_end is not None else 10 ** 9
            env = torch.zeros(len(P), dtype=torch.float64)
            for t in range(0, min(T, int(P.max()) // HOP + 1)):
                i = P - HOP * t - left
                ok = (i >= 0) & (i < WIN)
                env[ok] += w[i[ok]] ** 2
            ne = c.e1 - c.e0
            outs.append(v[:, :ne] / env[:ne])
            carry = torch.zeros_like(carry)
            carry[:, :c.carry_out] = v[:, ne:]

    n = 0
    for m in sizes:
        run(pl.push(m), n + m, None)
        n += m
    run(pl.flush(), n, n)
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("L", [257, 300, 401, 1600, 2345])
def test_plan_ranges_reproduce_stft_istft(L):
    g = torch.Generator().manual_seed(L)
    x = torch.randn(2, L, generator=g, dtype=torch.float64)
    w = torch.hann_window(WIN, periodic=True, dtype=torch.float64)
    ref = torch.istft(torch.stft(x, N_FFT, HOP, WIN, w, return_complex=True), N_FFT, HOP, WIN, w)
    for name, sizes in _chunkings(L).items():
        if name == "1" and L > 401:
            continue
        y = _emulate(x, sizes)
        assert y.shape == ref.shape, name
        assert float((y - ref).abs().max()) < 1e-9, name


def _cpu_model(causal=True, recon="mask"):
    np_ = O.net_params(causal, 4)
    return PM.DCCRN_(N_FFT, HOP, np_, causal, "cpu", WIN, [0, 1, 2, 3, 4, 5], recon, False, None, None)


def test_guards_raise_before_gpu_work():
    with pytest.raises(ValueError, match="causal"):
        S.check_model(_cpu_model(causal=False), 2)
    with pytest.raises(ValueError, match="recon_type"):
        S.check_model(_cpu_model(recon="polar"), 2)
    with pytest.raises(ValueError, match="batch"):
        S.check_model(_cpu_model(), 0)
    with pytest.raises(RuntimeError, match="GPU"):
        S.check_model(_cpu_model(), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        S.StreamingDCCRN(_cpu_model(), 2)
    with pytest.raises(ValueError, match="causal"):
        S.StreamingDCCRN(_cpu_model(causal=False), 2)
    with pytest.raises(ValueError, match="streams"):
        S.check_input(torch.zeros(3, 10), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        S.check_input(torch.zeros(2, 10), 2)
    pl = S.StreamPlan(N_FFT, HOP, WIN)
    pl.push(N_FFT // 2)
    with pytest.raises(ValueError, match="n_fft/2"):
        pl.flush()
    pl = S.StreamPlan(N_FFT, HOP, WIN)
    pl.push(N_FFT // 2 + 1)
    assert sum(c.e1 - c.e0 for c in pl.flush()) == HOP * ((N_FFT // 2 + 1) // HOP)
