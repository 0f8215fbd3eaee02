"""The streaming resampler (streaming.StreamingResampler / StreamingResamplerSessions) and the rate wrappers (AtRate,
SessionsAtRate) on the MI355X: bit identity with inference.resample however the signal is cut, the float64 restatement, both tap
forms, far positions, sessions against lock-step, and the wrappers against the offline-resampled composition."""
import importlib
import os
import random
import sys

import numpy as np
import pytest
import torch

from oracle import idccrn_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4          # the streaming-to-offline bar of tests/test_gpu_streaming.py
RATES = [(48000, 16000), (16000, 48000), (44100, 16000), (16000, 44100), (8000, 16000), (22050, 16000)]


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.streaming"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"),
            importlib.import_module("i-dccrn-vae_amd.inference"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _stream(st, x, sizes):
    outs, n = [], 0
    for m in sizes:
        outs.append(st.push(x[:, n:n + m]))
        n += m
    assert n == x.shape[1]
    outs.append(st.flush())
    return torch.cat(outs, dim=1)


def _signal(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, generator=g) * 0.1).cuda()


# ------------------------------------------------------------------------------------------------- 1. the lock-step resampler
@pytest.mark.parametrize("fs_in,fs_out", RATES)
def test_bit_identical_to_offline_however_cut(fs_in, fs_out):
    _, S, ops, _, I = _mods()
    up, down = ops.resample_ratio(fs_in, fs_out)
    H = ops.stream_resample_hist(up, down)
    h32 = ops.resample_taps(up, down, "cuda").double().cpu().numpy()
    rs = {B: S.StreamingResampler(fs_in, fs_out, B) for B in (1, 3)}
    assert rs[1].plan.H == H
    worst = 0.0
    for L in sorted({1, 2, H - 1, H, H + 1, 257, 2345}):
        x = _signal(3, L, L)
        want = I.resample(x, fs_in, fs_out)[0]
        # the float64 restatement with the kernel's own fp32 taps: what is left is the rounding of the result to fp32 (2^-24)
        ref = R.RefResampler(up, down, h32)
        for b in range(3):
            y64 = R.run(ref, x[b].double().cpu().numpy(), [L])[0]
            err = float(np.linalg.norm(want[b].double().cpu().numpy() - y64) / np.linalg.norm(y64))
            worst = max(worst, err)
            assert err < 1e-6, (L, b, err)
        for B in (1, 3):
            for name, sizes in R.chunkings(L, down, L).items():
                y = _stream(rs[B], x[:B], sizes)
                assert y.shape == (B, ops.resample_len(L, up, down)) and torch.equal(y, want[:B]), (L, B, name)
    print(f"{fs_in} -> {fs_out}: worst relative difference from the float64 restatement {worst:.2e}")


def test_against_float64_taps():
    """Against the restatement with scipy's float64 taps: the fp32 rounding of 2 half / up + 1 taps and of the result, 1e-6."""
    _, S, ops, _, _ = _mods()
    for fs_in, fs_out in RATES:
        up, down = ops.resample_ratio(fs_in, fs_out)
        x = _signal(2, 2345, 9)
        y = _stream(S.StreamingResampler(fs_in, fs_out, 2), x, [1000, 0, 1, 1344])
        for b in range(2):
            y64 = R.run(R.RefResampler(up, down), x[b].double().cpu().numpy(), [37] * 63 + [14])[0]
            err = float(np.linalg.norm(y[b].double().cpu().numpy() - y64) / np.linalg.norm(y64))
            print(f"{fs_in} -> {fs_out} row {b}: relative difference from float64 {err:.2e}")
            assert err < 1e-6


@pytest.mark.parametrize("fs_in,fs_out", [(48000, 16000), (16000, 44100), (44100, 16000)])
def test_tap_forms_pitched_inputs_and_reuse(fs_in, fs_out):
    _, S, ops, _, I = _mods()
    B, L = 3, 1500
    x = _signal(B, L, 21)
    want = I.resample(x, fs_in, fs_out)[0]
    sizes = [441, 0, 300, 1, 758]
    # the two instantiations give the same bits whichever the launcher would pick
    for mode in ("mem", "lds"):
        assert torch.equal(_stream(S.StreamingResampler(fs_in, fs_out, B, taps_mode=mode), x, sizes), want), mode
    rs = S.StreamingResampler(fs_in, fs_out, B)
    # a column slice of a wider buffer (pitched rows), a transposed view (no unit stride), float64 samples that are float32 values
    wide = torch.full((B, L + 64), float("nan"), device="cuda")
    wide[:, 32:32 + L] = x
    xt = x.t().contiguous().t()
    assert xt.stride(1) != 1
    for name, src in (("pitched", wide[:, 32:32 + L]), ("transposed", xt), ("float64", x.double())):
        assert torch.equal(_stream(rs, src, sizes), want), name
    # reuse after flush and after reset; an empty signal flushes to nothing
    assert torch.equal(_stream(rs, x, [L]), want)
    rs.push(x[:, :700])
    rs.reset()
    assert torch.equal(_stream(rs, x, [1] * 40 + [L - 40]), want)
    assert rs.flush().shape == (B, 0) and rs.push(x[:, :0]).shape == (B, 0) and rs.flush().shape == (B, 0)
    with pytest.raises(ValueError):
        rs.push(x[:2])
    with pytest.raises(RuntimeError):
        rs.push(x.cpu())
    assert rs.plan.n == 0 and torch.equal(_stream(rs, x, sizes), want)


@pytest.mark.parametrize("fs_in,fs_out,L,sizes", [(640, 1, 13000, [5000, 1, 7999]), (1, 640, 50, [1, 20, 0, 29])])
def test_largest_filter(fs_in, fs_out, L, sizes):
    """max(up, down) = 640: 12801 taps.  640 -> 1 Hz reads every tap per output (the LDS form, H = 12801), 1 -> 640 Hz 21 of them."""
    _, S, ops, _, I = _mods()
    x = _signal(2, L, 3)
    want = I.resample(x, fs_in, fs_out)[0]
    assert torch.equal(_stream(S.StreamingResampler(fs_in, fs_out, 2), x, sizes), want)
    other = "mem" if fs_out == 1 else "lds"
    assert torch.equal(_stream(S.StreamingResampler(fs_in, fs_out, 2, taps_mode=other), x, sizes), want)


@pytest.mark.parametrize("fs_in,fs_out", [(48000, 16000), (16000, 44100), (44100, 16000)])
def test_far_position_is_bit_identical(fs_in, fs_out):
    """A stream more than 2^33 samples in returns the bits of the same stream at its start: 64-bit positions, offsets from P0."""
    _, S, ops, _, _ = _mods()
    up, down = ops.resample_ratio(fs_in, fs_out)
    H = ops.stream_resample_hist(up, down)
    x = _signal(2, H + 7 + 500, 4)
    near, far = S.StreamingResampler(fs_in, fs_out, 2), S.StreamingResampler(fs_in, fs_out, 2)
    a0, b0 = near.push(x[:, :H + 7]), far.push(x[:, :H + 7])
    assert torch.equal(a0, b0)
    periods = 2 ** 33 // down + 1
    far._advance(periods)
    assert far.plan.n - near.plan.n == periods * down > 2 ** 33
    for lo, hi in ((H + 7, H + 8), (H + 8, H + 307), (H + 307, H + 507)):
        a, b = near.push(x[:, lo:hi]), far.push(x[:, lo:hi])
        assert a.shape == b.shape and torch.equal(a, b), (lo, hi)
    a, b = near.flush(), far.flush()
    assert a.shape[1] > 0 and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 2. sessions
def _session_schedule(seed, slots, width, lengths):
    """Calls (counts, end, drop-after) for ``slots`` slots: staggered starts, idle calls, counts 0 .. width, ends with the last
    samples or in a later call, ends of slots that have received nothing; -> (calls, signals [(slot, L, [(call, offset, n)])])."""
    rng = random.Random(seed)
    todo = {b: list(lengths[b]) for b in range(slots)}
    start = {b: b for b in range(slots)}
    cur, signals, calls, pending = {}, [], [], set()
    ci = 0
    while any(todo.values()) or cur or pending:
        counts, end = [0] * slots, sorted(pending)
        pending = set()
        for b in range(slots):
            if b in end:
                continue
            if b not in cur and todo[b] and ci >= start[b]:
                cur[b] = [len(signals), todo[b].pop(0), 0]
                signals.append((b, cur[b][1], []))
            if b not in cur:
                if rng.random() < 0.2:
                    end.append(b)
                continue
            idx, L, pos = cur[b]
            n = min(rng.choice([0, 1, 37, 160, width]), L - pos)
            counts[b] = n
            signals[idx][2].append((ci, pos, n))
            cur[b][2] = pos + n
            if pos + n == L:
                del cur[b]
                (end.append(b) if rng.random() < 0.5 else pending.add(b))
        calls.append((counts, sorted(end)))
        ci += 1
    return calls, signals


@pytest.mark.parametrize("fs_in,fs_out", [(44100, 16000), (16000, 44100), (48000, 16000)])
def test_sessions_equal_lockstep(fs_in, fs_out):
    _, S, ops, _, _ = _mods()
    slots, width = 5, 441
    up, down = ops.resample_ratio(fs_in, fs_out)
    calls, signals = _session_schedule(7, slots, width, {0: [2345, 61], 1: [1, 700], 2: [257], 3: [900, 2], 4: [1300]})
    sigs = [_signal(1, L, 100 + k)[0] for k, (_, L, _) in enumerate(signals)]
    rs = S.StreamingResamplerSessions(fs_in, fs_out, slots)
    lock = S.StreamingResampler(fs_in, fs_out, slots)
    # slot 2 first takes a signal that is dropped midway; the drop must leave nothing behind
    junk = torch.full((slots, width), float("nan"), device="cuda")
    junk[2, :300] = 1.0
    rs.push(junk, [0, 0, 300, 0, 0])
    assert rs.positions == [0, 0, 300, 0, 0]
    rs.drop([2])
    assert rs.positions == [0] * slots
    got = {k: [] for k in range(len(signals))}
    for ci, (counts, end) in enumerate(calls):
        x = torch.full((slots, width), float("nan"), device="cuda")      # whatever lies past counts[b] must not be read
        feeds = {}
        for k, (b, L, parts) in enumerate(signals):
            for c, pos, n in parts:
                if c == ci:
                    x[b, :n] = sigs[k][pos:pos + n]
                    feeds[b] = k
        before = rs.positions
        y, m = rs.push(x, counts, end)
        assert y.shape == (slots, max(m)) and not torch.isnan(y).any()
        for b in range(slots):
            assert not y[b, m[b]:].any(), (ci, b)                        # zeros behind m[b]
            assert rs.positions[b] == (0 if b in end else before[b] + counts[b])
            if b in feeds:
                got[feeds[b]].append(y[b, :m[b]].clone())
            elif m[b]:                                                   # an end in a later call than the last samples
                k = max(k for k, (sb, _, parts) in enumerate(signals) if sb == b and parts[-1][0] < ci)
                got[k].append(y[b, :m[b]].clone())
    assert rs.positions == [0] * slots
    for k, (b, L, _) in enumerate(signals):
        X = torch.zeros(slots, L, device="cuda")
        X[b] = sigs[k]
        want = _stream(lock, X, [L])[b]
        have = torch.cat(got[k])
        assert have.shape == want.shape and torch.equal(have, want), (k, b, L)
    # the guards: nothing changes
    rs.push(torch.zeros(slots, 50, device="cuda"), [50, 0, 0, 0, 7])
    pos = rs.positions
    for bad in (dict(counts=[51, 0, 0, 0, 0]), dict(counts=[1, 1]), dict(end=[5]), dict(counts=torch.tensor([1, 1, 1, 1, 1]).cuda())):
        with pytest.raises(ValueError):
            rs.push(torch.zeros(slots, 50, device="cuda"), **bad)
        assert rs.positions == pos
    y, m = rs.push(torch.zeros(slots, 0, device="cuda"), end=[1])       # ending a slot that has received nothing: a no-op
    assert y.shape == (slots, 0) and m == [0] * slots and rs.positions == pos


# ------------------------------------------------------------------------------------------------- 3. the wrappers
def _model(base, seed):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, SKIP, "mask", False, None, None)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k not in ("data_mean", "data_std")}, seed)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def _random_sizes(L, seed):
    rng = random.Random(seed)
    out, left = [], L
    while left:
        n = min(left, rng.choice([0, 0, 1, 13, 300, 441, 480, 1777]))
        out.append(n)
        left -= n
    return out


def _composition(I, st, x, fs):
    """The contract's right-hand side: offline resample -> whole-signal push + flush of the wrapped streamer -> offline resample."""
    x16 = I.resample(x, fs, 16000)[0]
    return I.resample(_stream(st, x16, [x16.shape[1]]), 16000, fs)[0]


@pytest.fixture(scope="module")
def dccrn():
    return _model(4, 11)


@pytest.mark.parametrize("fs", [48000, 44100])
def test_at_rate_dccrn(dccrn, fs):
    _, S, ops, _, I = _mods()
    B, L = 2, 7001
    x = _signal(B, L, fs)
    inner = S.StreamingDCCRN(dccrn, batch=B)
    want = _composition(I, inner, x, fs)
    st = S.AtRate(inner, fs)
    for name, sizes in (("whole", [L]), ("441", [441] * (L // 441) + [L % 441]), ("random", _random_sizes(L, 5))):
        y = _stream(st, x, sizes)
        assert y.shape == want.shape and torch.equal(y, want), name
    with torch.no_grad():
        off = I.resample(dccrn(I.resample(x, fs, 16000)[0], train=False)[0], 16000, fs)[0]
    print(f"AtRate({fs}) vs resample(model(resample(x))): {relerr(want, off):.3e}")
    assert want.shape == off.shape and relerr(want, off) < TOL


def test_at_rate_passthrough_and_short_signal(dccrn):
    _, S, ops, _, I = _mods()
    B = 2
    inner = S.StreamingDCCRN(dccrn, batch=B)
    x16 = _signal(B, 1234, 8)
    base = _stream(inner, x16, [1234])
    same = S.AtRate(inner, 16000)
    assert same.down is None and torch.equal(_stream(same, x16, [500, 734]), base)
    # a signal too short to end (0 < L16 <= n_fft/2) is refused before anything changes: more samples and the flush then give
    # the bits of the same signal streamed without the refused call
    fs = 48000
    x = _signal(B, 6000, 9)
    st = S.AtRate(inner, fs)
    want = _stream(st, x, [600, 5400])
    first = st.push(x[:, :600])                      # 200 samples at 16 kHz
    state = (st.down.plan.snapshot(), inner.plan.n, st.up.plan.snapshot())
    with pytest.raises(ValueError):
        st.flush()
    assert (st.down.plan.snapshot(), inner.plan.n, st.up.plan.snapshot()) == state
    assert torch.equal(torch.cat([first, st.push(x[:, 600:]), st.flush()], dim=1), want)
    assert torch.equal(_stream(st, x, [6000]), want)
    with pytest.raises(ValueError):
        st.flush()                                   # an empty signal, as the wrapped streamer refuses it


@pytest.mark.parametrize("fs", [44100, 48000])
def test_sessions_at_rate_equals_at_rate_per_slot(dccrn, fs):
    _, S, ops, _, I = _mods()
    slots, width = 3, 441
    lengths = {0: [7001], 1: [3000, 2500], 2: [5000]}
    calls, signals = _session_schedule(3, slots, width, lengths)
    sigs = [_signal(1, L, 200 + k)[0] for k, (_, L, _) in enumerate(signals)]
    st = S.SessionsAtRate(S.StreamingSessions(dccrn, slots), fs)
    lock = S.AtRate(S.StreamingDCCRN(dccrn, batch=slots), fs)
    got = {k: [] for k in range(len(signals))}
    for ci, (counts, end) in enumerate(calls):
        x = torch.full((slots, width), float("nan"), device="cuda")
        feeds = {}
        for k, (b, L, parts) in enumerate(signals):
            for c, pos, n in parts:
                if c == ci:
                    x[b, :n] = sigs[k][pos:pos + n]
                    feeds[b] = k
        y, m = st.push(x, counts, end)
        assert y.shape == (slots, max(m)) and not torch.isnan(y).any()
        for b in range(slots):
            assert not y[b, m[b]:].any()
            k = feeds.get(b)
            if k is None and m[b]:
                k = max(k for k, (sb, _, parts) in enumerate(signals) if sb == b and parts[-1][0] < ci)
            if k is not None:
                got[k].append(y[b, :m[b]].clone())
    assert st.positions == [0] * slots
    for k, (b, L, _) in enumerate(signals):
        X = torch.zeros(slots, L, device="cuda")
        X[b] = sigs[k]
        want = _stream(lock, X, [L])[b]
        have = torch.cat(got[k])
        assert have.shape == want.shape and torch.equal(have, want), (k, b, L)
    # the short-signal refusal of the wrapped sessions, before anything changes; the slot then goes on to the same bits
    x = torch.zeros(slots, width, device="cuda")
    x[1] = sigs[1][:width]
    y, m = st.push(x, [0, width, 0])
    outs = [y[1, :m[1]].clone()]
    pos = (st.positions, st.sessions.positions, st.up.positions)
    with pytest.raises(ValueError):
        st.push(x, [0, 100, 0], end=[1])
    assert (st.positions, st.sessions.positions, st.up.positions) == pos
    for lo in range(width, 3000, width):
        n = min(width, 3000 - lo)
        x[1, :n] = sigs[1][lo:lo + n]
        y, m = st.push(x, [0, n, 0], end=[1] if lo + n == 3000 else [])
        outs.append(y[1, :m[1]].clone())
    assert torch.equal(torch.cat(outs), torch.cat(got[1]))
    st.drop([0, 1, 2])
    assert st.positions == [0] * slots


def test_at_rate_vae():
    pm, S, ops, _, I = _mods()
    zdim, ns, B, L, fs = 16, 2, 2, 7001, 44100
    np_ = O.net_params(True, 4)
    enc = pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2)
    dec = pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP, False)
    for mod, seed in ((enc, 42), (dec, 43)):
        mod.load_state_dict(O.synth_state_dict({k: tuple(v.shape) for k, v in mod.state_dict().items()}, seed), strict=True)
        mod.cuda()
    x = _signal(B, L, 6)
    inner = S.StreamingVAE(enc, dec, batch=B, seed=3)
    want = _composition(I, inner, x, fs)
    st = S.AtRate(inner, fs)
    for name, sizes in (("441", [441] * (L // 441) + [L % 441]), ("random", _random_sizes(L, 9))):
        y = _stream(st, x, sizes)
        assert y.shape == want.shape and torch.equal(y, want), name
    with pytest.raises(ValueError):
        S.AtRate(S.StreamingVAE(enc, dec, batch=B, average=False), fs)
