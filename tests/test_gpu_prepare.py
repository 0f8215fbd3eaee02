"""Corpus preparation on the MI355X: the rational polyphase resampler (csrc/resample.hip through inference.resample / resample_list),
the zero-pad STFT framing (csrc/ragged.hip) and the STFT moment tables (csrc/moments.hip through dataset.stats) against the float64
host definitions of tests/prepare_ref.py.  Signals of at most 16000 samples; the references are computed once per module."""
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

import prepare_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NFFT, WIN, HOP = R.NFFT, R.WIN, R.HOP
SKIP = [0, 1, 2, 3, 4, 5]
OP_TOL = 2e-5         # an fp32 operator: the bound tests/test_gpu_ragged.py uses for the mirrored framing's STFT / ISTFT

# (up, down) -> (fs_in, fs_out)
RATES = {(1, 3): (48000, 16000), (160, 441): (44100, 16000), (441, 160): (16000, 44100), (2, 1): (8000, 16000), (1, 2): (32000, 16000)}
MOMENT_LENS = {"reflect": [257, 300, 1999, 6400, 16000], "constant": [257, 300, 1999, 6400, 16000, 100, 37]}


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.inference"), importlib.import_module("i-dccrn-vae_amd.ops"),
            importlib.import_module("i-dccrn-vae_amd.dataset.stats"))


def _lens_for(up, down):
    """1, 2, 3, 767, 768, 769 and 6000, and the two lengths whose output counts straddle the 256-output workgroup boundary."""
    at = 256 * down // up                                   # the longest input with at most 256 outputs
    assert R.n_out(at, up, down) <= 256 < R.n_out(at + 1, up, down)
    return sorted({1, 2, 3, 767, 768, 769, 6000, at, at + 1})


def _padded(rows, fill=float("nan"), extra=0):
    x = torch.full((len(rows), max(len(r) for r in rows) + extra), fill)
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(np.asarray(r, dtype=np.float32))
    return x.cuda()


@pytest.fixture(scope="module")
def rs_ref():
    """Per ratio: the float32 rows (what the device sees) and scipy's resample_poly of them in float64 and in float32."""
    table = {}
    for k, (up, down) in enumerate(RATES):
        rng = np.random.default_rng(100 + k)
        rows = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in _lens_for(up, down)]
        table[(up, down)] = (rows, [R.resample(r, up, down) for r in rows], [R.resample(r, up, down, np.float32) for r in rows])
    return table


@pytest.mark.parametrize("up,down", list(RATES))
def test_resampler_values_within_four_float32_floors(rs_ref, up, down):
    """One NaN-padded batch of all the lengths against scipy.signal.resample_poly in float64 on the same float32 samples:
    |device - float64| <= 4 x the largest |scipy in float32 - scipy in float64| of the case (the factor covers another summation
    order and nothing more); the output lengths are ceil(L up / down) and the columns behind them exactly zero.

    Measured on the MI355X, float32 floor / device worst: 1/3 4.5e-8 / 1.3e-8, 160/441 5.2e-8 / 1.1e-8, 441/160
    8.3e-8 / 2.5e-8, 2/1 5.9e-8 / 2.0e-8, 1/2 4.2e-8 / 1.6e-8: the double accumulator leaves the rounding of the float32 output
    (half an ulp of 0.4 is 1.5e-8) and of the float32 taps."""
    inf, _, _ = _mods()
    rows, want, f32 = rs_ref[(up, down)]
    fs_in, fs_out = RATES[(up, down)]
    lens = [len(r) for r in rows]
    y, out_lens = inf.resample(_padded(rows), fs_in, fs_out, lengths=lens)
    assert y.dtype == torch.float32 and y.shape == (len(rows), R.n_out(max(lens), up, down))
    assert out_lens == [R.n_out(n, up, down) for n in lens] == [len(w) for w in want]
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    floor = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(f32, want))
    worst = max(np.abs(y[b, :n].astype(np.float64) - want[b]).max() for b, n in enumerate(out_lens))
    print(f"resample {up}/{down}: float32 floor {floor:.3e} bound {4 * floor:.3e} device worst {worst:.3e}")
    assert 0 < floor < 1e-6
    assert worst <= 4 * floor
    for b, n in enumerate(out_lens):
        assert not y[b, n:].any(), (b, n)
        assert np.abs(y[b, :n]).max() > 0


@pytest.mark.parametrize("up,down", list(RATES))
def test_resampler_rows_are_independent(rs_ref, up, down):
    """NaN at and past every row's end, and a wider row pitch: each row is bit-identical to that row resampled alone at B = 1."""
    inf, _, _ = _mods()
    rows = rs_ref[(up, down)][0]
    fs_in, fs_out = RATES[(up, down)]
    lens = [len(r) for r in rows]
    y, out_lens = inf.resample(_padded(rows), fs_in, fs_out, lengths=torch.tensor(lens))
    wide = _padded(rows, extra=77)[:, :max(lens)]                            # a column slice: row pitch Lmax + 77
    y2, _ = inf.resample(wide, fs_in, fs_out, lengths=lens)
    assert torch.isfinite(y).all() and torch.equal(y, y2)
    for b, r in enumerate(rows):
        alone, n1 = inf.resample(torch.from_numpy(r).cuda(), fs_in, fs_out)
        assert alone.shape == (out_lens[b],) and n1 == [out_lens[b]]
        assert torch.equal(y[b, :out_lens[b]].view(torch.int32), alone.view(torch.int32)), (b, lens[b])
    full, _ = inf.resample(_padded(rows[-1:]), fs_in, fs_out)                # no lengths: every row is full
    assert torch.equal(full[0], y[lens.index(max(lens)), :out_lens[lens.index(max(lens))]])


def test_resampler_long_decimation_reads_memory_directly():
    """up = 1, down = 12: the input span of 256 outputs no longer fits the staged LDS segment, so the kernel form that reads the
    samples from memory runs; same definition, same bound, rows independent."""
    inf, _, _ = _mods()
    rng = np.random.default_rng(7)
    rows = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (5000, 3073, 12)]
    lens = [len(r) for r in rows]
    y, out_lens = inf.resample(_padded(rows), 16000 * 12, 16000, lengths=lens)
    y = y.cpu()
    worst = floor = 0.0
    for b, r in enumerate(rows):
        want = R.resample(r, 1, 12)
        floor = max(floor, np.abs(R.resample(r, 1, 12, np.float32).astype(np.float64) - want).max())
        worst = max(worst, np.abs(y[b, :out_lens[b]].numpy().astype(np.float64) - want).max())
        assert not y[b, out_lens[b]:].any()
        alone, _ = inf.resample(torch.from_numpy(r).cuda(), 16000 * 12, 16000)
        assert torch.equal(alone.cpu(), y[b, :out_lens[b]])
    print(f"resample 1/12: float32 floor {floor:.3e} device worst {worst:.3e}")
    assert worst <= 4 * floor


def test_resample_list(rs_ref):
    """Mixed rates per signal, shuffled lengths, batches of three: the caller's order comes back, every result equals the per-signal
    call bit for bit, and a signal already at the target rate comes back as the same tensor."""
    inf, _, _ = _mods()
    rates, sigs = [], []
    for (up, down), fs in ((1, 3), 48000), ((160, 441), 44100), ((1, 2), 32000):
        for r in rs_ref[(up, down)][0][::2]:
            rates.append(fs)
            sigs.append(torch.from_numpy(r).cuda())
    same = torch.from_numpy(rs_ref[(2, 1)][0][-1]).cuda()
    rates.insert(3, 16000)
    sigs.insert(3, same)
    order = np.random.default_rng(1).permutation(len(sigs)).tolist()
    rates, sigs = [rates[k] for k in order], [sigs[k] for k in order]
    got = inf.resample_list(sigs, rates, 16000, max_batch=3)
    assert len(got) == len(sigs)
    for k, (s, fs) in enumerate(zip(sigs, rates)):
        if fs == 16000:
            assert got[k] is s
            continue
        alone, _ = inf.resample(s, fs, 16000)
        assert got[k].shape == alone.shape and torch.equal(got[k].view(torch.int32), alone.view(torch.int32)), (k, fs)
    one = inf.resample_list(sigs[:2], 48000)                                 # one rate for all, default target
    assert [int(v.shape[0]) for v in one] == [R.n_out(int(s.shape[0]), 1, 3) for s in sigs[:2]]
    assert inf.resample(same, 16000)[0] is same and inf.resample(same, 16000, 16000)[1] == [int(same.shape[0])]


def test_taps_are_formed_once_per_ratio_and_device():
    inf, ops, _ = _mods()
    x = torch.zeros(1, 1000, device="cuda")
    inf.resample(x, 22050, 16000)
    t0 = ops.resample_taps(320, 441, x.device)
    inf.resample(x, 22050, 16000)
    assert ops.resample_taps(320, 441, "cuda") is t0 and t0.dtype == torch.float32 and t0.shape == (8821,)
    assert np.array_equal(t0.cpu().numpy(), R.taps(320, 441).astype(np.float32))


# ------------------------------------------------------------------------------------------------ framing
def _spectrum(ops, x, lens_obj, T, fwd, pad_mode):
    fr = ops.stft_frames_pad(x, lens_obj, NFFT, WIN, HOP, T, pad_mode)
    out = ops.Planar.empty(1, NFFT // 2 + 1, x.shape[0], T, T + 1, x.device)
    ops.pw_gemm(fr.ptr(), WIN, fwd[0], fwd[1], 2 * (NFFT // 2 + 1), x.shape[0], T + 1, fr.Jp, T, out.ptr())
    return fr, out


def test_zero_pad_framing_and_the_untouched_mirror():
    """"constant" mode: the frames are exact copies of the zero-padded signal (NaN past every row's end is never read), frames past a
    row's end and the guard column are zeros, and the STFT of the ragged batch equals prepare_ref.spec within the fp32 operator bound
    of tests/test_gpu_ragged.py.  "reflect" mode through the new entry gives the bits of idv_stft_frames_ragged and of
    ops.stft(lengths=...)."""
    _, ops, _ = _mods()
    lens = MOMENT_LENS["constant"]
    rows = [R.dc_signal(n, 40 + k) for k, n in enumerate(lens)]
    x = _padded(rows)
    T = 1 + max(lens) // HOP
    plan = ops.DftPlan(NFFT, WIN, HOP, T, x.device)
    L = ops.Lengths(lens, x.device)
    fr, spec = _spectrum(ops, x, L, T, plan.fwd, "constant")
    frames = fr.planes().reshape(WIN, len(lens), T + 1).cpu().numpy()
    S = spec.tensor4().cpu().numpy()                                         # [B, F, T, 2]
    assert np.isfinite(frames).all() and np.isfinite(S).all()
    left = (NFFT - WIN) // 2
    for b, r in enumerate(rows):
        Tb = 1 + lens[b] // HOP
        want = R.frames(r, "constant")[:, left:left + WIN]                   # [Tb, win]
        assert np.array_equal(frames[:, b, 1:1 + Tb], want.T), (b, lens[b])
        assert not frames[:, b, 0].any() and not frames[:, b, 1 + Tb:].any()
        ref = R.spec(r, "constant").transpose(1, 0, 2)                       # [F, Tb, 2]
        err = np.linalg.norm(S[b, :, :Tb] - ref) / np.linalg.norm(ref)
        print(f"constant-mode STFT row {b} len {lens[b]}: relerr {err:.3e}")
        assert err < OP_TOL
        assert not S[b, :, Tb:].any()
    # the mirror: the new entry in "reflect" mode, the existing entry and ops.stft(lengths=...) give the same bits
    lens_r = MOMENT_LENS["reflect"]
    xr = _padded(rows[:len(lens_r)])
    Lr = ops.Lengths(lens_r, xr.device)
    fr_new, spec_new = _spectrum(ops, xr, Lr, T, plan.fwd, "reflect")
    old = ops.stft(xr, plan, lengths=Lr)
    assert torch.equal(spec_new.planes().contiguous().view(torch.int32), old.planes().contiguous().view(torch.int32))
    fr_old = ops.Planar.empty(1, WIN // 2, len(lens_r), T, T + 1, xr.device)
    ops.call("idv_stft_frames_ragged", ops.p(xr), ops.ll(xr.stride(0)), ops.p(Lr.dev), ops.i(len(lens_r)), ops.i(NFFT), ops.i(WIN),
             ops.i(HOP), ops.i(T), fr_old.ptr(), ops.i(T + 1), ops.i(fr_old.Jp), ops.stream_ptr())
    assert torch.equal(fr_new.planes().contiguous().view(torch.int32), fr_old.planes().contiguous().view(torch.int32))
    assert not torch.equal(fr_new.planes()[..., 1], fr.planes()[:, :, :, :len(lens_r), 1])       # frame 0: mirrored, not zero-padded
    ref =R.spec(rows[2], "reflect").transpose(1, 0, 2)
    got = old.tensor4()[2, :, :ref.shape[1]].cpu().numpy()
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < OP_TOL


# ------------------------------------------------------------------------------------------------ moments
@pytest.fixture(scope="module")
def mo_ref():
    """Per pad mode: the float32 signals, the float64 moments and the float32-spectrum moments (the floor's yardstick)."""
    table = {}
    for mode, lens in MOMENT_LENS.items():
        sig = [R.dc_signal(n, 10 + k) for k, n in enumerate(lens)]
        table[mode] = (sig, R.moments(sig, mode), R.moments(sig, mode, dtype=np.float32))
    return table


def _acc(mode):
    _, _, stats = _mods()
    return stats.SpecMoments(NFFT, WIN, HOP, "cuda", mode)


@pytest.mark.parametrize("mode", ["constant", "reflect"])
def test_moments_values_within_four_float32_floors(mo_ref, mode):
    """One NaN-padded batch of 0.05 N(0, 1) + 0.5 signals (mean of bin 0 about 100, std below 1 away from the signal ends) against
    np.mean / np.std(ddof=1) over the float64 spectrum: |device - float64| <= 4 x the largest error of the same definition with a
    float32 spectrum and float64 moments, separately for the mean and the std table; count = sum(1 + L // hop) exactly.  A one-pass
    float32 sum / sum of squares is off by 1.9e-4 / 1.8e-3 on these inputs.

    Measured on the MI355X, float32 floor / device worst: "constant" mean 9.7e-7 / 1.8e-6, std 8.4e-7 / 7.5e-7;
    "reflect" mean 1.1e-6 / 2.2e-6, std 7.8e-7 / 1.3e-6.  The moments themselves are exact to 1e-15 (the cuts test); what is left
    is the fp32 matrix-core DFT: 400-term fp32 sums near 100 (ulp 7.6e-6) in another order than numpy's float32 product."""
    sig, (mean, std, n), (m32, s32, _) = mo_ref[mode]
    lens = [len(s) for s in sig]
    acc = _acc(mode).update(_padded(sig), lens)
    assert acc.count == n == sum(1 + v // HOP for v in lens)
    gm, gs = acc.result()
    assert gm.shape == gs.shape == (NFFT // 2 + 1, 2) and gm.dtype == gs.dtype == np.float64
    assert np.isfinite(gm).all() and np.isfinite(gs).all()
    fm, fs_ = np.abs(m32 - mean).max(), np.abs(s32 - std).max()
    em, es = np.abs(gm - mean).max(), np.abs(gs - std).max()
    print(f"moments {mode}: largest mean {np.abs(mean).max():.2f}; float32 floor mean {fm:.3e} std {fs_:.3e}; device mean {em:.3e} std {es:.3e}")
    assert 0 < fm < 1e-5 and 0 < fs_ < 1e-5 and np.abs(mean).max() > 50
    assert em <= 4 * fm
    assert es <= 4 * fs_
    # the imaginary parts of bins 0 and n_fft/2 are 0 in the reference, std included: absolute terms
    for k in (0, NFFT // 2):
        assert std[k, 1] == 0 and mean[k, 1] == 0
        assert abs(gm[k, 1]) <= 4 * fm and gs[k, 1] <= 4 * fs_


@pytest.mark.parametrize("mode", ["constant", "reflect"])
def test_moments_do_not_depend_on_the_cuts(mo_ref, mode):
    """The same signals in one update, in three updates of other batches, and in two accumulators merged: the spectra are the same
    floats and only the order of the double additions differs, so the tables agree within 1e-10 of their largest entry; the same
    sequence of calls run twice gives the same bits."""
    sig = mo_ref[mode][0]
    lens = [len(s) for s in sig]

    def one():
        return _acc(mode).update(_padded(sig), lens)

    def three():
        acc = _acc(mode)
        for part in (sig[:2], sig[2:3], sig[3:]):
            acc.update(_padded(part, fill=0.0, extra=5), [len(s) for s in part])
        return acc

    def merged():
        a, b = _acc(mode), _acc(mode)
        a.update(_padded(sig[1::2]), lens[1::2])
        b.update(_padded(sig[0::2]), lens[0::2])
        return a.merge(b).merge(_acc(mode))                                  # an empty one changes nothing

    res = [f().result() for f in (one, three, merged)]
    assert one().count == three().count == merged().count
    scale = max(np.abs(res[0][0]).max(), np.abs(res[0][1]).max())
    for k in (1, 2):
        dm, ds = np.abs(res[k][0] - res[0][0]).max(), np.abs(res[k][1] - res[0][1]).max()
        print(f"moments {mode} cut {k}: mean {dm:.3e} std {ds:.3e} (scale {scale:.1f})")
        assert dm <= 1e-10 * scale and ds <= 1e-10 * scale
    for f, first in zip((one, three, merged), res):
        again = f().result()
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


def test_moments_span_several_tiles_and_single_rows(mo_ref):
    """Rows of 161 frames, 30 of them: 4860 columns are three 2048-column tiles, with rows that straddle the tile edges; and an
    update of one 1-D signal.  Against the float64 reference within the four floors of its float32 form."""
    sig = [mo_ref["constant"][0][4]] * 30 + [mo_ref["constant"][0][6]]
    mean, std, n = R.moments(sig, "constant")
    m32, s32, _ = R.moments(sig, "constant", dtype=np.float32)
    acc = _acc("constant").update(_padded(sig[:30]), [len(s) for s in sig[:30]])
    acc.update(torch.from_numpy(sig[30]).cuda())
    assert acc.count == n == 30 * 161 + 1
    gm, gs = acc.result()
    assert np.abs(gm - mean).max() <= 4 * np.abs(m32 - mean).max() and np.abs(gs - std).max() <= 4 * np.abs(s32 - std).max()


def test_cal_mean_std_end_to_end(tmp_path):
    """A list that mixes 16 kHz tensors, (tensor, 48000) pairs and a 48 kHz wav file equals the host definition, resample followed
    by moments, within the same four floors; the saved tables load back, and their buffers() reshape builds a mini DCCRN_ with
    --data_norm that gives a finite eval forward."""
    import scipy.io.wavfile as wavfile
    from oracle import idccrn_oracle as O
    _, _, stats = _mods()
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    at16 = [R.dc_signal(n, 60 + k) for k, n in enumerate((1999, 6400, 300))]
    at48 = [R.dc_signal(n, 70 + k) for k, n in enumerate((6000, 9001))]
    pcm = np.round(R.dc_signal(4803, 80) * 32768.0).astype(np.int16)
    wavfile.write(str(tmp_path / "c.wav"), 48000, pcm)
    items = [torch.from_numpy(at16[0]).cuda(), (torch.from_numpy(at48[0]).cuda(), 48000), (torch.from_numpy(at16[1]).cuda(), 16000),
             str(tmp_path / "c.wav"), (torch.from_numpy(at48[1]).cuda(), 48000), torch.from_numpy(at16[2]).cuda()]
    acc = stats.cal_mean_std(items, NFFT, WIN, HOP, 16000, max_batch=2, num_workers=2)
    host = [at16[0], R.resample(at48[0], 1, 3), at16[1], R.resample(pcm.astype(np.float32) / 32768.0, 1, 3), R.resample(at48[1], 1, 3),
            at16[2]]
    mean, std, n = R.moments(host, "constant")
    m32, s32, _ = R.moments([h.astype(np.float32) for h in host], "constant", dtype=np.float32)
    gm, gs = acc.result()
    fm, fs_ = np.abs(m32 - mean).max(), np.abs(s32 - std).max()
    em, es = np.abs(gm - mean).max(), np.abs(gs - std).max()
    print(f"cal_mean_std: float32 floor mean {fm:.3e} std {fs_:.3e}; device mean {em:.3e} std {es:.3e}")
    assert acc.count == n
    assert em <= 4 * fm and es <= 4 * fs_
    acc.save(str(tmp_path / "mean.txt"), str(tmp_path / "std.txt"))
    lm, ls = np.loadtxt(str(tmp_path / "mean.txt")), np.loadtxt(str(tmp_path / "std.txt"))
    assert np.array_equal(lm, gm) and np.array_equal(ls, gs)
    dm, ds = acc.buffers()
    assert dm.shape == ds.shape == (1, NFFT // 2 + 1, 1, 2) and dm.dtype == torch.float32 and dm.is_cuda
    assert np.array_equal(dm.cpu().numpy(), lm.reshape(1, lm.shape[0], 1, lm.shape[1]).astype(np.float32))
    np_ = O.net_params(True, 4)                                              # the buffers go in as they are (std 0 at Im of bins 0, 256 too)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, SKIP, "real_imag", False, dm, ds)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k not in ("data_mean", "data_std")}, 5)
    sd.update({"data_mean": dm, "data_std": ds})
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y = m.cuda()(torch.from_numpy(at16[0][None]).cuda(), train=False)[0]
    assert y.shape == (1, HOP * (1999 // HOP)) and torch.isfinite(y).all() and float(y.abs().max()) > 0
