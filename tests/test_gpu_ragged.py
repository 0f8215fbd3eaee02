"""Batched enhancement of utterances of different lengths on the MI355X (``lengths=`` of inference.enhance_* / compute_sisdr,
inference.enhance_list): the ragged framing / overlap-add / SI-SDR kernels one by one, and the models against the CPU oracle
run on each utterance alone at its own length.  Every test is a single pass."""
import functools
import importlib
import random

import numpy as np
import pytest
import torch

from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4            # the project's waveform bound (tests/test_gpu_streaming.py TOL, tests/test_gpu_models.py WAVE_TOL)
OP_TOL = 2e-5         # an fp32 operator (tests/test_gpu_ops.py::_conv_case)
BF16X3_TOL = 1e-3     # the bf16x3 mode (tests/test_gpu_models.py)


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.inference"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _load(module, seed, extra=None):
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in module.state_dict().items() if k not in ("data_mean", "data_std")}, seed)
    sd.update(extra or {})
    module.load_state_dict(sd, strict=True)
    return module.cuda()


def _model(base, seed, recon="mask", mean=None, std=None):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, SKIP, recon, False, mean, std)
    return _load(m, seed, None if mean is None else {"data_mean": mean, "data_std": std}), np_


def _batch(lens, seed, fill=0.0):
    """Padded [B, max(lens)] batch of seeded signals (CPU); the padding holds ``fill``."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((len(lens), max(lens)), fill)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randn(n, generator=g) * 0.1
    return x


def _out_len(n):
    return HOP * (n // HOP)


FRAME_LENS = [NFFT // 2 + 1, 1500, 1299, 1701, 2345]        # n_fft/2 + 1, a multiple of hop, hop*k - 1, hop*k + 1, Lmax


def _frames_ragged(x, lens_dev, Tmax):
    """idv_stft_frames_ragged into a NaN-filled scratch -> [win, B, Tp]."""
    _, _, ops, L = _mods()
    B = x.shape[0]
    fr = ops.Planar.empty(1, WIN // 2, B, Tmax, Tmax + 1, x.device)
    fr.buf.fill_(float("nan"))
    L.call("idv_stft_frames_ragged", L.p(x), L.ll(x.stride(0)), L.p(lens_dev), L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.i(Tmax),
           fr.ptr(), L.i(Tmax + 1), L.i(fr.Jp), L.stream_ptr())
    return fr.planes().reshape(WIN, B, Tmax + 1).clone()


def _frames_alone(xb):
    _, _, ops, L = _mods()
    n = xb.shape[0]
    T = 1 + n // HOP
    fr = ops.Planar.empty(1, WIN // 2, 1, T, T + 1, xb.device)
    xb = xb.contiguous()
    L.call("idv_stft_frames", L.p(xb), L.i(1), L.i(n), L.i(NFFT), L.i(WIN), L.i(HOP), L.i(T), fr.ptr(), L.i(T + 1), L.i(fr.Jp),
           L.stream_ptr())
    return fr.planes().reshape(WIN, 1, T + 1)[:, 0].clone()


def _kimage_columns(kimg, ops):
    """hi and lo planes of a KImage as [KO, Jp, 8] int16 views."""
    n = kimg.nplanes // 8 * kimg.Jp * 8
    hi = kimg.buf[ops.IMG_SLACK:ops.IMG_SLACK + n].view(kimg.nplanes // 8, kimg.Jp, 8)
    lo = kimg.buf[ops.IMG_SLACK + kimg.lo_off:ops.IMG_SLACK + kimg.lo_off + n].view(kimg.nplanes // 8, kimg.Jp, 8)
    return hi, lo


def test_framing_is_exact_and_padding_is_never_read():
    _, _, ops, L = _mods()
    lens = FRAME_LENS
    Lmax = max(lens)
    Tmax = 1 + Lmax // HOP
    x0 = _batch(lens, 1).cuda()
    xn = _batch(lens, 1, fill=float("nan")).cuda()
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    got = _frames_ragged(x0, lens_dev, Tmax)
    got_nan = _frames_ragged(xn, lens_dev, Tmax)
    assert torch.isfinite(got_nan).all()
    assert torch.equal(got, got_nan)                               # no sample at or past lens[b] is read
    # a wider buffer at another row pitch gives the same frames
    wide = torch.full((len(lens), Lmax + 77), float("nan"), device="cuda")
    wide[:, :Lmax] = xn
    assert torch.equal(_frames_ragged(wide, lens_dev, Tmax), got)
    for b, n in enumerate(lens):
        Tb = 1 + n // HOP
        alone = _frames_alone(x0[b, :n])
        assert torch.equal(got[:, b, 1:1 + Tb], alone[:, 1:1 + Tb]), (b, n)
        assert float(got[:, b, 0].abs().max()) == 0.0              # guard column
        assert float(got[:, b, 1 + Tb:].abs().max() if Tb < Tmax else 0.0) == 0.0, (b, n)
    # the split-bf16 K-major image form
    B, Tp = len(lens), Tmax + 1
    Jp = ops.Planar.jp_for(B, Tp)
    kimg = ops.KImage((WIN + 63) // 64 * 64, Jp, "cuda")
    kimg.buf.fill_(0x7fc0)
    L.call("idv_stft_frames_kimage_ragged", L.p(xn), L.ll(xn.stride(0)), L.p(lens_dev), L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.i(Tmax),
           kimg.ptr(), L.ll(kimg.lo_off), L.i(Tp), L.i(Jp), L.stream_ptr())
    hi, lo = _kimage_columns(kimg, ops)
    for b, n in enumerate(lens):
        Tb = 1 + n // HOP
        xb = x0[b, :n].contiguous()
        k1 = ops.KImage(kimg.nplanes, ops.Planar.jp_for(1, Tb + 1), "cuda")
        L.call("idv_stft_frames_kimage", L.p(xb), L.i(1), L.i(n), L.i(NFFT), L.i(WIN), L.i(HOP), L.i(Tb), k1.ptr(), L.ll(k1.lo_off),
               L.i(Tb + 1), L.i(k1.Jp), L.stream_ptr())
        h1, l1 = _kimage_columns(k1, ops)
        assert torch.equal(hi[:, b * Tp:b * Tp + 1 + Tb], h1[:, :1 + Tb]) and torch.equal(lo[:, b * Tp:b * Tp + 1 + Tb], l1[:, :1 + Tb]), (b, n)
        assert int(hi[:, b * Tp + 1 + Tb:(b + 1) * Tp].abs().max() if Tb < Tmax else 0) == 0
        assert int(lo[:, b * Tp + 1 + Tb:(b + 1) * Tp].abs().max() if Tb < Tmax else 0) == 0


def test_enhance_ignores_padding_content_and_neighbours():
    _, inf, ops, _ = _mods()
    m, _ = _model(4, 21)
    lens = [2345, 1500, NFFT // 2 + 1, 1701, 1299]
    x0 = _batch(lens, 2).cuda()
    xn = _batch(lens, 2, fill=float("nan")).cuda()
    y0 = inf.enhance_supervised(m, x0, lengths=lens)
    yn = inf.enhance_supervised(m, xn, lengths=torch.tensor(lens))
    assert y0.shape == (len(lens), _out_len(max(lens)))
    assert torch.isfinite(yn).all() and torch.equal(y0, yn)
    for b, n in enumerate(lens):
        assert float(y0[b, _out_len(n):].abs().max() if _out_len(n) < y0.shape[1] else 0.0) == 0.0
        assert float(y0[b, :_out_len(n)].abs().max()) > 0.0
    # another signal of another length in row 1 (Tmax unchanged): every other row is bit-identical
    lens2 = list(lens)
    lens2[1] = 777
    x2 = xn.clone()
    x2[1] = float("nan")
    x2[1, :777] = torch.randn(777, generator=torch.Generator().manual_seed(99)).cuda()
    y2 = inf.enhance_supervised(m, x2, lengths=lens2)
    for b in (0, 2, 3, 4):
        assert torch.equal(y2[b], y0[b]), b
    assert not torch.equal(y2[1], y0[1])
    # a GPU tensor of lengths is refused (it would have to be fetched with a synchronisation)
    with pytest.raises(ValueError, match="GPU tensor"):
        inf.enhance_supervised(m, x0, lengths=torch.tensor(lens).cuda())


def test_op_level_istft_and_sisdr():
    pm, inf, ops, _ = _mods()
    F = NFFT // 2 + 1
    lens = [2345, 1500, NFFT // 2 + 1, 1701, 1299, 2300]
    Tmax = 1 + max(lens) // HOP
    plan = pm.dft_plan(NFFT, WIN, HOP, Tmax, torch.device("cuda"))
    g = torch.Generator().manual_seed(3)
    for div in (1, 2):
        B = len(lens) * div
        spec = ops.Planar.from_tensor5(torch.randn(B, 1, F, Tmax, 2, generator=g).cuda())
        y = ops.istft(spec, plan, lengths=lens)
        assert y.shape == (B, HOP * (Tmax - 1))
        for r in range(B):
            n = lens[r // div]
            Tb = 1 + n // HOP
            alone = ops.istft(ops.Planar.from_tensor5(spec.tensor5()[r:r + 1, :, :, :Tb].contiguous()),
                              pm.dft_plan(NFFT, WIN, HOP, Tb, torch.device("cuda")))
            e = relerr(y[r, :HOP * (Tb - 1)], alone[0])
            print(f"istft div={div} row={r} len={n}: relerr {e:.3e}")
            assert e < OP_TOL, (div, r, e)
            assert float(y[r, HOP * (Tb - 1):].abs().max() if Tb < Tmax else 0.0) == 0.0
        # against torch.istft semantics through the oracle, one row
        r = B - 2
        Tb = 1 + lens[r // div] // HOP
        want = O.istft(spec.tensor5()[r:r + 1, 0, :, :Tb].cpu(), NFFT, HOP, WIN)
        assert relerr(y[r:r + 1, :HOP * (Tb - 1)], want) < OP_TOL
    # SI-SDR over the first lens[b] samples
    ref = _batch(lens, 4, fill=float("nan"))
    est = ref + 0.3 * _batch(lens, 5)
    est[torch.isnan(ref)] = 7.0                                   # finite rubbish in the estimate's padding
    got = inf.compute_sisdr(est.cuda(), ref.cuda(), lengths=lens).cpu()
    trunc = torch.stack([inf.compute_sisdr(est[b, :n].cuda(), ref[b, :n].cuda()) for b, n in enumerate(lens)]).cpu()
    want = torch.tensor([float(O.sisdr_np(est[b, :n].numpy(), ref[b, :n].numpy())) for b, n in enumerate(lens)])
    print("sisdr ragged", got.tolist(), "truncated", trunc.tolist(), "oracle", want.tolist())
    assert torch.isfinite(got).all()
    assert relerr(got, trunc) < OP_TOL and relerr(got, want) < OP_TOL
    # the padded widths of the two inputs may differ
    assert torch.equal(inf.compute_sisdr(est[:, :2345].cuda(), torch.cat([ref, ref], 1).cuda(), lengths=lens).cpu(), got)


def _parity(m, np_, x, lens, recon="mask", mean=None, std=None, tol=TOL, alone_too=True, tag=""):
    _, inf, _, _ = _mods()
    y = inf.enhance_supervised(m, x.cuda(), lengths=lens)
    assert y.shape == (len(lens), _out_len(max(lens)))
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    for b, n in enumerate(lens):
        want = O.dccrn_forward(x[b:b + 1, :n], sd, np_, True, NFFT, HOP, WIN, SKIP, recon, False, None, mean, std)[0]
        got = y[b:b + 1, :_out_len(n)]
        e = relerr(got, want)
        msg = f"{tag} row {b} len {n}: vs oracle {e:.3e}"
        if alone_too:
            with torch.no_grad():
                own = m(x[b:b + 1, :n].cuda(), train=False)[0]
            e2 = relerr(got, own)
            msg += f", vs alone {e2:.3e}"
        print(msg)
        assert got.shape == want.shape and e < tol, msg
        if alone_too:
            assert e2 < tol, msg
        assert float(y[b, _out_len(n):].abs().max() if _out_len(n) < y.shape[1] else 0.0) == 0.0
    return y


MINI_LENS = [3456, 1500, NFFT // 2 + 1, 2999, 3401, 800]


def test_model_parity_mini_mask_and_datanorm(golden):
    lens = MINI_LENS
    x = _batch(lens, 6, fill=float("nan"))
    m, np_ = _model(4, 22)
    _parity(m, np_, x, lens, tag="mask")
    d = golden("dccrn_datanorm_mini")
    mean, std = torch.from_numpy(np.asarray(d["data_mean"])), torch.from_numpy(np.asarray(d["data_std"]))
    m, np_ = _model(4, int(d["seed"]), "real_imag", mean, std)
    _parity(m, np_, x, lens, "real_imag", mean, std, tag="real_imag+datanorm")


def test_model_parity_stream_split_gives_each_part_its_lengths():
    _, inf, ops, _ = _mods()
    lens = MINI_LENS
    x = _batch(lens, 6, fill=float("nan"))
    m, np_ = _model(4, 22)
    keep = (ops.STREAM_SPLIT, ops.STREAM_SPLIT_MIN_BATCH)
    try:
        ops.STREAM_SPLIT_MIN_BATCH = 1
        ops.STREAM_SPLIT = 1
        y1 = inf.enhance_supervised(m, x.cuda(), lengths=lens)
        ops.STREAM_SPLIT = 2
        assert ops.stream_split(len(lens)) == 2
        y2 = _parity(m, np_, x, lens, alone_too=False, tag="split2")
        torch.cuda.synchronize()
        assert torch.equal(y1, y2)
    finally:
        ops.STREAM_SPLIT, ops.STREAM_SPLIT_MIN_BATCH = keep


def test_model_parity_full_width():
    lens = [64000, 8000, 23456, 40100]                            # 0.5 s .. 4 s, one not a multiple of hop
    x = _batch(lens, 7, fill=float("nan"))
    m, np_ = _model(32, 23)
    _parity(m, np_, x, lens, tag="full")


def test_resynthesis_frames_the_outputs_at_their_own_lengths():
    pm = _mods()[0]
    lens = [3456, 1500, 300, 2999]
    x = _batch(lens, 9, fill=float("nan"))
    np_ = O.net_params(True, 4)
    m = _load(pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, SKIP, "mask", True, None, None), 25)
    with torch.no_grad():
        clean, predict = m(x.cuda(), train=False, lengths=lens)
    assert predict.shape == (len(lens), NFFT // 2 + 1, 1 + max(lens) // HOP)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    for b, n in enumerate(lens):
        Tb = 1 + n // HOP
        want = O.stft(O.dccrn_forward(x[b:b + 1, :n], sd, np_, True, NFFT, HOP, WIN, SKIP)[0], NFFT, HOP, WIN)
        with torch.no_grad():
            own = m(x[b:b + 1, :n].cuda(), train=False)[1]
        got = torch.view_as_real(predict[b:b + 1, :, :Tb])
        e, e2 = relerr(got, want), relerr(got, torch.view_as_real(own))
        print(f"resynthesis row {b} len {n}: vs oracle {e:.3e}, vs alone {e2:.3e}")
        assert got.shape == want.shape and e < TOL and e2 < TOL, (b, e, e2)
    with pytest.raises(ValueError, match="resynthesis"):
        m(x.cuda(), train=False, lengths=[3456, 1500, 299, 2999])


def test_model_parity_bf16x3():
    ops = _mods()[2]
    lens = MINI_LENS
    x = _batch(lens, 6, fill=float("nan"))
    m, np_ = _model(4, 22)
    keep = ops.PRECISION
    try:
        ops.set_precision("bf16x3")
        _parity(m, np_, x, lens, tol=BF16X3_TOL, alone_too=False, tag="bf16x3")
    finally:
        ops.set_precision(keep)


def _vae(ns, zdim, base=4):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    enc = _load(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2), 41)
    mk = lambda seed: _load(pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP, False), seed)
    return enc, mk(42), mk(43), np_


def test_vae_paths():
    _, inf, _, _ = _mods()
    base, zdim, ns = 4, 16, 3
    lens = [2345, 1500, NFFT // 2 + 1, 1701]
    B, Tmax = len(lens), 1 + max(lens) // HOP
    enc, dec_s, dec_n, np_ = _vae(ns, zdim, base)
    x = _batch(lens, 8, fill=float("nan"))
    g = torch.Generator().manual_seed(11)
    eps = [torch.randn(B, ns, Tmax, zdim, generator=g) for _ in range(4)]
    eps_d = tuple(e.cuda() for e in eps)
    got = {"vae": inf.enhance_vae(enc, dec_s, x.cuda(), eps=eps_d, lengths=lens),
           "clean_direct": inf.enhance_vae_two_latents(enc, dec_s, dec_n, x.cuda(), "clean_direct", 2, eps=eps_d, lengths=lens),
           "phase_mask": inf.enhance_vae_two_latents(enc, dec_s, dec_n, x.cuda(), "phase_mask", 2, eps=eps_d, lengths=lens)}
    sd_e = {k: v.cpu() for k, v in enc.state_dict().items()}
    sd_s = {k: v.cpu() for k, v in dec_s.state_dict().items()}
    sd_n = {k: v.cpu() for k, v in dec_n.state_dict().items()}
    for v in got.values():
        assert v.shape == (B, HOP * (Tmax - 1)) and torch.isfinite(v).all()
    for b, n in enumerate(lens):
        Tb = 1 + n // HOP
        oe = O.vae_encoder_forward(x[b:b + 1, :n], sd_e, np_, True, zdim, NFFT, HOP, WIN, ns, 2, [e[b:b + 1, :, :Tb] for e in eps], False)
        dec = lambda sd_d, z: O.vae_decoder_forward(oe["stft_x"], z, oe["skiper"], 8 * base, 5, sd_d, np_, True, ns, NFFT, HOP, WIN,
                                                    "mask", SKIP, "sig", True, False)
        rec_s, pred_s = dec(sd_s, oe["z_speech"])
        _, pred_n = dec(sd_n, oe["z_noise"])
        as_c = lambda t: t if t.is_complex() else torch.view_as_complex(t.contiguous())
        est = O.outtype_phase_sensitive_mask(as_c(pred_n), as_c(pred_s), oe["stft_x"])
        want = {"vae": rec_s.mean(0, keepdim=True), "clean_direct": rec_s.mean(0, keepdim=True),
                "phase_mask": O.istft(torch.view_as_real(est)[None], NFFT, HOP, WIN)}
        for k, v in got.items():
            e = relerr(v[b:b + 1, :_out_len(n)], want[k])
            print(f"vae {k} row {b} len {n}: relerr {e:.3e}")
            assert want[k].shape == (1, _out_len(n)) and e < TOL, (k, b, e)
            assert float(v[b, _out_len(n):].abs().max() if _out_len(n) < v.shape[1] else 0.0) == 0.0


def test_enhance_list_returns_the_callers_order():
    _, inf, _, _ = _mods()
    m, _ = _model(4, 24)
    rng = random.Random(37)
    lens = [rng.randint(4800, 64000) for _ in range(37)]          # 0.3 s .. 4 s
    g = torch.Generator().manual_seed(12)
    signals = [(torch.randn(n, generator=g) * 0.1).cuda() for n in lens]
    outs = inf.enhance_list(functools.partial(inf.enhance_supervised, m), signals, HOP, max_batch=8)
    assert len(outs) == len(lens)
    worst = 0.0
    for k, (sgn, y) in enumerate(zip(signals, outs)):
        assert y.shape == (_out_len(lens[k]),), k
        with torch.no_grad():
            own = m(sgn[None], train=False)[0][0]
        e = relerr(y, own)
        worst = max(worst, e)
        assert e < TOL, (k, lens[k], e)
    print(f"enhance_list: worst relerr vs alone {worst:.3e}")
    batches = inf.plan_ragged_batches(lens, HOP, max_batch=8)
    assert max(len(b) for b in batches) <= 8 and sorted(k for b in batches for k in b) == list(range(37))
