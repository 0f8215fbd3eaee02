"""Streaming two-latent I-DCCRN-VAE enhancement (streaming.StreamingVAETwoLatents) on the MI355X: the two new entries one by
one, chunk invariance to the bit, parity with the offline path (inference.enhance_vae_two_latents) and the CPU oracle for every
outtype at both phases, clean_direct against StreamingVAE, an eps callable, both conv engines, stream independence and reuse
after flush."""
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
TOL = 1e-4          # the streaming-to-offline bar of tests/test_gpu_streaming.py
TOL_ORACLE = 2e-4   # the bar of tests/test_gpu_models.py::test_two_latent_evaluation_path
OUTTYPES = ["clean_direct", "real_imag_mask", "complex_mask", "phase_mask"]


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.streaming"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"),
            importlib.import_module("i-dccrn-vae_amd.inference"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def load_synth(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(O.synth_state_dict(shapes, seed), strict=True)
    return module.cuda()


def _trio(base, zdim, ns, phase, seed=40, recon=None, zero_class=True):
    """(noisy encoder, speech decoder, noise decoder, net params): phase 2 fine-tuned decoders (mask), phase 1 the pre-trained
    zero-skip class (real_imag) or, ``zero_class=False``, the fine-tuned class run with zero skips."""
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    enc = load_synth(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2), seed + 1)
    if phase == 1 and zero_class:
        mk = lambda sd: load_synth(pm.pvae_dccrn_decoder_skip_prepare(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "real_imag", SKIP), sd)
    else:
        mk = lambda sd: load_synth(pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, recon or "mask",
                                                                        True, SKIP, False), sd)
    return enc, mk(seed + 2), mk(seed + 3), np_


def _signal(B, L, seed):
    return (torch.randn(B, L, generator=torch.Generator().manual_seed(seed)) * 0.1).cuda()


def _stream(st, x, sizes, check_counts=False):
    outs, n = [], 0
    for m in sizes:
        y = st.push(x[:, n:n + m])
        n += m
        if check_counts:        # StreamPlan's k(n) and final samples, unchanged
            k = 0 if n <= WIN // 2 else (n - WIN // 2) // HOP + 1
            assert sum(o.shape[1] for o in outs) + y.shape[1] == max(0, HOP * k - WIN // 2)
        outs.append(y)
    assert n == x.shape[1]
    outs.append(st.flush())
    return torch.cat(outs, dim=1)


def _hops(L, n=HOP):
    return [n] * (L // n) + ([L % n] if L % n else [])


# ----------------------------------------------------------------------------------------------------------- 1. the draws
M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (integers exact) -> the four output words."""
    u = np.uint64
    c0, c1, c2, c3 = [np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3)]
    k0, k1 = u(k0), u(k1)
    for _ in range(10):
        p0, p1 = u(M0) * c0, u(M1) * c2
        n0, n2 = (p1 >> u(32)) ^ c1 ^ k0, (p0 >> u(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & u(MASK), p0 & u(MASK), n0, n2
        k0, k1 = (k0 + u(W0)) & u(MASK), (k1 + u(W1)) & u(MASK)
    return c0, c1, c2, c3


def noise_eps_reference(seed, t0, k, B, ns, zdim):
    """float64 Box-Muller on words 2 and 3 -> (eps_nr, eps_ni) [B, ns, k, zdim]."""
    bs, t, uu = np.meshgrid(np.arange(B * ns, dtype=np.uint64), np.arange(t0, t0 + k, dtype=np.uint64),
                            np.arange(zdim, dtype=np.uint64), indexing="ij")
    _, _, w2, w3 = philox4x32_10(seed & MASK, seed >> 32, t & np.uint64(MASK), t >> np.uint64(32), bs, uu)
    u1 = ((w2 >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    th = 2.0 * np.pi * (w3 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return (r * np.cos(th)).reshape(B, ns, k, zdim), (r * np.sin(th)).reshape(B, ns, k, zdim)


def _eps(seed, t0, k, B, ns, zdim):
    L = _mods()[3]
    out = torch.empty(2, B, ns, k, zdim, device="cuda")
    L.call("idv_stream_eps", L.ll(seed), L.ll(t0), L.i(k), L.i(B), L.i(ns), L.i(zdim), L.p(out[0]), L.p(out[1]), L.stream_ptr())
    return out[0].cpu(), out[1].cpu()


def _eps_pair(seed, t0, k, B, ns, zdim):
    L = _mods()[3]
    out = torch.empty(4, B, ns, k, zdim, device="cuda")
    L.call("idv_stream_eps_pair", L.ll(seed), L.ll(t0), L.i(k), L.i(B), L.i(ns), L.i(zdim), L.p(out[0]), L.p(out[1]), L.p(out[2]),
           L.p(out[3]), L.stream_ptr())
    return tuple(out.cpu())


def test_eps_pair_kernel():
    assert [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in philox4x32_10(MASK, MASK, MASK, MASK, MASK, MASK)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    B, ns, k, zdim = 4, 2, 64, 16
    for seed, t0 in ((0, 0), (0x1234567890ABCDEF >> 1, 7), (3, 2 ** 32 + 5)):
        sr, si, nr, ni = _eps_pair(seed, t0, k, B, ns, zdim)
        er, ei = _eps(seed, t0, k, B, ns, zdim)
        assert torch.equal(sr, er) and torch.equal(si, ei), (seed, t0)           # the speech pair is idv_stream_eps's, to the bit
        wr, wi = noise_eps_reference(seed, t0, k, B, ns, zdim)
        err = max(float((nr.double() - torch.from_numpy(wr)).abs().max()), float((ni.double() - torch.from_numpy(wi)).abs().max()))
        print(f"noise draws vs float64 Box-Muller on words 2, 3; seed {seed} t0 {t0}: max abs err {err:.3e}")
        assert err < 1e-5, (seed, t0)
        assert not torch.equal(nr, sr) and not torch.equal(ni, si) and not torch.equal(nr, si) and not torch.equal(ni, sr)
    # a noise draw is a function of (seed, b, s, t, u) alone
    a = _eps_pair(5, 0, 7, B, ns, zdim)
    b = _eps_pair(5, 3, 2, B, ns, zdim)
    assert all(torch.equal(u[:, :, 3:5], v) for u, v in zip(a, b))
    a2 = _eps_pair(5, 0, 7, 2, ns, zdim)             # fewer streams: the streams that stay keep their draws
    assert all(torch.equal(u[:2], v) for u, v in zip(a, a2))
    c = _eps_pair(6, 0, 7, B, ns, zdim)
    assert all(not torch.equal(u, v) for u, v in zip(a, c))
    for part in a[2:]:                               # per b and per s
        assert not torch.equal(part[0], part[1]) and not torch.equal(part[:, 0], part[:, 1])
    far, near = _eps_pair(5, 2 ** 32 + 5, 4, B, ns, zdim), _eps_pair(5, 5, 4, B, ns, zdim)
    assert not torch.equal(far[2], near[2]) and not torch.equal(far[3], near[3])
    d = torch.cat([t.reshape(-1) for t in _eps_pair(11, 0, k, B, ns, zdim)[2:]]).double()      # 16 384 draws: 6 sigma of the mean is 0.047
    assert abs(float(d.mean())) < 0.05 and abs(float(d.var()) - 1.0) < 0.1


# ------------------------------------------------------------------------------------------------ 2. the estimator entry
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("recon", ["mask", "real_imag"])
def test_estimate_entry(recon, k):
    _, _, ops, L, inf = _mods()
    F, B, ns = 257, 3, 3
    Bn, Tp = B * ns, k + 1
    g = torch.Generator().manual_seed(17 + k)
    sp5, no5 = (torch.randn(Bn, 1, F, k, 2, generator=g).cuda() for _ in range(2))
    x5 = torch.randn(B, 1, F, k, 2, generator=g).cuda()
    sp, no, X = (ops.Planar.from_tensor5(t, Tp) for t in (sp5, no5, x5))
    if recon == "mask":          # the decoders' `predict` of the offline path: idv_mask_apply with x_div = ns
        preds = []
        for m in (sp, no):
            pl = ops.Planar.empty(1, F, Bn, k, Tp, "cuda", zero=True)
            pc = torch.empty(Bn, F, k, 2, device="cuda")
            L.call("idv_mask_apply", m.ptr(), X.ptr(), L.i(ns), L.i(X.Jp), pl.ptr(), L.p(pc), L.i(F), L.i(Bn), L.i(k), L.i(Tp),
                   L.i(m.Jp), L.stream_ptr())
            preds.append(torch.view_as_complex(pc))
    else:
        preds = [torch.view_as_complex(t[:, 0].contiguous()) for t in (sp5, no5)]
    for name, mode in inf.OUTTYPES.items():
        _, want = inf.outtype_estimate(preds[1], preds[0], x5[:, 0], name, ns)
        out = ops.Planar.empty(1, F, B, k, Tp, "cuda")
        out.buf.fill_(7.0)
        L.call("idv_stream_estimate", sp.ptr(), no.ptr(), X.ptr(), L.i(1 if recon == "mask" else 0), L.i(mode), L.i(ns), L.i(F),
               L.i(B), L.i(k), L.i(Tp), L.i(X.Jp), L.i(sp.Jp), out.ptr(), L.stream_ptr())
        got = out.tensor5()[:, 0]
        err = relerr(got, torch.view_as_real(want))
        print(f"idv_stream_estimate {recon} k {k} {name}: relerr {err:.3e}")
        assert err < 1e-5, name
        assert torch.all(out.planes()[..., 0] == 7.0)                        # the guard column of every row is untouched
        assert torch.all(out.buf[:ops.SLACK] == 7.0) and torch.all(out.buf[ops.SLACK + 2 * F * out.Jp:] == 7.0)
        if out.Jp > B * Tp:                                                  # nor the padding of a row
            pad = torch.as_strided(out.buf, (2 * F, out.Jp - B * Tp), (out.Jp, 1), ops.SLACK + B * Tp)
            assert torch.all(pad == 7.0)


# -------------------------------------------------------------------------------------------------- 3. chunk invariance
def _random_sizes(L, seed):
    rng = random.Random(seed)
    out, left = [], L
    while left:
        n = min(left, rng.choice([0, 0, 1, 13, 99, 100, 250, 777]))
        out.append(n)
        left -= n
    return out


def test_chunk_invariance_bit_identical():
    S = _mods()[1]
    zdim, ns, B, L = 16, 3, 3, 2345
    enc, dec_s, dec_n, _ = _trio(4, zdim, ns, 2)
    x = _signal(B, L, 5)
    st = S.StreamingVAETwoLatents(enc, dec_s, dec_n, batch=B, outtype="phase_mask", phase=2, seed=3, frames_per_launch=8)
    assert st.H == 96 and st.cap == 8
    chunkings = {"whole": [L], "1then100": [1] * 700 + [100] * ((L - 700) // 100) + [(L - 700) % 100],
                 "hop": _hops(L), "37": _hops(L, 37), "random": _random_sizes(L, 3), "over_cap": [1500, L - 1500]}
    assert 0 in chunkings["random"]
    ys = {k: _stream(st, x, v, check_counts=True) for k, v in chunkings.items()}
    base = ys["whole"]
    assert base.shape == (B, HOP * (L // HOP)) and bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    for k, y in ys.items():
        assert torch.equal(y, base), k


# ------------------------------------------------------------------------------------------------------------- 4. parity
@functools.lru_cache(maxsize=None)
def _parity_case(phase):
    """Models, input, the streamer's draws and the CPU oracle's encoder and decoder outputs for one phase, computed once and
    shared by the four outtypes (nobody writes to them)."""
    L = _mods()[3]
    base, zdim, ns, B, Lx = 4, 16, 3, 2, 1600
    T = 1 + Lx // HOP
    enc, dec_s, dec_n, np_ = _trio(base, zdim, ns, phase, seed=40)
    x = _signal(B, Lx, 10)
    eps = _eps_pair(7, 0, T, B, ns, zdim)
    sd_e = {k: v.cpu() for k, v in enc.state_dict().items()}
    oe = O.vae_encoder_forward(x.cpu(), sd_e, np_, True, zdim, NFFT, HOP, WIN, ns, 2, list(eps), False)

    def odec(dec, z):
        sd_d = {k: v.cpu() for k, v in dec.state_dict().items()}
        if phase == 2:
            return O.vae_decoder_forward(oe["stft_x"], z, oe["skiper"], 8 * base, 5, sd_d, np_, True, ns, NFFT, HOP, WIN, "mask", SKIP,
                                         "sig", True, False)
        return O.vae_decoder_forward(oe["stft_x"], z, oe["skiper"], 8 * base, 5, sd_d, np_, True, ns, NFFT, HOP, WIN, "real_imag", SKIP,
                                     "zero", True, False)
    rec_s, pred_s = odec(dec_s, oe["z_speech"])
    _, pred_n = odec(dec_n, oe["z_noise"])
    return dict(enc=enc, dec_s=dec_s, dec_n=dec_n, x=x, eps=eps, oe=oe, rec_s=rec_s, pred_s=pred_s, pred_n=pred_n, B=B, ns=ns, T=T)


def _oracle(c, outtype):
    B, ns = c["B"], c["ns"]
    if outtype == "clean_direct":
        return c["rec_s"].view(B, ns, -1).mean(1)
    fn = {"real_imag_mask": O.outtype_real_imag_mask, "complex_mask": O.outtype_complex_mask,
          "phase_mask": O.outtype_phase_sensitive_mask}[outtype]
    as_c = lambda t: t if t.is_complex() else torch.view_as_complex(t.contiguous())
    ps, pn = as_c(c["pred_s"]), as_c(c["pred_n"])
    ps, pn = ps.view(B, ns, *ps.shape[1:]), pn.view(B, ns, *pn.shape[1:])
    est = torch.stack([fn(pn[b], ps[b], c["oe"]["stft_x"][b:b + 1]) for b in range(B)])
    return O.istft(torch.view_as_real(est), NFFT, HOP, WIN)


# The streaming-to-offline bar per outtype: TOL unless the rule of the parity test's docstring applies.
OFFLINE_BAR = {(o, ph): TOL for o in OUTTYPES for ph in (1, 2)}


@pytest.mark.parametrize("outtype", OUTTYPES)
@pytest.mark.parametrize("phase", [1, 2])
def test_parity_offline_and_oracle(outtype, phase):
    """Streamed by hops with the streamer's own draws against inference.enhance_vae_two_latents given the same four draws
    (bar 1e-4, the streaming-to-offline bar) and against the CPU oracle composed as test_two_latent_evaluation_path composes
    it (bar 2e-4, that test's bar).  An estimator divides by a sum that can be small, so both paths amplify their rounding
    there; should one miss 1e-4 on these inputs while the offline path itself passes 2e-4 against the oracle, its bar is twice
    the offline path's own error against the oracle on the same input (OFFLINE_BAR), with the measured numbers recorded here."""
    _, S, _, _, inf = _mods()
    c = _parity_case(phase)
    st = S.StreamingVAETwoLatents(c["enc"], c["dec_s"], c["dec_n"], batch=c["B"], outtype=outtype, phase=phase, seed=7)
    own = st.eps(0, c["T"])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(own, c["eps"]))
    y = _stream(st, c["x"], _hops(c["x"].shape[1]), check_counts=True)
    off = inf.enhance_vae_two_latents(c["enc"], c["dec_s"], c["dec_n"], c["x"], outtype, phase, eps=own)
    orc = _oracle(c, outtype)
    assert y.shape == off.shape == orc.shape
    e_off, e_orc, e_off_orc = relerr(y, off), relerr(y, orc), relerr(off, orc)
    print(f"two latents {outtype} phase {phase}: vs offline {e_off:.3e}, vs CPU oracle {e_orc:.3e}, offline vs oracle {e_off_orc:.3e}")
    assert e_off < OFFLINE_BAR[outtype, phase] and e_orc < TOL_ORACLE


def test_phase1_with_the_fine_tuned_class():
    """Zero skips apply to either decoder class: nsvae_pvae_dccrn_decoder_twophase (mask) run as pad='zero' offline."""
    _, S, _, _, inf = _mods()
    zdim, ns, B, L = 16, 2, 2, 900
    enc, dec_s, dec_n, _ = _trio(4, zdim, ns, 1, seed=60, zero_class=False)
    x = _signal(B, L, 12)
    for outtype in ("clean_direct", "complex_mask"):
        st = S.StreamingVAETwoLatents(enc, dec_s, dec_n, batch=B, outtype=outtype, phase=1, seed=1)
        assert st.skip_n == {} and all(cp.C1 == 0 for cp in st.speech.dec)       # no skip, and no zeros, are read
        y = _stream(st, x, _hops(L))
        off = inf.enhance_vae_two_latents(enc, dec_s, dec_n, x, outtype, 1, eps=st.eps(0, 1 + L // HOP))
        print(f"phase 1, fine-tuned class, {outtype}: vs offline {relerr(y, off):.3e}")
        assert y.shape == off.shape and relerr(y, off) < TOL


# -------------------------------------------------------------------------------------------- 5. clean_direct at phase 2
def test_clean_direct_phase2_is_streaming_vae():
    S = _mods()[1]
    zdim, ns, B, L = 16, 2, 3, 1234
    enc, dec_s, dec_n, _ = _trio(4, zdim, ns, 2, seed=70)
    x = _signal(B, L, 9)
    sizes = _hops(L, 160)
    want = _stream(S.StreamingVAE(enc, dec_s, batch=B, seed=2, latent="speech"), x, sizes)
    for dn in (None, dec_n):
        st = S.StreamingVAETwoLatents(enc, dec_s, dn, batch=B, outtype="clean_direct", phase=2, seed=2)
        assert len(st.conv_engines) == 12 and st.noise is None
        assert torch.equal(_stream(st, x, sizes), want)


# ------------------------------------------------------------------------- 6. an eps callable, engines, independence, reuse
def test_eps_callable_engines_independence_reuse():
    _, S, _, L, _ = _mods()
    zdim, ns, B, Lx = 16, 2, 3, 1234
    enc, dec_s, dec_n, _ = _trio(4, zdim, ns, 2, seed=70)
    x = _signal(B, Lx, 9)
    sizes = _hops(Lx, 160)
    mk = lambda **kw: S.StreamingVAETwoLatents(enc, dec_s, dec_n, batch=B, outtype="complex_mask", phase=2, **kw)
    st = mk(seed=2)
    a = _stream(st, x, sizes)
    # the four draws through an eps callable
    four = st.eps(0, 1 + Lx // HOP)
    asked = []

    def draws(t0, k):
        asked.append((t0, k))
        return tuple(e[:, :, t0:t0 + k] for e in four)
    assert torch.equal(_stream(mk(seed=99, eps=draws), x, sizes), a)
    assert sum(k for _, k in asked) == 1 + Lx // HOP and [t for t, _ in asked] == sorted(t for t, _ in asked)
    with pytest.raises(ValueError, match="eps_nr"):
        mk(eps=lambda t0, k: four[:2]).push(x[:, :400])
    # engines
    stm = mk(seed=2, conv="mfma")
    sup = L.lib().idv_stream_cconv_mfma_supported
    packs = stm.enc + stm.speech.dec + stm.noise.dec
    want = ["mfma" if sup(1 if cp.transposed else 0, cp.C0 + cp.C1, cp.Cout) == 1 else "valu" for cp in packs]
    assert len(stm.conv_engines) == 18 and stm.conv_engines == want and "mfma" in want and st.conv_engines == ["valu"] * 18
    assert torch.equal(_stream(stm, x, sizes), a)
    # stream 1's input changes: streams 0 and 2 keep their bits
    g = torch.Generator().manual_seed(1)
    x2 = x.clone()
    x2[1] = torch.randn(Lx, generator=g).cuda()
    b = _stream(st, x2, sizes)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])
    # after flush the streamer is as new
    x3 = _signal(B, 1100, 11)
    again = _stream(st, x3, [250] * 4 + [100])
    assert torch.equal(again, _stream(mk(seed=2), x3, [250] * 4 + [100]))
    # another seed, other draws
    st.seed = 4
    assert st.seed == 4 and not torch.equal(_stream(st, x, sizes), a)


# ------------------------------------------------------------------------------------------------------ 7. full width once
def test_full_width():
    _, S, _, _, inf = _mods()
    zdim, ns, B, L = 128, 2, 1, 1600
    enc, dec_s, dec_n, _ = _trio(32, zdim, ns, 2, seed=80)
    x = _signal(B, L, 10)
    mk = lambda conv: S.StreamingVAETwoLatents(enc, dec_s, dec_n, batch=B, outtype="phase_mask", phase=2, seed=5, conv=conv)
    st, stm = mk("valu"), mk("mfma")
    assert st.H == 768 and len(stm.conv_engines) == 18 and stm.conv_engines.count("mfma") == 16
    y = _stream(st, x, _hops(L), check_counts=True)
    assert torch.equal(_stream(stm, x, _hops(L)), y)
    off = inf.enhance_vae_two_latents(enc, dec_s, dec_n, x, "phase_mask", 2, eps=st.eps(0, 1 + L // HOP))
    assert y.shape == off.shape
    print(f"full width StreamingVAETwoLatents vs enhance_vae_two_latents: {relerr(y, off):.3e}")
    assert relerr(y, off) < TOL
