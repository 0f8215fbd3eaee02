"""Streaming I-DCCRN-VAE enhancement (streaming.StreamingVAE) on the MI355X: the three new kernels one by one, chunk invariance
to the bit, parity with the offline path (inference.enhance_vae), the CPU oracle and the reference's own outputs, both conv
engines, stream independence and reuse after flush."""
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


def _pair(base, zdim, ns, latent_num, recon="mask", seed=40, skip_prepare=False):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    if skip_prepare:
        enc = pm.pvae_dccrn_encoder_skip_prepare(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns)
    else:
        enc = pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, latent_num)
    dec = pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, recon, True, SKIP, False)
    return load_synth(enc, seed + 2), load_synth(dec, seed + 3), np_


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


# --------------------------------------------------------------------------------------------------------- 1. the eps kernel
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


def eps_reference(seed, t0, k, B, ns, zdim):
    """float64 Box-Muller on words 0 and 1 -> (eps_r, eps_i) [B, ns, k, zdim]."""
    bs, t, uu = np.meshgrid(np.arange(B * ns, dtype=np.uint64), np.arange(t0, t0 + k, dtype=np.uint64),
                            np.arange(zdim, dtype=np.uint64), indexing="ij")
    w0, w1, _, _ = philox4x32_10(seed & MASK, seed >> 32, t & np.uint64(MASK), t >> np.uint64(32), bs, uu)
    u1 = ((w0 >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    th = 2.0 * np.pi * (w1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return (r * np.cos(th)).reshape(B, ns, k, zdim), (r * np.sin(th)).reshape(B, ns, k, zdim)


def _eps(seed, t0, k, B, ns, zdim):
    L = _mods()[3]
    out = torch.empty(2, B, ns, k, zdim, device="cuda")
    L.call("idv_stream_eps", L.ll(seed), L.ll(t0), L.i(k), L.i(B), L.i(ns), L.i(zdim), L.p(out[0]), L.p(out[1]), L.stream_ptr())
    return out[0].cpu(), out[1].cpu()


def test_eps_kernel():
    # the restatement itself against the published known answers of Philox4x32-10 (Random123 kat_vectors)
    assert [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in philox4x32_10(MASK, MASK, MASK, MASK, MASK, MASK)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    B, ns, k, zdim = 4, 2, 64, 16
    for seed, t0 in ((0, 0), (0x1234567890ABCDEF >> 1, 7), (3, 2 ** 32 + 5)):
        er, ei = _eps(seed, t0, k, B, ns, zdim)
        wr, wi = eps_reference(seed, t0, k, B, ns, zdim)
        err = max(float((er.double() - torch.from_numpy(wr)).abs().max()), float((ei.double() - torch.from_numpy(wi)).abs().max()))
        print(f"eps kernel vs float64 Box-Muller, seed {seed} t0 {t0}: max abs err {err:.3e}")
        assert err < 1e-5, (seed, t0)
    # a draw is a function of (seed, b, s, t, u) alone
    a = _eps(5, 0, 7, B, ns, zdim)
    b = _eps(5, 3, 2, B, ns, zdim)
    assert torch.equal(a[0][:, :, 3:5], b[0]) and torch.equal(a[1][:, :, 3:5], b[1])
    a2 = _eps(5, 0, 7, 2, ns, zdim)                  # fewer streams: the streams that stay keep their draws
    assert torch.equal(a[0][:2], a2[0]) and torch.equal(a[1][:2], a2[1])
    c = _eps(6, 0, 7, B, ns, zdim)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    for part in a:                                   # per b and per s
        assert not torch.equal(part[0], part[1]) and not torch.equal(part[:, 0], part[:, 1])
    far, near = _eps(5, 2 ** 32 + 5, 4, B, ns, zdim), _eps(5, 5, 4, B, ns, zdim)
    assert not torch.equal(far[0], near[0]) and not torch.equal(far[1], near[1])
    er, ei = _eps(11, 0, k, B, ns, zdim)
    for part in (er, ei):
        d = part.double()
        assert abs(float(d.mean())) < 0.05 and abs(float(d.var()) - 1.0) < 0.1
    d = torch.cat([er.reshape(-1), ei.reshape(-1)]).double()      # 16 384 draws: 6 sigma of the mean is 0.047
    assert abs(float(d.mean())) < 0.05 and abs(float(d.var()) - 1.0) < 0.1


# ------------------------------------------------------------------------------------------------ 2. the wide LSTM entry
def _lstm_case(H, B, k, seed):
    g = torch.Generator().manual_seed(seed)
    sc = 1.0 / H ** 0.5
    wt = (torch.rand(2, 3, H, 4 * H, generator=g) * 2 - 1) * sc          # [set][W_hh0, W_ih1, W_hh1][H][4H] (transposed)
    b1 = (torch.rand(2, 4 * H, generator=g) * 2 - 1) * sc
    G = torch.randn(2, k, B, 8 * H, generator=g)
    state = torch.randn(4, 2, 2, B, H, generator=g) * 0.5
    return wt, b1, G, state


def _lstm_cpu(wt, b1, G, state, H, B, k):
    """float64 restatement: four real two-layer LSTM runs (gates i, f, g, o) from a given state; real = rr - ii, imag = ir + ri."""
    wt, b1, G, st = wt.double(), b1.double(), G.double(), state.double().clone()
    u = torch.arange(H)
    hs = torch.zeros(4, k, B, H, dtype=torch.float64)
    for run in range(4):
        z, s = run >> 1, run & 1
        col = torch.cat([s * 4 * H + ((u // 16) * 4 + g) * 16 + u % 16 for g in range(4)])      # column of gate row g*H + u
        h0, c0, h1, c1 = st[run, 0, 0], st[run, 0, 1], st[run, 1, 0], st[run, 1, 1]
        for t in range(k):
            def cell(pre, c):
                i_, f_, g_, o_ = pre[:, :H], pre[:, H:2 * H], pre[:, 2 * H:3 * H], pre[:, 3 * H:]
                c = torch.sigmoid(f_) * c + torch.sigmoid(i_) * torch.tanh(g_)
                return torch.sigmoid(o_) * torch.tanh(c), c
            h0, c0 = cell(G[z, t][:, col] + h0 @ wt[s, 0], c0)
            h1, c1 = cell(b1[s] + h0 @ wt[s, 1] + h1 @ wt[s, 2], c1)
            hs[run, t] = h1
        st[run, 0, 0], st[run, 0, 1], st[run, 1, 0], st[run, 1, 1] = h0, c0, h1, c1
    out = torch.stack((hs[0] - hs[3], hs[2] + hs[1]), dim=-1)            # [k, B, H, 2]
    return out, st


def _lstm_gpu(wt, b1, G, state, H, B, steps):
    _, _, ops, L, _ = _mods()
    wt_d, b1_d = wt.cuda().contiguous(), b1.cuda().contiguous()
    st = state.cuda().contiguous().clone()
    outs, t0 = [], 0
    for k in steps:
        Gk = G[:, t0:t0 + k].contiguous().cuda()
        out = ops.Planar.empty(H, 1, B, k, k + 1, "cuda", zero=True)
        hstep = torch.empty(int(L.lib().idv_stream_clstm_wide_hstep_floats(H, B, k)), device="cuda")
        L.call("idv_stream_clstm_wide", L.p(Gk), L.p(wt_d), L.p(b1_d), L.p(st), L.p(hstep), out.ptr(), L.i(H), L.i(B), L.i(k),
               L.i(k + 1), L.i(out.Jp), L.stream_ptr())
        outs.append(out.channel_slice(0, H).cpu())                       # [B, k, H, 2]
        t0 += k
    return torch.cat(outs, dim=1).permute(1, 0, 2, 3).contiguous(), st.cpu()


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("H", [48, 96])
def test_wide_lstm_entry_across_pushes(H, B):
    k = 5
    wt, b1, G, state = _lstm_case(H, B, k, 100 + H + B)
    one, st_one = _lstm_gpu(wt, b1, G, state, H, B, [5])
    for steps in ([2, 3], [1] * 5):
        got, st = _lstm_gpu(wt, b1, G, state, H, B, steps)
        assert torch.equal(got, one) and torch.equal(st, st_one), steps
    want, st_want = _lstm_cpu(wt, b1, G, state, H, B, k)
    print(f"wide LSTM H {H} B {B}: out relerr {relerr(one, want):.3e}, state relerr {relerr(st_one, st_want):.3e}")
    assert relerr(one, want) < 2e-5 and relerr(st_one, st_want) < 2e-5
    if B > 1:                                        # stream 0 does not see stream 1's input
        G2 = G.clone()
        G2[:, :, 1] = torch.randn(2, k, 8 * H, generator=torch.Generator().manual_seed(1))
        other, st2 = _lstm_gpu(wt, b1, G2, state, H, B, [5])
        assert torch.equal(other[:, 0], one[:, 0]) and not torch.equal(other[:, 1], one[:, 1])
        assert torch.equal(st2[:, :, :, 0], st_one[:, :, :, 0])
        if B > 8:                                    # nor does the stream past the tile of 8
            assert torch.equal(other[:, 8], one[:, 8])


def test_wide_lstm_entry_full_width():
    H, B, k = 768, 2, 2
    wt, b1, G, state = _lstm_case(H, B, k, 7)
    one, st_one = _lstm_gpu(wt, b1, G, state, H, B, [2])
    got, st = _lstm_gpu(wt, b1, G, state, H, B, [1, 1])
    assert torch.equal(got, one) and torch.equal(st, st_one)
    want, st_want = _lstm_cpu(wt, b1, G, state, H, B, k)
    print(f"wide LSTM H 768: out relerr {relerr(one, want):.3e}, state relerr {relerr(st_one, st_want):.3e}")
    assert relerr(one, want) < 2e-5 and relerr(st_one, st_want) < 2e-5


# ----------------------------------------------------------------------------------------------------- 3. the repeat entry
@pytest.mark.parametrize("k", [1, 4])
def test_repeat_entry(k):
    _, _, ops, L, _ = _mods()
    C, F, B, ns = 3, 5, 3, 2
    g = torch.Generator().manual_seed(k)
    x5 = torch.randn(B, C, F, k, 2, generator=g)
    hist = torch.randn(2, C, F, B, generator=g)
    src = ops.Planar.from_tensor5(x5.cuda(), k + 1)
    dst = ops.Planar.empty(C, F, B * ns, k, k + 1, "cuda", zero=True)
    hn = torch.zeros(2 * C * F * B * ns, device="cuda")
    L.call("idv_stream_repeat", src.ptr(), L.p(hist.cuda()), L.i(C), L.i(F), L.i(B), L.i(ns), L.i(k), L.i(k + 1), L.i(src.Jp),
           dst.ptr(), L.p(hn), L.i(dst.Jp), L.stream_ptr())
    assert torch.equal(dst.tensor5().cpu(), x5.repeat_interleave(ns, dim=0))
    assert torch.equal(hn.cpu().reshape(2, C, F, B * ns), hist.repeat_interleave(ns, dim=3))
    assert float(dst.planes()[..., 0].abs().max()) == 0.0              # the guard columns stay as they were


# -------------------------------------------------------------------------------------------------- 4. chunk invariance
def _random_sizes(L, seed):
    rng = random.Random(seed)
    out, left = [], L
    while left:
        n = min(left, rng.choice([0, 0, 1, 13, 99, 100, 250, 777]))
        out.append(n)
        left -= n
    return out


def _offline_and_oracle(enc, dec, np_, st, x, latent, latent_num, zdim, ns, recon):
    """(inference.enhance_vae, CPU oracle) with st's draws in the chosen latent's slots and randn in the other's."""
    inf = _mods()[4]
    B, L = x.shape
    T = 1 + L // HOP
    own = st.eps(0, T)
    g = torch.Generator().manual_seed(99)
    other = tuple(torch.randn(B, ns, T, zdim, generator=g).cuda() for _ in range(2))
    if latent_num == 1:
        eps = own
    else:
        eps = own + other if latent == "speech" else other + own
    off = inf.enhance_vae(enc, dec, x, eps=eps, latent=latent)
    sd_e = {k: v.cpu() for k, v in enc.state_dict().items()}
    sd_d = {k: v.cpu() for k, v in dec.state_dict().items()}
    r = O.vae_encoder_forward(x.cpu(), sd_e, np_, True, zdim, NFFT, HOP, WIN, ns, latent_num, [e.cpu() for e in eps])
    rec, _ = O.vae_decoder_forward(r["stft_x"], r[f"z_{latent}"], r["skiper"], r["C"], r["F"], sd_d, np_, True, ns, NFFT, HOP, WIN,
                                   recon, SKIP, pad="sig")
    return off, rec.view(B, ns, -1).mean(1)


def test_chunk_invariance_bit_identical():
    _, S, _, _, _ = _mods()
    zdim, ns, B, L = 16, 2, 3, 2345
    enc, dec, np_ = _pair(4, zdim, ns, 2)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, L, generator=g) * 0.1).cuda()
    st = S.StreamingVAE(enc, dec, batch=B, seed=3, frames_per_launch=8)
    assert st.H == 96 and st.cap == 8
    chunkings = {"whole": [L], "1then100": [1] * 700 + [100] * ((L - 700) // 100) + [(L - 700) % 100],
                 "hop": _hops(L), "37": _hops(L, 37), "random": _random_sizes(L, 3), "over_cap": [1500, L - 1500]}
    ys = {k: _stream(st, x, v, check_counts=True) for k, v in chunkings.items()}
    base = ys["whole"]
    for k, y in ys.items():
        assert torch.equal(y, base), k
    off, orc = _offline_and_oracle(enc, dec, np_, st, x, "speech", 2, zdim, ns, "mask")
    assert base.shape == off.shape == orc.shape == (B, HOP * (L // HOP))
    print(f"StreamingVAE vs enhance_vae {relerr(base, off):.3e}, vs CPU oracle {relerr(base, orc):.3e}")
    assert relerr(base, off) < TOL and relerr(base, orc) < TOL
    # average=False returns the ns waveforms of stream b in rows b*ns .. b*ns+ns-1
    rows = _stream(S.StreamingVAE(enc, dec, batch=B, seed=3, frames_per_launch=8, average=False), x, _hops(L))
    assert rows.shape == (B * ns, base.shape[1]) and relerr(rows.view(B, ns, -1).mean(1), base) < 1e-6
    # another seed, other draws
    st.seed = 4
    assert not torch.equal(_stream(st, x, _hops(L)), base)


@pytest.mark.parametrize("latent,recon,latent_num", [("noise", "mask", 2), ("speech", "real_imag", 2), ("speech", "mask", 1)])
def test_other_latent_recon_and_width(latent, recon, latent_num):
    _, S, _, _, _ = _mods()
    zdim, ns, B, L = 16, 2, 3, 2345
    enc, dec, np_ = _pair(4, zdim, ns, latent_num, recon, seed=50)
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(B, L, generator=g) * 0.1).cuda()
    st = S.StreamingVAE(enc, dec, batch=B, seed=8, latent=latent, frames_per_launch=8)
    assert st.H == 48 * latent_num
    y = _stream(st, x, _hops(L), check_counts=True)
    off, orc = _offline_and_oracle(enc, dec, np_, st, x, latent, latent_num, zdim, ns, recon)
    assert y.shape == off.shape == orc.shape
    print(f"{latent} {recon} latent_num {latent_num}: vs enhance_vae {relerr(y, off):.3e}, vs CPU oracle {relerr(y, orc):.3e}")
    assert relerr(y, off) < TOL and relerr(y, orc) < TOL


def test_cvae_encoder_class():
    """pvae_dccrn_encoder_skip_prepare (one latent, 8-tuple offline) as the noisy encoder."""
    _, S, _, _, inf = _mods()
    zdim, ns, B, L = 16, 2, 2, 900
    enc, dec, _ = _pair(4, zdim, ns, 1, seed=60, skip_prepare=True)
    x = (torch.randn(B, L, generator=torch.Generator().manual_seed(7)) * 0.1).cuda()
    st = S.StreamingVAE(enc, dec, batch=B, seed=1)
    y = _stream(st, x, _hops(L))
    r = enc(x, train=False, eps=st.eps(0, 1 + L // HOP))
    rec, _ = dec(r[7], r[0], r[4], r[5], r[6], train=False, pad="sig")
    assert relerr(y, inf.mean_over_samples(rec, ns)) < TOL


# ---------------------------------------------------------------------------------------------------- 5. reference parity
def test_reference_parity(golden):
    _, S, _, _, _ = _mods()
    d = golden("vae_nsvae_mini_eval")
    base, seed, zdim, ns = int(d["base"]), int(d["seed"]), int(d["zdim"]), int(d["ns"])
    np_ = O.net_params(True, base)
    pm = _mods()[0]
    enc = load_synth(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2), seed + 2)
    dec = load_synth(pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP, False), seed + 3)
    x = torch.from_numpy(np.asarray(d["x"])).cuda()
    e0, e1 = (torch.from_numpy(np.asarray(d[f"eps{j}"])).cuda() for j in range(2))
    draws = lambda t0, k: (e0[:, :, t0:t0 + k], e1[:, :, t0:t0 + k])
    want = torch.from_numpy(np.asarray(d["recon"]))
    B = x.shape[0]
    y = _stream(S.StreamingVAE(enc, dec, batch=B, eps=draws, average=False), x, _hops(x.shape[1]))
    assert y.shape == want.shape
    print(f"StreamingVAE vs the reference's recon: {relerr(y, want):.3e}")
    assert relerr(y, want) < TOL
    ya = _stream(S.StreamingVAE(enc, dec, batch=B, eps=draws, average=True), x, _hops(x.shape[1]))
    assert relerr(ya, want.view(B, ns, -1).mean(1)) < TOL


# ------------------------------------------------------------------------------------- 6. engines, independence, reuse
def test_engines_independence_reuse():
    _, S, _, L, _ = _mods()
    zdim, ns, B, Lx = 16, 2, 3, 1234
    enc, dec, _ = _pair(4, zdim, ns, 2, seed=70)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(B, Lx, generator=g) * 0.1).cuda()
    sizes = _hops(Lx, 160)
    st = S.StreamingVAE(enc, dec, batch=B, seed=2)
    a = _stream(st, x, sizes)
    stm = S.StreamingVAE(enc, dec, batch=B, seed=2, conv="mfma")
    sup = L.lib().idv_stream_cconv_mfma_supported
    want = ["mfma" if sup(1 if cp.transposed else 0, cp.C0 + cp.C1, cp.Cout) == 1 else "valu" for cp in stm.enc + stm.dec]
    assert stm.conv_engines == want and "mfma" in want and st.conv_engines == ["valu"] * 12
    assert torch.equal(_stream(stm, x, sizes), a)
    # stream 1's input changes: streams 0 and 2 keep their bits
    x2 = x.clone()
    x2[1] = torch.randn(Lx, generator=g).cuda()
    b = _stream(st, x2, sizes)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])
    # after flush the streamer is as new
    x3 = (torch.randn(B, 1100, generator=g) * 0.1).cuda()
    again = _stream(st, x3, [250] * 4 + [100])
    fresh = _stream(S.StreamingVAE(enc, dec, batch=B, seed=2), x3, [250] * 4 + [100])
    assert torch.equal(again, fresh)


# ------------------------------------------------------------------------------------------------------ 7. full width once
def test_full_width():
    _, S, _, _, inf = _mods()
    zdim, ns, B, L = 128, 2, 1, 1600
    enc, dec, _ = _pair(32, zdim, ns, 2, seed=80)
    x = (torch.randn(B, L, generator=torch.Generator().manual_seed(10)) * 0.1).cuda()
    stm = S.StreamingVAE(enc, dec, batch=B, seed=5, conv="mfma")
    assert stm.conv_engines.count("mfma") == 11 and stm.conv_engines[-1] == "valu" and len(stm.conv_engines) == 12
    st = S.StreamingVAE(enc, dec, batch=B, seed=5)
    assert st.H == 768
    y = _stream(st, x, _hops(L), check_counts=True)
    T = 1 + L // HOP
    own = st.eps(0, T)
    other = tuple(torch.randn(B, ns, T, zdim, device="cuda") for _ in range(2))
    off = inf.enhance_vae(enc, dec, x, eps=own + other, latent="speech")
    assert y.shape == off.shape
    print(f"full width StreamingVAE vs enhance_vae: {relerr(y, off):.3e}")
    assert relerr(y, off) < TOL
    assert torch.equal(_stream(st, x, [L]), y)
