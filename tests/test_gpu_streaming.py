"""Streaming enhancement (streaming.StreamingDCCRN) on the MI355X: parity with the reference and the offline path, chunk
invariance, stream independence, reuse after flush, and the new stream kernels one by one."""
import importlib
import random

import numpy as np
import pytest
import torch

from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.streaming"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _model(base, seed, recon="mask", skip=SKIP, mean=None, std=None):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, skip, recon, False, mean, std)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k not in ("data_mean", "data_std")}, seed)
    if mean is not None:
        sd["data_mean"], sd["data_std"] = mean, std
    m.load_state_dict(sd, strict=True)
    return m.cuda(), np_


def _stream(st, x, sizes, check_counts=False):
    outs, n = [], 0
    for m in sizes:
        y = st.push(x[:, n:n + m])
        n += m
        if check_counts:
            k = 0 if n <= WIN // 2 else (n - WIN // 2) // HOP + 1
            assert sum(o.shape[1] for o in outs) + y.shape[1] == max(0, HOP * k - WIN // 2)
        outs.append(y)
    assert n == x.shape[1]
    outs.append(st.flush())
    return torch.cat(outs, dim=1)


def test_reference_parity_full_width(golden):
    _, S, _, _ = _mods()
    d = golden("dccrn_full_eval")
    m, _ = _model(int(d["base"]), int(d["seed"]))
    x = torch.from_numpy(np.asarray(d["x"])).cuda()
    st = S.StreamingDCCRN(m, batch=x.shape[0])
    y = _stream(st, x, [160] * (x.shape[1] // 160) + ([x.shape[1] % 160] if x.shape[1] % 160 else []))
    want = torch.from_numpy(np.asarray(d["clean"]))
    assert y.shape == want.shape and y.shape[1] == 64000
    assert relerr(y, want) < TOL


def test_datanorm_mask_and_real_imag(golden):
    _, S, _, _ = _mods()
    d = golden("dccrn_datanorm_mini")
    mean, std = torch.from_numpy(np.asarray(d["data_mean"])), torch.from_numpy(np.asarray(d["data_std"]))
    x = torch.from_numpy(np.asarray(d["x"])).cuda()
    for rt in ("mask", "real_imag"):
        m, _ = _model(4, int(d["seed"]), rt, mean=mean, std=std)
        st = S.StreamingDCCRN(m, batch=x.shape[0])
        y = _stream(st, x, [100] * (x.shape[1] // 100) + [x.shape[1] % 100])
        want = torch.from_numpy(np.asarray(d[f"clean_{rt}"]))
        assert y.shape == want.shape and relerr(y, want) < TOL, rt


def _random_sizes(L, seed):
    rng = random.Random(seed)
    out, left = [], L
    while left:
        n = min(left, rng.choice([0, 0, 1, 13, 99, 100, 250, 777]))
        out.append(n)
        left -= n
    return out


def test_chunk_invariance_bit_identical():
    _, S, _, _ = _mods()
    m, np_ = _model(4, 11)
    B, L = 3, 2345
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, L, generator=g) * 0.1).cuda()
    st = S.StreamingDCCRN(m, batch=B, frames_per_launch=8)
    chunkings = {"whole": [L], "1then100": [1] * 700 + [100] * ((L - 700) // 100) + [(L - 700) % 100],
                 "hop": [HOP] * (L // HOP) + [L % HOP], "37": [37] * (L // 37) + [L % 37], "random": _random_sizes(L, 3),
                 "over_cap": [1500, L - 1500]}
    ys = {k: _stream(st, x, v, check_counts=True) for k, v in chunkings.items()}
    base = ys["whole"]
    for k, y in ys.items():
        assert torch.equal(y, base), k
    with torch.no_grad():
        off = m(x, train=False)[0]
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    o = O.dccrn_forward(x.cpu(), sd, np_, True, NFFT, HOP, WIN, SKIP)[0]
    assert base.shape == off.shape == o.shape
    assert relerr(base, off) < TOL and relerr(base, o) < TOL


def test_stream_independence_and_batch_sizes():
    _, S, _, _ = _mods()
    m, _ = _model(4, 12)
    L = 1234
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(3, L, generator=g) * 0.1).cuda()
    st = S.StreamingDCCRN(m, batch=3)
    a = _stream(st, x, [160] * (L // 160) + [L % 160])
    x2 = x.clone()
    x2[1] = torch.randn(L, generator=g).cuda()
    b = _stream(st, x2, [160] * (L // 160) + [L % 160])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])
    for B in (1, 64, 300):
        xb = (torch.randn(B, 700, generator=g) * 0.1).cuda()
        stb = S.StreamingDCCRN(m, batch=B)
        y = _stream(stb, xb, [100] * 7)
        with torch.no_grad():
            off = m(xb, train=False)[0]
        assert y.shape == off.shape and relerr(y, off) < TOL, B


def test_reuse_after_flush():
    _, S, _, _ = _mods()
    m, _ = _model(4, 13)
    g = torch.Generator().manual_seed(7)
    x1 = (torch.randn(2, 900, generator=g) * 0.1).cuda()
    x2 = (torch.randn(2, 1100, generator=g) * 0.1).cuda()
    st = S.StreamingDCCRN(m, batch=2)
    _stream(st, x1, [300, 300, 300])
    again = _stream(st, x2, [250] * 4 + [100])
    fresh = _stream(S.StreamingDCCRN(m, batch=2), x2, [250] * 4 + [100])
    assert torch.equal(again, fresh)


def _hist(x5):
    """[B, C, F, 2] -> hist [2][C][F][B]"""
    return x5.permute(3, 1, 2, 0).contiguous().reshape(-1)


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("k", [1, 4])
def test_conv_entries_every_block_shape(B, k):
    _, S, ops, L = _mods()
    g = torch.Generator().manual_seed(B * 10 + k)
    for skip in (SKIP, []):
        m, np_ = _model(4, 14, skip=skip)
        st = S.StreamingDCCRN(m, batch=B)
        sd = {kk: v.cpu() for kk, v in m.state_dict().items()}
        blocks = [("enc", e, cp) for e, cp in enumerate(st.enc)] + [("dec", d, cp) for d, cp in enumerate(st.dec)]
        for kind, idx, cp in blocks:
            if kind == "enc" and skip == []:
                continue
            cin = cp.C0 + cp.C1
            x5 = torch.randn(B, cin, cp.Fin, k + 1, 2, generator=g)
            if kind == "enc":
                want = O.encoder_block(x5, sd, f"std_DCCRN.encoders.{idx}.", np_, idx, True, False)
            else:
                want = O.decoder_block(x5, sd, f"std_DCCRN.decoders.{idx}.", np_, idx, True, False)
            want = want[:, :, :, 1:]
            xs = [x5[:, :cp.C0].cuda()] + ([x5[:, cp.C0:].cuda()] if cp.C1 else [])
            srcs = [ops.Planar.from_tensor5(v[:, :, :, 1:].contiguous(), k + 1) for v in xs]
            hists = [_hist(v[:, :, :, 0]) for v in xs]
            out = ops.Planar.empty(cp.Cout, cp.Fout, B, k, k + 1, "cuda", zero=True)
            hout = torch.empty(2 * cp.Cout * cp.Fout * B, device="cuda")
            x0h = torch.empty(2 * cp.C0 * cp.Fin * B, device="cuda")
            Jp = out.Jp
            st._conv_call(cp, srcs[0].ptr(), hists[0], srcs[1].ptr() if cp.C1 else None, hists[1] if cp.C1 else None, out.ptr(),
                          hout, L.p(x0h), B, k, k + 1, Jp)
            got = out.tensor5().cpu()
            assert relerr(got, want) < 2e-5, (kind, idx, skip == [])
            assert torch.equal(hout.cpu(), _hist(got[:, :, :, -1]).cpu()), (kind, idx)
            assert torch.equal(x0h.cpu(), _hist(xs[0][:, :, :, -1].cpu())), (kind, idx)


def test_lstm_entry_across_pushes():
    _, S, ops, L = _mods()
    m, np_ = _model(4, 15)
    B, steps = 5, [2, 1, 3]
    T = sum(steps)
    st = S.StreamingDCCRN(m, batch=B)
    H, K = st.H, st.K
    g = torch.Generator().manual_seed(8)
    x = torch.randn(T, B, K, 2, generator=g)
    sd = {kk: v.cpu() for kk, v in m.state_dict().items()}
    want = O.complex_lstm(x, sd, "std_DCCRN.lstms.0.", 2)                   # [T, B, H, 2]
    state = torch.zeros(4 * 4 * B * H, device="cuda")
    t0, got = 0, []
    for k in steps:
        xin = ops.Planar.from_tensor5(x[t0:t0 + k].permute(1, 2, 0, 3).unsqueeze(2).contiguous().cuda(), k + 1)
        G = torch.empty(2 * k * B * 8 * H, device="cuda")
        for z in range(2):
            ops.pw_gemm(xin.ptr(z * K), K, st.lstm_ih[0], st.lstm_ih[1], 8 * H, B, k + 1, xin.Jp, k,
                        L._P(G.data_ptr() + 4 * z * k * B * 8 * H), swap=True, ldo=8 * H)
        out = ops.Planar.empty(H, 1, B, k, k + 1, "cuda", zero=True)
        hout = torch.empty(4 * k * B * H, device="cuda")
        L.call("idv_stream_clstm", L.p(G), L.p(st.lstm_wt), L.p(st.lstm_b1), L.p(state), L.p(hout), out.ptr(), L.i(H), L.i(B), L.i(k),
               L.i(k + 1), L.i(out.Jp), L.stream_ptr())
        got.append(out.channel_slice(0, H).cpu())                          # [B, k, H, 2]
        t0 += k
    got = torch.cat(got, dim=1).permute(1, 0, 2, 3)
    assert relerr(got, want) < 2e-5


@pytest.mark.parametrize("k", [1, 4])
def test_conv_entries_full_width_shapes(k):
    """Every full-width block shape (Cin up to 512 with the skip, several 16-channel tiles, the deepest K split at B = 1)."""
    _, S, ops, L = _mods()
    B = 1
    g = torch.Generator().manual_seed(100 + k)
    m, np_ = _model(32, 16)
    st = S.StreamingDCCRN(m, batch=B)
    sd = {kk: v.cpu() for kk, v in m.state_dict().items()}
    assert max(cp.nsplit for cp in st.enc + st.dec) > 16
    for kind, idx, cp in [("enc", e, cp) for e, cp in enumerate(st.enc)] + [("dec", d, cp) for d, cp in enumerate(st.dec)]:
        x5 = torch.randn(B, cp.C0 + cp.C1, cp.Fin, k + 1, 2, generator=g)
        if kind == "enc":
            want = O.encoder_block(x5, sd, f"std_DCCRN.encoders.{idx}.", np_, idx, True, False)
        else:
            want = O.decoder_block(x5, sd, f"std_DCCRN.decoders.{idx}.", np_, idx, True, False)
        xs = [x5[:, :cp.C0].cuda()] + ([x5[:, cp.C0:].cuda()] if cp.C1 else [])
        srcs = [ops.Planar.from_tensor5(v[:, :, :, 1:].contiguous(), k + 1) for v in xs]
        hists = [_hist(v[:, :, :, 0]) for v in xs]
        out = ops.Planar.empty(cp.Cout, cp.Fout, B, k, k + 1, "cuda", zero=True)
        hout = torch.empty(2 * cp.Cout * cp.Fout * B, device="cuda")
        st._conv_call(cp, srcs[0].ptr(), hists[0], srcs[1].ptr() if cp.C1 else None, hists[1] if cp.C1 else None, out.ptr(), hout,
                      L.p(None), B, k, k + 1, out.Jp)
        got = out.tensor5().cpu()
        assert relerr(got, want[:, :, :, 1:]) < 2e-5, (kind, idx, cp.nsplit)
        assert torch.equal(hout.cpu(), _hist(got[:, :, :, -1]).cpu()), (kind, idx)


def test_far_stream_position_is_bit_identical():
    """Nothing but indices depends on where a stream is: moving a stream's position on by a multiple of the input ring and the
    hop (lcm(512, 100) samples) leaves every output bit-identical, here about 4.4 hours into the stream with no flush before."""
    _, S, _, _ = _mods()
    m, _ = _model(4, 17)
    B, L = 2, 3000
    g = torch.Generator().manual_seed(10)
    x = (torch.randn(B, L, generator=g) * 0.1).cuda()
    sizes = [700, 100, 37, 463, 100, 1000, 600]
    a = S.StreamingDCCRN(m, batch=B)
    b = S.StreamingDCCRN(m, batch=B)
    D = 12800 * 20000                       # 256e6 samples, 2.56e6 frames
    ya, yb, n = [], [], 0
    for j, sz in enumerate(sizes):
        if j == 1:                          # b: the same state, the stream D samples further on
            pl = b.plan
            pl.n, pl.k, pl.emitted = pl.n + D, pl.k + D // HOP, pl.emitted + D
        ya.append(a.push(x[:, n:n + sz]))
        yb.append(b.push(x[:, n:n + sz]))
        n += sz
    ya.append(a.flush())
    yb.append(b.flush())
    for u, v in zip(ya, yb):
        assert torch.equal(u, v)


def test_ola_entry_envelope_at_large_position():
    """idv_stream_ola far into a stream: the same frames give the same samples at frame 7 and at frame 3e9 / hop, and both
    match a float64 overlap-add divided by the envelope."""
    _, S, _, L = _mods()
    B, k = 3, 5
    pl = S.StreamPlan(NFFT, HOP, WIN)
    g = torch.Generator().manual_seed(11)
    fr = torch.randn(WIN, B, k + 1, generator=g)
    fr[:, :, 0] = 0
    frames = fr.reshape(WIN, B * (k + 1)).cuda().contiguous()
    carry = torch.randn(B, pl.carry_cap, generator=g)
    half, left = NFFT // 2, (NFFT - WIN) // 2
    w = torch.hann_window(WIN, periodic=True, dtype=torch.float64)
    outs = []
    for t0 in (7, 3_000_000_000 // HOP):
        e0 = HOP * t0 + pl.lo                           # emitted before: everything final after frames 0 .. t0-1
        cin = HOP * (t0 - 1) + left + WIN - (half + e0)
        e1 = HOP * (t0 + k) + pl.lo
        p_end = HOP * (t0 + k - 1) + left + WIN
        y = torch.zeros(B, e1 - e0, device="cuda")
        cout = torch.zeros(B, pl.carry_cap, device="cuda")
        L.call("idv_stream_ola", L.p(frames), L.i(k + 1), L.i(B * (k + 1)), L.p(carry.cuda()), L.i(cin), L.p(cout),
               L.i(pl.carry_cap), L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.ll(t0), L.i(k), L.ll(-1), L.ll(e0), L.ll(e1), L.ll(p_end),
               L.p(y), L.i(e1 - e0), L.ll(0), L.stream_ptr())
        outs.append(y.cpu())
        # float64: carry + frames, divided by the sum of squared windows of the frames that cover each position
        P = torch.arange(half + e0, half + e1)
        acc = torch.zeros(B, len(P), dtype=torch.float64)
        acc[:, :cin] = carry[:, :cin].double()
        env = torch.zeros(len(P), dtype=torch.float64)
        for t in range(t0 - 4, t0 + k):
            i = P - HOP * t - left
            ok = (i >= 0) & (i < WIN)
            env[ok] += w[i[ok]] ** 2
            if t >= t0:
                acc[:, ok] += fr[i[ok], :, 1 + t - t0].t().double()
        assert relerr(y, acc / env) < 1e-6
    assert torch.equal(outs[0], outs[1])
