"""Streaming VAE sessions (streaming.StreamingVAESessions) on the MI355X: the three per-slot entries one by one against their
lock-step twins, and slots that start, receive samples and end on their own against the lock-step StreamingVAE, bit for bit, for
the same signal in the same slot."""
import functools
import importlib
import random

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


@functools.lru_cache(maxsize=None)
def _pair(base=4, zdim=16, ns=2, latent_num=2, recon="mask", seed=40):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    enc = pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, latent_num)
    dec = pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, recon, True, SKIP, False)
    return load_synth(enc, seed + 2), load_synth(dec, seed + 3)


def _signals(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(L, generator=g) * 0.1).cuda() for L in lengths]


def _lockstep(ref, slot, sig):
    """The signal whole in slot ``slot`` of the lock-step streamer ``ref`` (the other slots carry zeros), then flushed -> the
    rows of that slot, [1, m] (average=False: [ns, m])."""
    x = torch.zeros(ref.B, len(sig), device="cuda")
    x[slot] = sig
    y = torch.cat([ref.push(x), ref.flush()], dim=1)
    nrow = y.shape[0] // ref.B
    return y[slot * nrow:(slot + 1) * nrow]


def _serve(st, queues, starts, width, count_of, on_call=None):
    """Feeds ``queues[b]`` (the signals of slot b, one after the other, the first from call ``starts[b]``) through ``st`` with
    ``count_of(b, call, remaining)`` samples per call; a signal ends in the call that brings its last samples.  Every call's
    x[b, counts[b]:] is NaN.  Returns {(slot, index of the signal in its queue): output rows [1 or ns, samples]}."""
    B = st.B
    nrow = 1 if st.average else st.ns
    queues = [list(q) for q in queues]
    cur, pos, idx = [None] * B, [0] * B, [-1] * B
    outs = {}
    ci = 0
    while any(queues) or any(c is not None for c in cur):
        x = torch.full((B, width), float("nan"), device="cuda")
        counts, end = [0] * B, []
        for b in range(B):
            if cur[b] is None and queues[b] and ci >= starts[b]:
                cur[b], pos[b], idx[b] = queues[b].pop(0), 0, idx[b] + 1
            if cur[b] is None:
                continue
            n = min(count_of(b, ci, len(cur[b]) - pos[b]), len(cur[b]) - pos[b], width)
            x[b, :n] = cur[b][pos[b]:pos[b] + n]
            counts[b], pos[b] = n, pos[b] + n
            if pos[b] == len(cur[b]):
                end.append(b)
        assert st.positions == [pos[b] - counts[b] if cur[b] is not None else 0 for b in range(B)]
        y, m = st.push(x, counts, end)
        assert y.shape == (B * nrow, max(m)) and bool(torch.isfinite(y).all())
        for b in range(B):
            assert not bool(y[b * nrow:(b + 1) * nrow, m[b]:].any())
            if cur[b] is not None:
                outs.setdefault((b, idx[b]), []).append(y[b * nrow:(b + 1) * nrow, :m[b]])
            else:
                assert m[b] == 0
        for b in end:
            cur[b] = None
        if on_call is not None:
            on_call(ci, cur, pos)
        ci += 1
    return {k: torch.cat(v, dim=1) for k, v in outs.items()}


def _rows(S, B, **fields):
    t = torch.zeros(B, S.NF, dtype=torch.int64)
    for name, v in fields.items():
        t[:, S.ROW_FIELDS.index(name)] = torch.tensor(v, dtype=torch.int64)
    return t


# ------------------------------------------------------------------------------------------------ 1. the wide LSTM rows entry
def test_wide_lstm_rows_entry_across_two_calls():
    """B = 9 is one past a stream tile.  Per slot, the columns < k_b and the final h / c equal idv_stream_clstm_wide run on that
    slot's G alone with k_b steps; hstep is NaN before each call, so an idle stream's unwritten rows reaching anything shows."""
    _, S, ops, L, _ = _mods()
    H, B, KL = 48, 9, 5
    ks = [[3, 0, 5, 1, 5, 0, 2, 4, 1], [0, 2, 1, 5, 0, 3, 5, 0, 4]]
    g = torch.Generator().manual_seed(77)
    sc = 1.0 / H ** 0.5
    wt = ((torch.rand(2, 3, H, 4 * H, generator=g) * 2 - 1) * sc).cuda()
    b1 = ((torch.rand(2, 4 * H, generator=g) * 2 - 1) * sc).cuda()
    state = (torch.randn(4, 2, 2, B, H, generator=g) * 0.5).cuda()               # [run][layer][h | c][B][H]
    want_state = state.clone()
    nh = int(L.lib().idv_stream_clstm_wide_hstep_floats(H, B, KL))
    for call in range(2):
        G = torch.randn(2, KL, B, 8 * H, generator=g).cuda()
        rows = _rows(S, B, k=ks[call]).cuda()
        out = ops.Planar.empty(H, 1, B, KL, KL + 1, "cuda", zero=False)
        out.buf.fill_(float("nan"))
        hstep = torch.full((nh,), float("nan"), device="cuda")
        before = state.clone()
        L.call("idv_stream_clstm_wide_rows", L.p(G), L.p(wt), L.p(b1), L.p(state), L.p(hstep), out.ptr(), L.i(H), L.i(B), L.i(KL),
               L.i(KL + 1), L.i(out.Jp), L.p(rows), L.stream_ptr())
        got = out.channel_slice(0, H)                                            # [B, KL, H, 2]
        for b, kb in enumerate(ks[call]):
            assert not bool(got[b, kb:].any()), (call, b)                        # zeros, and no NaN, from column k_b on
            if kb == 0:
                assert torch.equal(state[:, :, :, b].view(torch.int32), before[:, :, :, b].view(torch.int32)), (call, b)
                continue
            Gb = G[:, :kb, b:b + 1].contiguous()
            stb = want_state[:, :, :, b:b + 1].contiguous()
            ob = ops.Planar.empty(H, 1, 1, kb, kb + 1, "cuda", zero=True)
            hb = torch.empty(int(L.lib().idv_stream_clstm_wide_hstep_floats(H, 1, kb)), device="cuda")
            L.call("idv_stream_clstm_wide", L.p(Gb), L.p(wt), L.p(b1), L.p(stb), L.p(hb), ob.ptr(), L.i(H), L.i(1), L.i(kb),
                   L.i(kb + 1), L.i(ob.Jp), L.stream_ptr())
            assert torch.equal(got[b, :kb], ob.channel_slice(0, H)[0]), (call, b)
            want_state[:, :, :, b] = stb[:, :, :, 0]
        assert torch.equal(state, want_state), call
    with pytest.raises(L.IdvError):
        L.call("idv_stream_clstm_wide_rows", L.p(G), L.p(wt), L.p(b1), L.p(state), L.p(hstep), out.ptr(), L.i(H), L.i(B), L.i(KL),
               L.i(KL + 1), L.i(out.Jp), L.p(None), L.stream_ptr())


# ------------------------------------------------------------------------------------------------------- 2. the eps rows entry
def test_eps_rows_entry():
    _, S, _, L, _ = _mods()
    B, ns, zdim, KL, seed = 3, 2, 16, 4, 0x1234567890ABCDEF >> 1
    t0, ks = [0, 7, 2 ** 32 + 1], [4, 0, 2]
    rows = _rows(S, B, t0=t0, k=ks).cuda()
    got = torch.full((2, B, ns, KL, zdim), float("nan"), device="cuda")
    L.call("idv_stream_eps_rows", L.ll(seed), L.p(rows), L.i(B), L.i(ns), L.i(zdim), L.i(KL), L.p(got[0]), L.p(got[1]), L.stream_ptr())
    for b in range(B):
        assert not bool(got[:, b, :, ks[b]:].any()), b
        if ks[b] == 0:
            continue
        want = torch.empty(2, B, ns, ks[b], zdim, device="cuda")
        L.call("idv_stream_eps", L.ll(seed), L.ll(t0[b]), L.i(ks[b]), L.i(B), L.i(ns), L.i(zdim), L.p(want[0]), L.p(want[1]),
               L.stream_ptr())
        assert torch.equal(got[:, b, :, :ks[b]], want[:, b]), b
        assert bool(want[:, b].any())


# ---------------------------------------------------------------------------------------------------- 3. the repeat rows entry
def test_repeat_rows_entry():
    _, S, ops, L, _ = _mods()
    C, F, B, ns, KL = 3, 5, 4, 2, 4
    ks, par = [4, 0, 2, 1], [0, 1, 1, 0]
    SENT = 7.0
    g = torch.Generator().manual_seed(3)
    x5 = torch.randn(B, C, F, KL, 2, generator=g)
    hist = torch.randn(2, 2 * C * F, B, generator=g).cuda()                       # [parity][2][C][F][B]
    src = ops.Planar.from_tensor5(x5.cuda(), KL + 1)
    dst = ops.Planar.empty(C, F, B * ns, KL, KL + 1, "cuda", zero=False)
    dst.buf.fill_(SENT)
    hn = torch.full((2, 2 * C * F, B * ns), SENT, device="cuda")
    want = ops.Planar(dst.buf.clone(), C, F, B * ns, KL, KL + 1, dst.Jp)
    want_hn = hn.clone()
    rep = x5.cuda().repeat_interleave(ns, dim=0)
    for b in range(B):
        if ks[b] == 0:
            continue
        for s in range(ns):
            want.tensor5()[b * ns + s, :, :, :ks[b]] = rep[b * ns + s, :, :, :ks[b]]
            want_hn[par[b], :, b * ns + s] = hist[par[b], :, b]
    rows = _rows(S, B, k=ks, parity=par).cuda()
    L.call("idv_stream_repeat_rows", src.ptr(), L.p(hist), L.i(C), L.i(F), L.i(B), L.i(ns), L.i(KL), L.i(KL + 1), L.i(src.Jp),
           L.p(rows), dst.ptr(), L.p(hn), L.i(dst.Jp), L.stream_ptr())
    assert torch.equal(dst.buf, want.buf)                 # the copies in the right place, the sentinel everywhere else
    assert torch.equal(hn, want_hn)
    assert int((dst.buf != SENT).sum()) == 2 * C * F * ns * sum(ks)
    assert int((hn != SENT).sum()) == 2 * C * F * ns * sum(1 for k in ks if k)


# --------------------------------------------------------------------------------------------------------- 4. the sessions
def _staggered(st, seed=4):
    """The schedule of tests/test_gpu_stream_sessions.py: queues [[a], [b1, b2], [c]], starts at calls 0, 1, 3."""
    sigs = _signals([1234, 777, 401, 2345], 31)
    a, b1, b2, c = sigs
    rng = random.Random(seed)
    got = _serve(st, [[a], [b1, b2], [c]], [0, 1, 3], 300, lambda b, ci, left: rng.choice([0, 0, 1, 37, 100, 250, 300]))
    assert st.positions == [0, 0, 0]
    return got, {(0, 0): a, (1, 0): b1, (1, 1): b2, (2, 0): c}


def test_staggered_sessions_equal_the_lockstep_streamer_and_offline():
    _, S, _, _, inf = _mods()
    zdim, ns = 16, 2
    enc, dec = _pair()
    st = S.StreamingVAESessions(enc, dec, slots=3, seed=3, frames_per_launch=8)
    assert st.H == 96 and st.cap == 8
    got, sigs = _staggered(st)
    ref = S.StreamingVAE(enc, dec, batch=3, seed=3, frames_per_launch=8)
    g = torch.Generator().manual_seed(99)
    for (slot, j), sig in sigs.items():
        want = _lockstep(ref, slot, sig)
        assert got[(slot, j)].shape == want.shape == (1, HOP * (len(sig) // HOP))
        assert torch.equal(got[(slot, j)], want), (slot, j)
        T = 1 + len(sig) // HOP
        own = tuple(e[slot:slot + 1] for e in st.eps(0, T))
        other = tuple(torch.randn(1, ns, T, zdim, generator=g).cuda() for _ in range(2))
        off = inf.enhance_vae(enc, dec, sig[None], eps=own + other, latent="speech")
        err = relerr(got[(slot, j)], off)
        print(f"slot {slot} signal {j} ({len(sig)} samples) vs enhance_vae: {err:.3e}")
        assert off.shape == want.shape and err < TOL, (slot, j)
    # the draws are StreamingVAE's, and the seed does not move in mid-signal
    assert all(torch.equal(u, v) for u, v in zip(st.eps(5, 3), ref.eps(5, 3)))
    st.push(torch.zeros(3, 50, device="cuda"), [50, 0, 0])
    with pytest.raises(ValueError, match="between signals"):
        st.seed = 4
    st.drop([0])
    st.seed = 4
    assert st.seed == 4 and st.positions == [0, 0, 0]


def test_nine_slots_cross_the_lstm_stream_tile():
    """9 slots: the wide LSTM runs 8 streams per workgroup.  Slots 7 and 8 complete different frame counts in the same call (300
    and 100 samples), slot 3 idles for calls 3 .. 6 in the middle of its signal."""
    _, S, _, _, _ = _mods()
    enc, dec = _pair()
    lengths = [900, 650, 1000, 1100, 800, 257, 950, 1200, 700]
    sigs = _signals(lengths, 32)
    steps = [100, 250, 37, 300, 1, 163]

    def count_of(b, ci, left):
        if b == 3 and 3 <= ci <= 6:
            return 0
        return {7: 300, 8: 100}.get(b, steps[(b + ci) % len(steps)])

    st = S.StreamingVAESessions(enc, dec, slots=9, seed=1, frames_per_launch=8)
    got = _serve(st, [[s] for s in sigs], [0] * 9, 300, count_of)
    ref = S.StreamingVAE(enc, dec, batch=9, seed=1, frames_per_launch=8)
    for b, sig in enumerate(sigs):
        assert torch.equal(got[(b, 0)], _lockstep(ref, b, sig)), b


def test_counts_none_equals_lockstep_push_call_by_call():
    _, S, _, _, _ = _mods()
    enc, dec = _pair()
    x = (torch.randn(3, 1500, generator=torch.Generator().manual_seed(33)) * 0.1).cuda()
    st = S.StreamingVAESessions(enc, dec, slots=3, seed=2, frames_per_launch=8)
    ref = S.StreamingVAE(enc, dec, batch=3, seed=2, frames_per_launch=8)
    n = 0
    for sz in [700, 100, 37, 0, 463, 100, 100]:
        y, mm = st.push(x[:, n:n + sz])
        want = ref.push(x[:, n:n + sz])
        n += sz
        assert mm == [want.shape[1]] * 3 and torch.equal(y, want), n
    assert st.positions == [1500] * 3
    y, mm = st.push(x[:, :0], end=[0, 1, 2])
    assert torch.equal(y, ref.flush()) and mm == [y.shape[1]] * 3 and st.positions == [0, 0, 0]
    with pytest.raises(ValueError, match="GPU tensor"):
        st.push(x[:, :10], counts=torch.tensor([1, 2, 3], device="cuda"))
    with pytest.raises(ValueError, match="0 .. 10"):
        st.push(x[:, :10], counts=[1, 2, 11])
    with pytest.raises(ValueError, match="n_fft/2"):
        st.push(x[:, :10], counts=[10, 0, 0], end=[0])
    assert st.positions == [0, 0, 0]


def test_drop_and_reuse():
    _, S, _, _, _ = _mods()
    enc, dec = _pair()
    a, b_old, b_new, c = _signals([1000, 900, 600, 1100], 34)
    st = S.StreamingVAESessions(enc, dec, slots=3, seed=5, frames_per_launch=8)

    def on_call(ci, cur, pos):
        if ci == 3:                                   # slot 1 is 400 samples into b_old: abandon it
            assert st.positions[1] == 400
            st.drop([1])
            assert st.positions[1] == 0
            cur[1] = None
    got = _serve(st, [[a], [b_old, b_new], [c]], [0, 0, 0], 100, lambda b, ci, left: 100, on_call)
    fresh = _serve(S.StreamingVAESessions(enc, dec, slots=3, seed=5, frames_per_launch=8), [[], [b_new], []], [0, 0, 0], 100,
                   lambda b, ci, left: 100)
    assert got[(1, 1)].shape == (1, 600) and torch.equal(got[(1, 1)], fresh[(1, 0)])
    assert got[(1, 0)].shape == (1, 100)              # what b_old returned before it was dropped
    ref = S.StreamingVAE(enc, dec, batch=3, seed=5, frames_per_launch=8)
    assert torch.equal(got[(0, 0)], _lockstep(ref, 0, a)) and torch.equal(got[(2, 0)], _lockstep(ref, 2, c))


def test_average_false_rows():
    _, S, _, _, _ = _mods()
    ns = 2
    enc, dec = _pair()
    rows, sigs = _staggered(S.StreamingVAESessions(enc, dec, slots=3, seed=3, frames_per_launch=8, average=False))
    mean, _ = _staggered(S.StreamingVAESessions(enc, dec, slots=3, seed=3, frames_per_launch=8))
    ref = S.StreamingVAE(enc, dec, batch=3, seed=3, frames_per_launch=8, average=False)
    for (slot, j), sig in sigs.items():
        want = _lockstep(ref, slot, sig)               # rows slot * ns .. slot * ns + ns - 1 of the lock-step streamer
        assert rows[(slot, j)].shape == want.shape == (ns, HOP * (len(sig) // HOP))
        assert torch.equal(rows[(slot, j)], want), (slot, j)
        assert not torch.equal(want[0], want[1])
        # the mean of two floats is exact up to the final rounding, whichever way it is formed
        assert torch.equal(rows[(slot, j)].double().mean(0).float()[None], mean[(slot, j)]), (slot, j)


@pytest.mark.parametrize("latent,recon,latent_num", [("noise", "mask", 2), ("speech", "real_imag", 2), ("speech", "mask", 1)])
def test_other_latent_recon_and_width(latent, recon, latent_num):
    _, S, _, _, _ = _mods()
    enc, dec = _pair(latent_num=latent_num, recon=recon, seed=50)
    st = S.StreamingVAESessions(enc, dec, slots=3, seed=8, latent=latent, frames_per_launch=8)
    assert st.H == 48 * latent_num
    got, sigs = _staggered(st, seed=6)
    ref = S.StreamingVAE(enc, dec, batch=3, seed=8, latent=latent, frames_per_launch=8)
    for (slot, j), sig in sigs.items():
        assert torch.equal(got[(slot, j)], _lockstep(ref, slot, sig)), (slot, j)


def test_mfma_engine_gives_the_bits_of_valu():
    _, S, _, _, _ = _mods()
    enc, dec = _pair()
    stm = S.StreamingVAESessions(enc, dec, slots=3, seed=3, frames_per_launch=8, conv="mfma")
    stv = S.StreamingVAESessions(enc, dec, slots=3, seed=3, frames_per_launch=8)
    assert "mfma" in stm.conv_engines and stv.conv_engines == ["valu"] * 12
    gm, sigs = _staggered(stm)
    gv, _ = _staggered(stv)
    ref = S.StreamingVAE(enc, dec, batch=3, seed=3, frames_per_launch=8, conv="mfma")
    for key, sig in sigs.items():
        assert torch.equal(gm[key], gv[key]), key
        assert torch.equal(gm[key], _lockstep(ref, key[0], sig)), key


# ------------------------------------------------------------------------------------------------------ 5. full width once
def test_full_width():
    """base 32, zdim 128, num_samples 3: H = 768, the widest LSTM the entry takes; two signals staggered by one call."""
    _, S, _, _, _ = _mods()
    enc, dec = _pair(32, 128, 3, 2, "mask", 80)
    sigs = _signals([1300, 900], 35)
    st = S.StreamingVAESessions(enc, dec, slots=2, seed=5)
    assert st.H == 768 and st.ns == 3
    steps = [300, 100, 250]
    got = _serve(st, [[sigs[0]], [sigs[1]]], [0, 1], 300, lambda b, ci, left: steps[(b + ci) % 3])
    assert st.positions == [0, 0]
    ref = S.StreamingVAE(enc, dec, batch=2, seed=5)
    for b, sig in enumerate(sigs):
        want = _lockstep(ref, b, sig)
        assert want.shape == (1, HOP * (len(sig) // HOP))
        assert torch.equal(got[(b, 0)], want), b
