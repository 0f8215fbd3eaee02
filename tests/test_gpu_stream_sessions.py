"""Streaming sessions (streaming.StreamingSessions) on the MI355X: slots that start, receive samples and end on their own give,
bit for bit, what the lock-step streamer gives for the same signal in the same slot; drop and reuse; the per-row entries one by
one against the lock-step entries."""
import importlib
import random

import pytest
import torch

from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4                      # the waveform tolerance of tests/test_gpu_streaming.py


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.streaming"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _model(base, seed, skip=SKIP):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, skip, "mask", False, None, None)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k not in ("data_mean", "data_std")}, seed)
    m.load_state_dict(sd, strict=True)
    return m.cuda(), np_


def _signals(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(L, generator=g) * 0.1).cuda() for L in lengths]


def _lockstep(ref, slot, sig):
    """The signal whole in slot ``slot`` of the lock-step streamer ``ref`` (the other slots carry zeros), then flushed."""
    x = torch.zeros(ref.B, len(sig), device="cuda")
    x[slot] = sig
    return torch.cat([ref.push(x), ref.flush()], dim=1)[slot]


def _serve(st, queues, starts, width, count_of, on_call=None):
    """Feeds ``queues[b]`` (the signals of slot b, one after the other, the first from call ``starts[b]``) through ``st`` with
    ``count_of(b, call, remaining)`` samples per call; a signal ends in the call that brings its last samples.  Every call's
    x[b, counts[b]:] is NaN.  Returns {(slot, index of the signal in its queue): output}."""
    B = st.B
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
        assert y.shape == (B, max(m)) and bool(torch.isfinite(y).all())
        for b in range(B):
            assert not bool(y[b, m[b]:].any())
            if cur[b] is not None:
                outs.setdefault((b, idx[b]), []).append(y[b, :m[b]])
            else:
                assert m[b] == 0
        for b in end:
            cur[b] = None
        if on_call is not None:
            on_call(ci, cur, pos)
        ci += 1
    return {k: torch.cat(v) for k, v in outs.items()}


def test_staggered_sessions_equal_the_lockstep_streamer():
    _, S, _, _ = _mods()
    m, np_ = _model(4, 21)
    a, b1, b2, c = _signals([1234, 777, 401, 2345], 31)
    rng = random.Random(4)
    st = S.StreamingSessions(m, slots=3, frames_per_launch=8)
    got = _serve(st, [[a], [b1, b2], [c]], [0, 1, 3], 300, lambda b, ci, left: rng.choice([0, 0, 1, 37, 100, 250, 300]))
    assert st.positions == [0, 0, 0]
    ref = S.StreamingDCCRN(m, batch=3, frames_per_launch=8)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    for (slot, j), sig in {(0, 0): a, (1, 0): b1, (1, 1): b2, (2, 0): c}.items():
        want = _lockstep(ref, slot, sig)
        assert got[(slot, j)].shape == want.shape == (HOP * (len(sig) // HOP),)
        assert torch.equal(got[(slot, j)], want), (slot, j)
        o = O.dccrn_forward(sig[None].cpu(), sd, np_, True, NFFT, HOP, WIN, SKIP)[0]
        assert relerr(got[(slot, j)][None], o) < TOL, (slot, j)


def test_nine_slots_cross_the_lstm_workgroup():
    """9 slots: the LSTM kernel runs 8 streams per workgroup.  Slots 7 and 8 complete different frame counts in the same call
    (300 and 100 samples), slot 3 idles for calls 3 .. 6 in the middle of its signal."""
    _, S, _, _ = _mods()
    m, _ = _model(4, 22)
    lengths = [900, 650, 1000, 1100, 800, 257, 950, 1200, 700]
    sigs = _signals(lengths, 32)
    steps = [100, 250, 37, 300, 1, 163]

    def count_of(b, ci, left):
        if b == 3 and 3 <= ci <= 6:
            return 0
        return {7: 300, 8: 100}.get(b, steps[(b + ci) % len(steps)])

    st = S.StreamingSessions(m, slots=9, frames_per_launch=8)
    got = _serve(st, [[s] for s in sigs], [0] * 9, 300, count_of)
    ref = S.StreamingDCCRN(m, batch=9, frames_per_launch=8)
    for b, sig in enumerate(sigs):
        assert torch.equal(got[(b, 0)], _lockstep(ref, b, sig)), b


def test_counts_none_equals_lockstep_push_call_by_call():
    _, S, _, _ = _mods()
    m, _ = _model(4, 23)
    g = torch.Generator().manual_seed(33)
    x = (torch.randn(3, 1500, generator=g) * 0.1).cuda()
    st = S.StreamingSessions(m, slots=3, frames_per_launch=8)
    ref = S.StreamingDCCRN(m, batch=3, frames_per_launch=8)
    n = 0
    for sz in [700, 100, 37, 0, 463, 100, 100]:
        y, mm = st.push(x[:, n:n + sz])
        want = ref.push(x[:, n:n + sz])
        n += sz
        assert mm == [want.shape[1]] * 3 and torch.equal(y, want), n
    assert st.positions == [1500] * 3
    with pytest.raises(ValueError, match="GPU tensor"):
        st.push(x[:, :10], counts=torch.tensor([1, 2, 3], device="cuda"))
    with pytest.raises(ValueError, match="0 .. 10"):
        st.push(x[:, :10], counts=[1, 2, 11])
    assert st.positions == [1500] * 3


def test_drop_and_reuse():
    _, S, _, _ = _mods()
    m, _ = _model(4, 24)
    a, b_old, b_new, c = _signals([1000, 900, 600, 1100], 34)
    st = S.StreamingSessions(m, slots=3, frames_per_launch=8)

    def on_call(ci, cur, pos):
        if ci == 3:                                   # slot 1 is 400 samples into b_old: abandon it
            assert st.positions[1] == 400
            st.drop([1])
            assert st.positions[1] == 0
            cur[1] = None
    got = _serve(st, [[a], [b_old, b_new], [c]], [0, 0, 0], 100, lambda b, ci, left: 100, on_call)
    fresh = _serve(S.StreamingSessions(m, slots=3, frames_per_launch=8), [[], [b_new], []], [0, 0, 0], 100, lambda b, ci, left: 100)
    assert got[(1, 1)].shape == (600,) and torch.equal(got[(1, 1)], fresh[(1, 0)])
    assert got[(1, 0)].shape == (100,)                # what b_old returned before it was dropped
    ref = S.StreamingDCCRN(m, batch=3, frames_per_launch=8)
    assert torch.equal(got[(0, 0)], _lockstep(ref, 0, a)) and torch.equal(got[(2, 0)], _lockstep(ref, 2, c))


def _hist(x5):
    """[B, C, F, 2] -> hist [2][C][F][B]"""
    return x5.permute(3, 1, 2, 0).contiguous().reshape(-1)


def _rows(S, B, **fields):
    t = torch.zeros(B, S.NF, dtype=torch.int64)
    for name, v in fields.items():
        t[:, S.ROW_FIELDS.index(name)] = torch.tensor(v, dtype=torch.int64)
    return t


@pytest.mark.parametrize("B", [3, 130])
def test_cconv_rows_entry_every_block_shape(B):
    """Per block shape (conv and transposed, with and without a second source): rows with k_b in {0, 1, 4} and mixed parities
    against the lock-step entry run with k = k_b."""
    _, S, ops, L = _mods()
    g = torch.Generator().manual_seed(B)
    KL = 4
    ks = [(4, 0, 1, 1, 4, 0)[b % 6] for b in range(B)]
    par = [(0, 1, 1, 0, 1)[b % 5] for b in range(B)]
    rows = _rows(S, B, k=ks, parity=par).cuda()
    par_t, every = torch.tensor(par).cuda(), torch.arange(B).cuda()
    sel = {kk: torch.tensor([b for b in range(B) if ks[b] == kk]) for kk in (0, 1, 4)}
    for skip in (SKIP, []):
        m, _ = _model(4, 14, skip=skip)
        st = S.StreamingDCCRN(m, batch=B)
        blocks = [cp for cp in st.enc if skip] + list(st.dec)
        for cp in blocks:
            x5 = torch.randn(B, cp.C0 + cp.C1, cp.Fin, KL + 1, 2, generator=g).cuda()
            xs = [x5[:, :cp.C0]] + ([x5[:, cp.C0:]] if cp.C1 else [])
            # hist halves [2][2*C*F][B]: half parity_b holds column 0 of row b, the other half a marker
            hin = []
            for v in xs:
                h = torch.full((2, v.shape[1] * v.shape[2] * 2, B), 7.0, device="cuda")
                h[par_t, :, every] = _hist(v[:, :, :, 0]).reshape(-1, B).t()
                hin.append(h)
            hin_before = [h.clone() for h in hin]
            srcs = [ops.Planar.from_tensor5(v[:, :, :, 1:].contiguous(), KL + 1) for v in xs]
            out = ops.Planar.empty(cp.Cout, cp.Fout, B, KL, KL + 1, "cuda", zero=True)
            hout = torch.full((2, 2 * cp.Cout * cp.Fout, B), 5.0, device="cuda")
            x0h = torch.full((2, 2 * cp.C0 * cp.Fin, B), 3.0, device="cuda")
            L.call("idv_stream_cconv_rows", srcs[0].ptr(), L.p(hin[0]), L.i(cp.C0), srcs[1].ptr() if cp.C1 else L.p(None),
                   L.p(hin[1]) if cp.C1 else L.p(None), L.i(cp.C1), L.p(cp.w), L.p(cp.bias), L.p(cp.fold), L.p(cp.slope), out.ptr(),
                   L.p(hout), L.p(x0h), L.p(st.work), L.i(cp.nsplit), L.i(1 if cp.transposed else 0), L.i(cp.Cout), L.i(cp.Fin),
                   L.i(B), L.i(KL), L.i(KL + 1), L.i(out.Jp), L.p(rows), L.stream_ptr())
            got = out.tensor5()
            for kk in (1, 4):
                lsrc = [ops.Planar.from_tensor5(v[:, :, :, 1:1 + kk].contiguous(), kk + 1) for v in xs]
                lh = [_hist(v[:, :, :, 0]) for v in xs]
                lout = ops.Planar.empty(cp.Cout, cp.Fout, B, kk, kk + 1, "cuda", zero=True)
                lhout = torch.empty(2 * cp.Cout * cp.Fout * B, device="cuda")
                lx0h = torch.empty(2 * cp.C0 * cp.Fin * B, device="cuda")
                st._conv_call(cp, lsrc[0].ptr(), lh[0], lsrc[1].ptr() if cp.C1 else None, lh[1] if cp.C1 else None, lout.ptr(), lhout,
                              L.p(lx0h), B, kk, kk + 1, lout.Jp)
                s = sel[kk].cuda()
                what = (cp.transposed, cp.C0, cp.C1, cp.Cout, kk)
                assert torch.equal(got[s][:, :, :, :kk], lout.tensor5()[s]), what
                assert torch.equal(hout[1 - par_t[s], :, s], lhout.reshape(-1, B)[:, s].t()), what
                assert torch.equal(x0h[1 - par_t[s], :, s], lx0h.reshape(-1, B)[:, s].t()), what
                assert bool((hout[par_t[s], :, s] == 5.0).all()) and bool((x0h[par_t[s], :, s] == 3.0).all()), what
            idle = sel[0].cuda()                                                 # k_b = 0: no half of any history is written
            assert bool((hout[:, :, idle] == 5.0).all()) and bool((x0h[:, :, idle] == 3.0).all())
            assert all(torch.equal(h, hb) for h, hb in zip(hin, hin_before))     # the histories read stay as they were


def test_clstm_rows_entry_across_two_calls():
    _, S, _, L = _mods()
    m, _ = _model(4, 15)
    B, KL = 11, 4                                       # two workgroups of 8 streams, the second partly filled
    st = S.StreamingDCCRN(m, batch=B)
    H = st.H
    g = torch.Generator().manual_seed(9)
    ks = [[4, 1, 0, 4, 1, 0, 1, 4, 0, 4, 1], [0, 4, 1, 1, 0, 4, 4, 1, 0, 0, 4]]
    state0 = (torch.randn(16, B, H, generator=g) * 0.5).cuda()

    def lock(state, G, kk):
        """The lock-step entry over the first kk steps for all B rows -> (out [B, kk, H, 2], state after)."""
        ops = _mods()[2]
        stt = state.clone()
        out = ops.Planar.empty(H, 1, B, kk, kk + 1, "cuda", zero=True)
        hout = torch.empty(4 * kk * B * H, device="cuda")
        Gk = G.reshape(2, KL * B, 8 * H)[:, :kk * B].contiguous()
        L.call("idv_stream_clstm", L.p(Gk), L.p(st.lstm_wt), L.p(st.lstm_b1), L.p(stt), L.p(hout), out.ptr(), L.i(H), L.i(B), L.i(kk),
               L.i(kk + 1), L.i(out.Jp), L.stream_ptr())
        return out.channel_slice(0, H), stt

    ops = _mods()[2]
    state = state0.clone()                              # the rows entry's state, carried over both calls
    want_state = state0.clone()
    for call in range(2):
        G = torch.randn(2 * KL * B * 8 * H, generator=g).cuda()
        rows = _rows(S, B, k=ks[call]).cuda()
        out = ops.Planar.empty(H, 1, B, KL, KL + 1, "cuda", zero=False)
        hout = torch.full((4 * KL * B * H,), float("nan"), device="cuda")
        L.call("idv_stream_clstm_rows", L.p(G), L.p(st.lstm_wt), L.p(st.lstm_b1), L.p(state), L.p(hout), out.ptr(), L.i(H), L.i(B),
               L.i(KL), L.i(KL + 1), L.i(out.Jp), L.p(rows), L.stream_ptr())
        got = out.channel_slice(0, H)
        before = want_state.clone()
        for kk in (1, 4):
            lo, ls = lock(before, G, kk)
            for b in [b for b in range(B) if ks[call][b] == kk]:
                assert torch.equal(got[b, :kk], lo[b]), (call, b)
                want_state[:, b] = ls[:, b]
        for b in range(B):
            assert not bool(got[b, ks[call][b]:].any()), (call, b)            # steps the slot did not run: zeros
        assert torch.equal(state, want_state), call


def test_frames_and_ola_rows_entries_far_apart():
    """One row 2.56 million frames into its signal, the other at sample 0, in one table: each equals the scalar entry run with
    that row's values."""
    _, S, _, L = _mods()
    B, R, n = 2, NFFT, 700
    pl = S.StreamPlan(NFFT, HOP, WIN)
    half, left, cap = NFFT // 2, (NFFT - WIN) // 2, pl.carry_cap
    g = torch.Generator().manual_seed(12)
    D = 12800 * 20000
    n_prev = [0, D + 300]
    count = [700, 500]
    t0 = [0, pl.frames_ready(n_prev[1])]
    k = [pl.frames_ready(700), pl.frames_ready(n_prev[1] + 500) - t0[1]]
    assert t0[1] > 2_560_000 and k == [6, 5]
    KL, Tp = max(k), max(k) + 1
    e0 = [0, HOP * t0[1] + pl.lo]
    e1 = [pl.final_samples(k[0]), HOP * (t0[1] + k[1]) + pl.lo]
    cin = [0, HOP * (t0[1] - 1) + left + WIN - (half + e0[1])]
    p_end = [HOP * (t0[b] + k[b] - 1) + left + WIN for b in range(B)]
    y_off = [3, 0]
    par = [0, 1]
    ldy = max(y_off[b] + e1[b] - e0[b] for b in range(B))
    span = max(p_end[b] - (half + e0[b]) for b in range(B))
    rows = _rows(S, B, n_prev=n_prev, count=count, L_end=[-1, -1], t0=t0, k=k, parity=par, e0=e0, e1=e1, p_end=p_end, carry_in=cin,
                 T_total=[-1, -1], y_off=y_off)
    assert L.lib().idv_stream_rows_check(L._P(rows.data_ptr()), B, R, n, NFFT, WIN, HOP, cap, KL, Tp, ldy, span) == 0
    rows_d = rows.cuda()
    ring = torch.randn(B, R, generator=g).cuda()
    x = torch.randn(B, n, generator=g)
    for b in range(B):
        x[b, count[b]:] = float("nan")
    x = x.cuda()
    Jp = (B * Tp + 3) // 4 * 4
    fr = torch.full((WIN, Jp), float("nan"), device="cuda")
    L.call("idv_stream_frames_rows", L.p(ring), L.i(R), L.p(x), L.ll(n), L.p(rows_d), L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.i(KL),
           L.p(fr), L.i(Tp), L.i(Jp), L.stream_ptr())
    ifr = torch.randn(WIN, Jp, generator=g).cuda()
    carry = torch.randn(2, B, cap, generator=g).cuda()
    carry_before = carry.clone()
    y = torch.zeros(B, ldy, device="cuda")
    L.call("idv_stream_ola_rows", L.p(ifr), L.i(Tp), L.i(Jp), L.p(carry), L.i(cap), L.p(rows_d), L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP),
           L.i(KL), L.ll(span), L.p(y), L.ll(ldy), L.stream_ptr())
    for b in range(B):
        kb, Tb = k[b], k[b] + 1
        Jb = (B * Tb + 3) // 4 * 4
        sfr = torch.zeros(WIN, Jb, device="cuda")
        L.call("idv_stream_frames", L.p(ring), L.i(R), L.p(x), L.ll(n), L.i(count[b]), L.ll(n_prev[b]), L.ll(-1), L.i(B), L.i(NFFT),
               L.i(WIN), L.i(HOP), L.ll(t0[b]), L.i(kb), L.p(sfr), L.i(Tb), L.i(Jb), L.stream_ptr())
        assert torch.equal(fr[:, b * Tp + 1:b * Tp + 1 + kb], sfr[:, b * Tb + 1:b * Tb + 1 + kb]), b
        assert not bool(fr[:, b * Tp + 1 + kb:b * Tp + 1 + KL].any()), b
        sifr = torch.zeros(WIN, Jb, device="cuda")
        sifr[:, b * Tb + 1:b * Tb + 1 + kb] = ifr[:, b * Tp + 1:b * Tp + 1 + kb]
        sy = torch.zeros(B, e1[b] - e0[b], device="cuda")
        cout = torch.zeros(B, cap, device="cuda")
        L.call("idv_stream_ola", L.p(sifr), L.i(Tb), L.i(Jb), L.p(carry_before[par[b]].contiguous()), L.i(cin[b]), L.p(cout), L.i(cap),
               L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.ll(t0[b]), L.i(kb), L.ll(-1), L.ll(e0[b]), L.ll(e1[b]), L.ll(p_end[b]), L.p(sy),
               L.i(e1[b] - e0[b]), L.ll(0), L.stream_ptr())
        assert torch.equal(y[b, y_off[b]:y_off[b] + e1[b] - e0[b]], sy[b]), b
        nc = p_end[b] - (half + e1[b])
        assert torch.equal(carry[1 - par[b], b, :nc], cout[b, :nc]), b
        assert torch.equal(carry[par[b], b], carry_before[par[b], b]), b
    assert bool(torch.isfinite(y).all()) and not bool(y[0, :3].any())


def _ring_case(seed=21):
    """R = 512, four slots: nothing new; 37 samples from the last ring cell on (the write wraps); a full ring 256 million
    samples into the signal; more samples than the ring holds.  x is NaN at and past count[b] -> (rows, ring, x)."""
    _, S, _, _ = _mods()
    B, R, n = 4, NFFT, 600
    count = [0, 37, 512, 557]
    n_prev = [300, 511, 12800 * 20000 + 300, 0]
    g = torch.Generator().manual_seed(seed)
    ring = torch.randn(B, R, generator=g)
    x = torch.randn(B, n, generator=g)
    for b in range(B):
        x[b, count[b]:] = float("nan")
    return _rows(S, B, n_prev=n_prev, count=count), ring, x


def _ring_entries(rows, ring, x):
    """idv_stream_ring_rows on the table -> the ring; idv_stream_ring with row b's n_new = count_b and n_prev_b on a clone,
    for every b -> row b of each (the other rows of such a call take row b's ranges over their own x, NaN included)."""
    _, S, _, L = _mods()
    B, R = ring.shape
    n = x.shape[1]
    ring, x = ring.cuda(), x.cuda()
    got = ring.clone()
    L.call("idv_stream_ring_rows", L.p(got), L.i(R), L.p(x), L.ll(n), L.i(n), L.p(rows.cuda()), L.i(B), L.stream_ptr())
    want = []
    for b in range(B):
        r = ring.clone()
        L.call("idv_stream_ring", L.p(r), L.i(R), L.p(x), L.ll(n), L.i(int(rows[b, S.ROW_FIELDS.index("count")])),
               L.ll(int(rows[b, S.ROW_FIELDS.index("n_prev")])), L.i(B), L.stream_ptr())
        want.append(r[b])
    return got, torch.stack(want)


def test_ring_rows_entry_equals_the_lockstep_entry():
    """Counts 0, 37, 512 and 557 at a ring of 512 in one table (a wrap inside the write, a far position, a write that starts on
    the last ring cell, more samples than cells): row b equals the scalar entry run with that row's values."""
    rows, ring, x = _ring_case()
    got, want = _ring_entries(rows, ring, x)
    assert torch.equal(got, want)
    assert torch.equal(got[0], ring[0].cuda())                                 # count 0: untouched
    assert not torch.equal(got[1:], ring[1:].cuda())
    assert bool(torch.isfinite(got).all())


def _signal_end_entries(c):
    """The six signal-end entries on one stored case ``c``: ``rows`` [B][NF], ``ring`` [B][R], ``x`` [B][n] (n may be 0),
    ``ifr`` [WIN][Jp], ``carry`` [2][B][cap], ``ldy``, ``span``.  The rows entries run once on the table; the scalar entries run
    once per slot with that slot's values, and what such a run gives for row b is put where the rows entry puts it
    (test_frames_and_ola_rows_entries_far_apart) -> frames [2][WIN][Jp], y [2][B][ldy], carry [2][2][B][cap]: index 0 from the
    rows entries, index 1 from the scalar ones."""
    _, S, _, L = _mods()
    rows = torch.as_tensor(c["rows"])
    f = lambda name: [int(v) for v in rows[:, S.ROW_FIELDS.index(name)]]
    ring, x, ifr, carry0 = (torch.as_tensor(c[k]).cuda() for k in ("ring", "x", "ifr", "carry"))
    ldy, span = int(c["ldy"]), int(c["span"])
    (B, R), n, cap, half = ring.shape, x.shape[1], carry0.shape[2], NFFT // 2
    k, t0, e0, e1, p_end, par, y_off = f("k"), f("t0"), f("e0"), f("e1"), f("p_end"), f("parity"), f("y_off")
    KL, Tp, Jp = max(k), max(k) + 1, ifr.shape[1]
    xp = L.p(x) if n else L.p(None)
    rows_d = rows.cuda()
    fr = torch.zeros(2, WIN, Jp, device="cuda")
    y = torch.zeros(2, B, ldy, device="cuda")
    carry = torch.stack([carry0, carry0])
    L.call("idv_stream_frames_rows", L.p(ring), L.i(R), xp, L.ll(n), L.p(rows_d), L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.i(KL),
           L.p(fr[0]), L.i(Tp), L.i(Jp), L.stream_ptr())
    L.call("idv_stream_ola_rows", L.p(ifr), L.i(Tp), L.i(Jp), L.p(carry[0]), L.i(cap), L.p(rows_d), L.i(B), L.i(NFFT), L.i(WIN),
           L.i(HOP), L.i(KL), L.ll(span), L.p(y[0]), L.ll(ldy), L.stream_ptr())
    for b in range(B):
        kb, Tb, m = k[b], k[b] + 1, e1[b] - e0[b]
        Jb = (B * Tb + 3) // 4 * 4
        sfr = torch.zeros(WIN, Jb, device="cuda")
        L.call("idv_stream_frames", L.p(ring), L.i(R), xp, L.ll(n), L.i(f("count")[b]), L.ll(f("n_prev")[b]), L.ll(f("L_end")[b]),
               L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.ll(t0[b]), L.i(kb), L.p(sfr), L.i(Tb), L.i(Jb), L.stream_ptr())
        fr[1, :, b * Tp + 1:b * Tp + 1 + kb] = sfr[:, b * Tb + 1:b * Tb + 1 + kb]
        sifr = torch.zeros(WIN, Jb, device="cuda")
        sifr[:, b * Tb + 1:b * Tb + 1 + kb] = ifr[:, b * Tp + 1:b * Tp + 1 + kb]
        sy = torch.zeros(B, m, device="cuda")
        cout = torch.zeros(B, cap, device="cuda")
        L.call("idv_stream_ola", L.p(sifr), L.i(Tb), L.i(Jb), L.p(carry0[par[b]].contiguous()), L.i(f("carry_in")[b]), L.p(cout),
               L.i(cap), L.i(B), L.i(NFFT), L.i(WIN), L.i(HOP), L.ll(t0[b]), L.i(kb), L.ll(f("T_total")[b]), L.ll(e0[b]), L.ll(e1[b]),
               L.ll(p_end[b]), L.p(sy), L.i(m), L.ll(0), L.stream_ptr())
        nc = p_end[b] - (half + e1[b])
        y[1, b, y_off[b]:y_off[b] + m] = sy[b]
        carry[1, 1 - par[b], b, :nc] = cout[b, :nc]
    return {"frames": fr, "y": y, "carry": carry}


SIGNAL_END_CASES = ("far", "flush")      # test_frames_and_ola_rows_entries_far_apart's inputs; the end of a signal of 737 samples


def _replay_signal_ends(d):
    """Every output of the six signal-end entries for the inputs stored in ``d`` -> {"<case>.<name>": tensor}."""
    out = {}
    for case in SIGNAL_END_CASES:
        c = {key[len(case) + 4:]: d[key] for key in d.files if key.startswith(case + ".in.")}
        out.update({f"{case}.{name}": v for name, v in _signal_end_entries(c).items()})
    out["ring.ring"] = torch.stack(_ring_entries(*(torch.as_tensor(d[f"ring.in.{k}"]) for k in ("rows", "ring", "x"))))
    return out


def test_signal_end_entries_give_the_recorded_bits(golden):
    """tests/golden/stream_io_parent.npz holds inputs and the outputs of idv_stream_frames / _ring / _ola and their _rows forms
    as the kernels gave them on the MI355X while each form had a kernel body of its own: the shared bodies give the same bits
    (the same sums in the same order; the envelope's device cos is not reproducible on a host, so no CPU reference pins this).
    The flush case has L_end / T_total set and an odd tail, so the end mirror and the clipped envelope are in it."""
    d = golden("stream_io_parent")
    out = _replay_signal_ends(d)
    recorded = sorted(key for key in d.files if ".in." not in key)
    assert recorded == sorted(out) and len(recorded) == 2 * 3 + 1          # per case frames, y, carry: rows and scalar forms
    for name in recorded:
        want = torch.as_tensor(d[name]).cuda()
        assert bool(torch.isfinite(want).all()) and torch.equal(out[name], want), name
    flush = d["flush.in.rows"]
    assert (flush[:, 2] == 737).all() and (flush[:, 10] == 8).all()             # L_end, T_total
