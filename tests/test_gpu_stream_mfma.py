"""The fp32-MFMA streaming conv engine (``conv="mfma"``) on the MI355X against the vector-ALU engine: v_mfma_f32_32x32x2_f32 is fed
the products of the vector-ALU fmaf chain in its order, so every comparison between the engines is ``torch.equal``: the entries
block by block (lock-step and per-row), the deepest K split, both streamers end to end, and the reference waveform."""
import importlib
import random

import numpy as np
import pytest
import torch

from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4                      # the waveform tolerance of tests/test_gpu_streaming.py
OP_TOL = 2e-5                   # its operator tolerance


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


def _hist(x5):
    """[B, C, F, 2] -> hist [2][C][F][B]"""
    return x5.permute(3, 1, 2, 0).contiguous().reshape(-1)


def _blocks(st):
    return [("enc", e, cp) for e, cp in enumerate(st.enc)] + [("dec", d, cp) for d, cp in enumerate(st.dec)]


def _entry(L, name, cp, work, srcs, hists, out, hout, x0h, B, k):
    """One lock-step entry (idv_stream_cconv or idv_stream_cconv_mfma) with the pack ``cp``."""
    L.call(name, srcs[0].ptr(), L.p(hists[0]), L.i(cp.C0), srcs[1].ptr() if cp.C1 else L.p(None), L.p(hists[1]) if cp.C1 else L.p(None),
           L.i(cp.C1), L.p(cp.w), L.p(cp.bias), L.p(cp.fold), L.p(cp.slope), out.ptr(), L.p(hout), L.p(x0h), L.p(work),
           L.i(cp.nsplit), L.i(1 if cp.transposed else 0), L.i(cp.Cout), L.i(cp.Fin), L.i(B), L.i(k), L.i(k + 1), L.i(out.Jp),
           L.stream_ptr())


def _compare_entries(va, mf, B, k, g, np_, sd, kinds, x0hist=True):
    """Every supported block of the streamers ``va`` (conv="valu") and ``mf`` (conv="mfma"): both entries on the same inputs ->
    the number of blocks compared."""
    _, _, ops, L = _mods()
    n = 0
    for (kind, idx, cv), (_, _, cm) in zip(_blocks(va), _blocks(mf)):
        assert cv.engine == "valu" and cm.engine == ("mfma" if cm.Cout >= 16 else "valu") and cv.nsplit == cm.nsplit
        if cm.engine != "mfma" or kind not in kinds:
            continue
        x5 = torch.randn(B, cv.C0 + cv.C1, cv.Fin, k + 1, 2, generator=g)
        if kind == "enc":
            want = O.encoder_block(x5, sd, f"std_DCCRN.encoders.{idx}.", np_, idx, True, False)
        else:
            want = O.decoder_block(x5, sd, f"std_DCCRN.decoders.{idx}.", np_, idx, True, False)
        xs = [x5[:, :cv.C0].cuda()] + ([x5[:, cv.C0:].cuda()] if cv.C1 else [])
        srcs = [ops.Planar.from_tensor5(v[:, :, :, 1:].contiguous(), k + 1) for v in xs]
        hists = [_hist(v[:, :, :, 0]) for v in xs]
        res = []
        for name, cp, st in (("idv_stream_cconv", cv, va), ("idv_stream_cconv_mfma", cm, mf)):
            out = ops.Planar.empty(cv.Cout, cv.Fout, B, k, k + 1, "cuda", zero=True)
            hout = torch.full((2 * cv.Cout * cv.Fout * B,), 5.0, device="cuda")
            x0h = torch.full((2 * cv.C0 * cv.Fin * B,), 3.0, device="cuda") if x0hist else None
            _entry(L, name, cp, st.work, srcs, hists, out, hout, x0h, B, k)
            res.append((out, hout, x0h))
        (ov, hv, xv), (om, hm, xm) = res
        what = (kind, idx, cv.transposed, cv.C0, cv.C1, cv.Cout, cv.nsplit, B, k)
        assert torch.equal(om.buf, ov.buf), what                 # guard columns and slack included
        assert torch.equal(hm, hv), what
        if x0hist:
            assert torch.equal(xm, xv), what
        assert relerr(om.tensor5().cpu(), want[:, :, :, 1:]) < OP_TOL, what
        n += 1
    return n


@pytest.mark.parametrize("base,least", [(4, 7), (12, 9)])
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("k", [1, 4])
def test_entries_every_block_shape_bit_identical(base, least, B, k):
    """Base 12: Cout 24 / 48 / 96 (partly filled and odd numbers of 32-row tiles), Cin no multiple of 8."""
    _, S, _, _ = _mods()
    g = torch.Generator().manual_seed(1000 * base + 10 * B + k)
    for skip in (SKIP, []):
        m, np_ = _model(base, 14, skip=skip)
        sd = {kk: v.cpu() for kk, v in m.state_dict().items()}
        va, mf = S.StreamingDCCRN(m, batch=B, conv="valu"), S.StreamingDCCRN(m, batch=B, conv="mfma")
        n = _compare_entries(va, mf, B, k, g, np_, sd, ("enc", "dec") if skip else ("dec",))
        assert n >= (least if skip else 3), (n, skip)        # of the 12 blocks with the skips; the decoders alone without


@pytest.mark.parametrize("k", [1, 4])
def test_full_width_deep_split_bit_identical(k):
    _, S, _, _ = _mods()
    B = 1
    g = torch.Generator().manual_seed(200 + k)
    m, np_ = _model(32, 16)
    sd = {kk: v.cpu() for kk, v in m.state_dict().items()}
    va, mf = S.StreamingDCCRN(m, batch=B, conv="valu"), S.StreamingDCCRN(m, batch=B, conv="mfma")
    assert max(cp.nsplit for cp in mf.enc + mf.dec) > 16
    assert _compare_entries(va, mf, B, k, g, np_, sd, ("enc", "dec"), x0hist=False) == 11


def _rows(S, B, **fields):
    t = torch.zeros(B, S.NF, dtype=torch.int64)
    for name, v in fields.items():
        t[:, S.ROW_FIELDS.index(name)] = torch.tensor(v, dtype=torch.int64)
    return t


@pytest.mark.parametrize("B", [3, 130])
def test_rows_entry_bit_identical(B):
    """k_b in {0, 1, 4} and mixed parities in one table, sentinels in every history half."""
    _, S, ops, L = _mods()
    g = torch.Generator().manual_seed(300 + B)
    KL = 4
    ks = [(4, 0, 1, 1, 4, 0)[b % 6] for b in range(B)]
    par = [(0, 1, 1, 0, 1)[b % 5] for b in range(B)]
    rows = _rows(S, B, k=ks, parity=par).cuda()
    par_t, every = torch.tensor(par).cuda(), torch.arange(B).cuda()
    for skip in (SKIP, []):
        n = 0
        m, _ = _model(12, 14, skip=skip)
        va, mf = S.StreamingDCCRN(m, batch=B, conv="valu"), S.StreamingDCCRN(m, batch=B, conv="mfma")
        for (kind, idx, cv), (_, _, cm) in zip(_blocks(va), _blocks(mf)):
            if cm.engine != "mfma" or (kind == "enc" and not skip):
                continue
            x5 = torch.randn(B, cv.C0 + cv.C1, cv.Fin, KL + 1, 2, generator=g).cuda()
            xs = [x5[:, :cv.C0]] + ([x5[:, cv.C0:]] if cv.C1 else [])
            hin = []
            for v in xs:                                  # half parity_b holds column 0 of row b, the other half a marker
                h = torch.full((2, v.shape[1] * v.shape[2] * 2, B), 7.0, device="cuda")
                h[par_t, :, every] = _hist(v[:, :, :, 0]).reshape(-1, B).t()
                hin.append(h)
            hin_before = [h.clone() for h in hin]
            srcs = [ops.Planar.from_tensor5(v[:, :, :, 1:].contiguous(), KL + 1) for v in xs]
            res = []
            for name, cp, st in (("idv_stream_cconv_rows", cv, va), ("idv_stream_cconv_mfma_rows", cm, mf)):
                out = ops.Planar.empty(cv.Cout, cv.Fout, B, KL, KL + 1, "cuda", zero=True)
                hout = torch.full((2, 2 * cv.Cout * cv.Fout, B), 5.0, device="cuda")
                x0h = torch.full((2, 2 * cv.C0 * cv.Fin, B), 3.0, device="cuda")
                L.call(name, srcs[0].ptr(), L.p(hin[0]), L.i(cp.C0), srcs[1].ptr() if cp.C1 else L.p(None),
                       L.p(hin[1]) if cp.C1 else L.p(None), L.i(cp.C1), L.p(cp.w), L.p(cp.bias), L.p(cp.fold), L.p(cp.slope), out.ptr(),
                       L.p(hout), L.p(x0h), L.p(st.work), L.i(cp.nsplit), L.i(1 if cp.transposed else 0), L.i(cp.Cout), L.i(cp.Fin),
                       L.i(B), L.i(KL), L.i(KL + 1), L.i(out.Jp), L.p(rows), L.stream_ptr())
                res.append((out.tensor5(), hout, x0h))
            (ov, hv, xv), (om, hm, xm) = res
            what = (kind, idx, cv.transposed, cv.C0, cv.C1, cv.Cout, cv.nsplit)
            for b in range(B):
                assert torch.equal(om[b, :, :, :ks[b]], ov[b, :, :, :ks[b]]), (what, b)
            assert torch.equal(hm, hv) and torch.equal(xm, xv), what
            idle = torch.tensor([b for b in range(B) if ks[b] == 0]).cuda()
            assert bool((hm[:, :, idle] == 5.0).all()) and bool((xm[:, :, idle] == 3.0).all()), what
            live = torch.tensor([b for b in range(B) if ks[b] > 0]).cuda()
            assert bool((hm[par_t[live], :, live] == 5.0).all()) and bool((xm[par_t[live], :, live] == 3.0).all()), what
            assert not bool((hm[1 - par_t[live], :, live] == 5.0).all()), what
            assert all(torch.equal(h, hb) for h, hb in zip(hin, hin_before)), what
            n += 1
        assert n == (9 if skip else 4), (n, skip)


def _stream(st, x, sizes):
    outs, n = [], 0
    for m in sizes:
        outs.append(st.push(x[:, n:n + m]))
        n += m
    assert n == x.shape[1]
    outs.append(st.flush())
    return torch.cat(outs, dim=1)


def _random_sizes(L, seed):
    rng = random.Random(seed)
    out, left = [], L
    while left:
        n = min(left, rng.choice([0, 0, 1, 13, 99, 100, 250, 777]))
        out.append(n)
        left -= n
    return out


def test_streamer_chunk_invariance_equals_valu():
    _, S, _, _ = _mods()
    m, _ = _model(4, 11)
    B, L = 3, 2345
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, L, generator=g) * 0.1).cuda()
    want = _stream(S.StreamingDCCRN(m, batch=B, frames_per_launch=8, conv="valu"), x, [L])
    st = S.StreamingDCCRN(m, batch=B, frames_per_launch=8, conv="mfma")
    assert st.conv_engines == ["mfma" if cp.Cout >= 16 else "valu" for cp in st.enc + st.dec]
    assert st.conv_engines.count("mfma") == 7 and S.StreamingDCCRN(m, batch=B).conv_engines == ["valu"] * 12
    chunkings = {"whole": [L], "1then100": [1] * 700 + [100] * ((L - 700) // 100) + [(L - 700) % 100],
                 "hop": [HOP] * (L // HOP) + [L % HOP], "37": [37] * (L // 37) + [L % 37], "random": _random_sizes(L, 3),
                 "over_cap": [1500, L - 1500]}
    for name, sizes in chunkings.items():
        assert torch.equal(_stream(st, x, sizes), want), name


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


def test_sessions_equal_the_valu_lockstep_streamer():
    """The staggered scenario of tests/test_gpu_stream_sessions.py with conv="mfma" sessions."""
    _, S, _, _ = _mods()
    m, np_ = _model(4, 21)
    a, b1, b2, c = _signals([1234, 777, 401, 2345], 31)
    rng = random.Random(4)
    st = S.StreamingSessions(m, slots=3, frames_per_launch=8, conv="mfma")
    assert st.conv_engines.count("mfma") == 7
    got = _serve(st, [[a], [b1, b2], [c]], [0, 1, 3], 300, lambda b, ci, left: rng.choice([0, 0, 1, 37, 100, 250, 300]))
    assert st.positions == [0, 0, 0]
    ref = S.StreamingDCCRN(m, batch=3, frames_per_launch=8, conv="valu")
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    for (slot, j), sig in {(0, 0): a, (1, 0): b1, (1, 1): b2, (2, 0): c}.items():
        want = _lockstep(ref, slot, sig)
        assert got[(slot, j)].shape == want.shape == (HOP * (len(sig) // HOP),)
        assert torch.equal(got[(slot, j)], want), (slot, j)
        o = O.dccrn_forward(sig[None].cpu(), sd, np_, True, NFFT, HOP, WIN, SKIP)[0]
        assert relerr(got[(slot, j)][None], o) < TOL, (slot, j)


def test_reference_parity_full_width(golden):
    _, S, _, _ = _mods()
    d = golden("dccrn_full_eval")
    m, _ = _model(int(d["base"]), int(d["seed"]))
    x = torch.from_numpy(np.asarray(d["x"])).cuda()
    st = S.StreamingDCCRN(m, batch=x.shape[0], conv="mfma")
    assert x.shape[0] == 2 and st.conv_engines.count("mfma") == 11 and st.conv_engines[-1] == "valu"
    y = _stream(st, x, [160] * (x.shape[1] // 160) + ([x.shape[1] % 160] if x.shape[1] % 160 else []))
    want = torch.from_numpy(np.asarray(d["clean"]))
    assert y.shape == want.shape and relerr(y, want) < TOL


def test_unknown_engine_is_refused():
    _, S, _, _ = _mods()
    m, _ = _model(4, 11)
    for cls in (S.StreamingDCCRN, S.StreamingSessions):
        with pytest.raises(ValueError, match="conv"):
            cls(m, 2, conv="bogus")
