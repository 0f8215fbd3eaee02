"""The split-bf16 streaming conv engine (``conv="bf16x3"``, csrc/stream_conv_bf16.hip) on the MI355X.

Exact integers first: with 10-bit integers on one side and integers in -3 .. 3 on the other every product and every partial sum
is an exact fp32 number in any order and the dropped lo lo term is zero, so the engine must return the bits of the vector-ALU
entry (every wrong index, lane map, tap, sign, tile edge or K-part boundary shows).  Then normal data against the float64 split
model of tests/stream_bf16_ref.py, the per-row entry, the streamers (cut invariance to the bit, the waveform tolerance of the
fp32 engines), sessions with save / load, the VAE kinds and the full width."""
import importlib
import random

import numpy as np
import pytest
import torch

import stream_bf16_ref as R
from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4                      # the streaming waveform tolerance of the fp32 engines (tests/test_gpu_streaming.py)
CONV_KEYS = ("conv.conv_re.weight", "conv.conv_im.weight", "transconv.tconv_re.weight", "transconv.tconv_im.weight")


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.streaming"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"),
            importlib.import_module("i-dccrn-vae_amd.inference"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _model(base, seed, skip=SKIP, wmax=None):
    """``wmax``: the conv weights of the DCCRN blocks are integers in -wmax .. wmax (bias, batch norm and PReLU stay random)."""
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, skip, "mask", False, None, None)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k not in ("data_mean", "data_std")}, seed)
    if wmax is not None:
        g = torch.Generator().manual_seed(seed + 1)
        for k in sd:
            if k.startswith("std_DCCRN.") and k.endswith(CONV_KEYS):
                sd[k] = torch.randint(-wmax, wmax + 1, tuple(sd[k].shape), generator=g).to(sd[k].dtype)
    m.load_state_dict(sd, strict=True)
    return m.cuda(), np_


def _expected_engines(st):
    lib = _mods()[3].lib()
    out = []
    for cp in st.enc + (st.dec if hasattr(st, "dec") else [cp for ch in st.chains for cp in ch.dec]):
        shape = (1 if cp.transposed else 0, cp.C0 + cp.C1, cp.Cout)
        out.append("bf16x3" if lib.idv_stream_cconv_bf16_supported(*shape) == 1 else
                   ("mfma" if lib.idv_stream_cconv_mfma_supported(*shape) == 1 else "valu"))
    return out


def _hist(x5):
    """[B, C, F, 2] -> hist [2][C][F][B]"""
    return x5.permute(3, 1, 2, 0).contiguous().reshape(-1)


def _blocks(st):
    return [("enc", e, cp) for e, cp in enumerate(st.enc)] + [("dec", d, cp) for d, cp in enumerate(st.dec)]


def _entry(name, cp, work, xs, B, k, x0hist=True):
    """One lock-step entry with the pack ``cp`` on xs (per source [B, C, Fin, k + 1, 2], column 0 the history) -> (out, hist_out,
    x0hist_out): out zeroed first, the histories filled with markers."""
    _, _, ops, L, _ = _mods()
    srcs = [ops.Planar.from_tensor5(v[:, :, :, 1:].contiguous(), k + 1) for v in xs]
    hists = [_hist(v[:, :, :, 0]) for v in xs]
    out = ops.Planar.empty(cp.Cout, cp.Fout, B, k, k + 1, "cuda", zero=True)
    hout = torch.full((2 * cp.Cout * cp.Fout * B,), 5.0, device="cuda")
    x0h = torch.full((2 * cp.C0 * cp.Fin * B,), 3.0, device="cuda") if x0hist else None
    L.call(name, srcs[0].ptr(), L.p(hists[0]), L.i(cp.C0), srcs[1].ptr() if cp.C1 else L.p(None), L.p(hists[1]) if cp.C1 else L.p(None),
           L.i(cp.C1), L.p(cp.w), L.p(cp.bias), L.p(cp.fold), L.p(cp.slope), out.ptr(), L.p(hout), L.p(x0h), L.p(work),
           L.i(cp.nsplit), L.i(1 if cp.transposed else 0), L.i(cp.Cout), L.i(cp.Fin), L.i(B), L.i(k), L.i(k + 1), L.i(out.Jp),
           L.stream_ptr())
    return out, hout, x0h


def _sources(x5, cp):
    return [x5[:, :cp.C0].cuda()] + ([x5[:, cp.C0:].cuda()] if cp.C1 else [])


def _abs_sum_bound(m, kind, idx, xmax):
    """An upper bound of sum |w| |x| of any output of block idx: xmax times the largest sum over (ci, kf, kt) of |wr| + |wi|."""
    sd = m.state_dict()
    pre = f"std_DCCRN.{'encoders' if kind == 'enc' else 'decoders'}.{idx}." + ("conv.conv_" if kind == "enc" else "transconv.tconv_")
    w = sd[pre + "re.weight"].abs().double() + sd[pre + "im.weight"].abs().double()
    return xmax * float(w.sum(dim=(1, 2, 3) if kind == "enc" else (0, 2, 3)).max())


# ------------------------------------------------------------------------------------------------- 1. exact integers, no tolerance
def _compare_exact(m, B, k, g, xmax, kinds, x0hist=True):
    """Every bf16x3 block of StreamingDCCRN(m): idv_stream_cconv_bf16 against idv_stream_cconv on integers in -xmax .. xmax ->
    the number of blocks compared."""
    S = _mods()[1]
    va, bf = S.StreamingDCCRN(m, batch=B, conv="valu"), S.StreamingDCCRN(m, batch=B, conv="bf16x3")
    assert bf.conv_engines == _expected_engines(bf)
    n = 0
    for (kind, idx, cv), (_, _, cb) in zip(_blocks(va), _blocks(bf)):
        assert cv.engine == "valu" and cv.nsplit == cb.nsplit
        if cb.engine != "bf16x3" or kind not in kinds:
            continue
        assert _abs_sum_bound(m, kind, idx, xmax) < 2 ** 24          # every partial sum is an exact fp32 number
        x5 = torch.randint(-xmax, xmax + 1, (B, cv.C0 + cv.C1, cv.Fin, k + 1, 2), generator=g).float()
        xs = _sources(x5, cv)
        ov, hv, xv = _entry("idv_stream_cconv", cv, va.work, xs, B, k, x0hist)
        ob, hb, xb = _entry("idv_stream_cconv_bf16", cb, bf.work, xs, B, k, x0hist)
        what = (kind, idx, cv.transposed, cv.C0, cv.C1, cv.Cout, cv.nsplit, B, k, xmax)
        assert torch.equal(ob.buf, ov.buf), what                     # guard columns and slack included
        assert torch.equal(hb, hv), what
        if x0hist:
            assert torch.equal(xb, xv), what
        assert float(ob.buf.abs().max()) > 0
        n += 1
    return n


@pytest.mark.parametrize("base,least", [(4, 7), (12, 9)])
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("k", [1, 4])
def test_exact_integers_every_block_shape_equals_valu(base, least, B, k):
    """x in -1023 .. 1023 with w in -3 .. 3 (the x_lo path) and the mirror set (the w_lo path).  Base 12: Cout 24 / 48 / 96 (partly
    filled and odd numbers of 32-row tiles), Cin no multiple of 8, K parts that are no multiple of the channel group."""
    g = torch.Generator().manual_seed(1000 * base + 10 * B + k)
    for wmax, xmax in ((3, 1023), (1023, 3)):
        for skip in (SKIP, []):
            m, _ = _model(base, 14, skip=skip, wmax=wmax)
            n = _compare_exact(m, B, k, g, xmax, ("enc", "dec") if skip else ("dec",))
            assert n >= (least if skip else 3), (n, skip)


@pytest.mark.parametrize("k", [1, 4])
def test_exact_integers_full_width_deep_split_equals_valu(k):
    S = _mods()[1]
    m, _ = _model(32, 16, wmax=1)
    bf = S.StreamingDCCRN(m, batch=1, conv="bf16x3")
    assert max(cp.nsplit for cp in bf.enc + bf.dec) > 16
    assert bf.conv_engines == ["mfma"] + ["bf16x3"] * 10 + ["valu"]
    assert _compare_exact(m, 1, k, torch.Generator().manual_seed(200 + k), 1023, ("enc", "dec"), x0hist=False) == 10


# ------------------------------------------------------------------------------------------------------------------ 2. normal data
@pytest.mark.parametrize("base,B,k", [(4, 3, 4), (12, 1, 1), (12, 130, 4), (12, 3, 1)])
def test_normal_data_within_the_fp32_engines_error_of_the_split_model(base, B, k):
    """e32: the relative L2 error of idv_stream_cconv_mfma against the float64 block, measured here (that engine is not under
    test).  The bf16x3 entry stands within 4 e32 of the float64 split model (it adds three times as many terms, in the matrix
    core's own order) and within (split model against float64) + 4 e32 of the float64 block."""
    S = _mods()[1]
    g = torch.Generator().manual_seed(77 * base + 10 * B + k)
    m, np_ = _model(base, 14)
    sd = {kk: v.cpu() for kk, v in m.state_dict().items()}
    mf, bf = S.StreamingDCCRN(m, batch=B, conv="mfma"), S.StreamingDCCRN(m, batch=B, conv="bf16x3")
    n = 0
    for (kind, idx, cm), (_, _, cb) in zip(_blocks(mf), _blocks(bf)):
        if cb.engine != "bf16x3":
            continue
        assert cm.engine == "mfma" and cm.nsplit == cb.nsplit
        x5 = torch.randn(B, cm.C0 + cm.C1, cm.Fin, k + 1, 2, generator=g)
        exact = R.split_block(kind, idx, x5, sd, np_, exact=True)[:, :, :, 1:]
        model = R.split_block(kind, idx, x5, sd, np_)[:, :, :, 1:]
        xs = _sources(x5, cm)
        om = _entry("idv_stream_cconv_mfma", cm, mf.work, xs, B, k)[0].tensor5()
        ob = _entry("idv_stream_cconv_bf16", cb, bf.work, xs, B, k)[0].tensor5()
        e32, e_model, e_exact, model_exact = relerr(om, exact), relerr(ob, model), relerr(ob, exact), relerr(model, exact)
        print(f"base {base} B {B} k {k} {kind}{idx} Cin {cm.C0 + cm.C1} Cout {cm.Cout} nsplit {cm.nsplit}: fp32 MFMA vs float64 "
              f"{e32:.3e}, bf16x3 vs split model {e_model:.3e} ({e_model / e32:.2f} e32), vs float64 {e_exact:.3e}, split model vs "
              f"float64 {model_exact:.3e}")
        what = (kind, idx, B, k)
        assert e_model <= 4 * e32, what
        assert e_exact <= model_exact + 4 * e32, what
        n += 1
    assert n == (7 if base == 4 else 9)


# ---------------------------------------------------------------------------------------------------------------- 3. the rows entry
def _rows(S, B, **fields):
    t = torch.zeros(B, S.NF, dtype=torch.int64)
    for name, v in fields.items():
        t[:, S.ROW_FIELDS.index(name)] = torch.tensor(v, dtype=torch.int64)
    return t


@pytest.mark.parametrize("B,integers", [(3, False), (130, False), (130, True)])
def test_rows_entry_equals_the_lockstep_entry_per_row(B, integers):
    """k_b in {0, 1, 4} and mixed parities in one table, sentinels in every history half.  A row with k_b frames equals the
    lock-step entry at k = k_b (the same B, so the same K parts); ``integers``: the exact-integer set against
    idv_stream_cconv_rows as well."""
    _, S, ops, L, _ = _mods()
    g = torch.Generator().manual_seed(300 + B)
    KL = 4
    ks = [(4, 0, 1, 1, 4, 0)[b % 6] for b in range(B)]
    par = [(0, 1, 1, 0, 1)[b % 5] for b in range(B)]
    rows = _rows(S, B, k=ks, parity=par).cuda()
    par_t, every = torch.tensor(par).cuda(), torch.arange(B).cuda()
    idle = torch.tensor([b for b in range(B) if ks[b] == 0]).cuda()
    live = torch.tensor([b for b in range(B) if ks[b] > 0]).cuda()
    for skip in (SKIP, []):
        n = 0
        m, _ = _model(12, 14, skip=skip, wmax=3 if integers else None)
        va, bf = S.StreamingDCCRN(m, batch=B, conv="valu"), S.StreamingDCCRN(m, batch=B, conv="bf16x3")
        for (kind, idx, cv), (_, _, cb) in zip(_blocks(va), _blocks(bf)):
            if cb.engine != "bf16x3" or (kind == "enc" and not skip):
                continue
            if integers:
                assert _abs_sum_bound(m, kind, idx, 1023) < 2 ** 24
                x5 = torch.randint(-1023, 1024, (B, cv.C0 + cv.C1, cv.Fin, KL + 1, 2), generator=g).float()
            else:
                x5 = torch.randn(B, cv.C0 + cv.C1, cv.Fin, KL + 1, 2, generator=g)
            xs = _sources(x5, cv)
            hin = []
            for v in xs:                                  # half parity_b holds column 0 of row b, the other half a marker
                h = torch.full((2, v.shape[1] * v.shape[2] * 2, B), 7.0, device="cuda")
                h[par_t, :, every] = _hist(v[:, :, :, 0]).reshape(-1, B).t()
                hin.append(h)
            hin_before = [h.clone() for h in hin]
            srcs = [ops.Planar.from_tensor5(v[:, :, :, 1:].contiguous(), KL + 1) for v in xs]
            res = []
            for name, cp, st in (("idv_stream_cconv_bf16_rows", cb, bf),) + ((("idv_stream_cconv_rows", cv, va),) if integers else ()):
                out = ops.Planar.empty(cv.Cout, cv.Fout, B, KL, KL + 1, "cuda", zero=True)
                hout = torch.full((2, 2 * cv.Cout * cv.Fout, B), 5.0, device="cuda")
                x0h = torch.full((2, 2 * cv.C0 * cv.Fin, B), 3.0, device="cuda")
                L.call(name, srcs[0].ptr(), L.p(hin[0]), L.i(cp.C0), srcs[1].ptr() if cp.C1 else L.p(None),
                       L.p(hin[1]) if cp.C1 else L.p(None), L.i(cp.C1), L.p(cp.w), L.p(cp.bias), L.p(cp.fold), L.p(cp.slope), out.ptr(),
                       L.p(hout), L.p(x0h), L.p(st.work), L.i(cp.nsplit), L.i(1 if cp.transposed else 0), L.i(cp.Cout), L.i(cp.Fin),
                       L.i(B), L.i(KL), L.i(KL + 1), L.i(out.Jp), L.p(rows), L.stream_ptr())
                res.append((out.tensor5(), hout, x0h))
            ob, hb, xb = res[0]
            what = (kind, idx, cv.transposed, cv.C0, cv.C1, cv.Cout, cv.nsplit)
            for kb in (1, 4):                             # the lock-step entry at k = k_b, every row
                lo, lh, lx = _entry("idv_stream_cconv_bf16", cb, bf.work, [v[:, :, :, :kb + 1] for v in xs], B, kb)
                lo, lh, lx = lo.tensor5(), lh.reshape(-1, B), lx.reshape(-1, B)
                for b in [b for b in range(B) if ks[b] == kb]:
                    assert torch.equal(ob[b, :, :, :kb], lo[b]), (what, b)
                    assert torch.equal(hb[1 - par[b], :, b], lh[:, b]) and torch.equal(xb[1 - par[b], :, b], lx[:, b]), (what, b)
            assert bool((hb[:, :, idle] == 5.0).all()) and bool((xb[:, :, idle] == 3.0).all()), what
            assert bool((hb[par_t[live], :, live] == 5.0).all()) and bool((xb[par_t[live], :, live] == 3.0).all()), what
            assert not bool((hb[1 - par_t[live], :, live] == 5.0).all()), what
            assert all(torch.equal(h, h0) for h, h0 in zip(hin, hin_before)), what
            if integers:
                ov, hv, xv = res[1]
                for b in range(B):
                    assert torch.equal(ob[b, :, :, :ks[b]], ov[b, :, :, :ks[b]]), (what, b)
                assert torch.equal(hb, hv) and torch.equal(xb, xv), what
            n += 1
        assert n == (9 if skip else 4), (n, skip)


# ------------------------------------------------------------------------------------------------------------------ 4. the streamer
def _stream(st, x, sizes):
    outs, n = [], 0
    for m in sizes:
        outs.append(st.push(x[:, n:n + m]))
        n += m
    assert n == x.shape[1]
    outs.append(st.flush())
    return torch.cat(outs, dim=1)


def _hops(L, n=HOP):
    return [n] * (L // n) + ([L % n] if L % n else [])


def _random_sizes(L, seed):
    rng = random.Random(seed)
    out, left = [], L
    while left:
        n = min(left, rng.choice([0, 0, 1, 13, 99, 100, 250, 777]))
        out.append(n)
        left -= n
    return out


@pytest.mark.parametrize("base,count", [(4, 7), (12, 9)])
def test_streamer_cut_invariance_and_waveform_tolerance(base, count):
    _, S, _, _, _ = _mods()
    m, np_ = _model(base, 11)
    B, L = 3, 2345
    x = (torch.randn(B, L, generator=torch.Generator().manual_seed(5)) * 0.1).cuda()
    st = S.StreamingDCCRN(m, batch=B, frames_per_launch=8, conv="bf16x3")
    assert st.conv_engines == _expected_engines(st) and st.conv_engines.count("bf16x3") == count
    assert set(st.conv_engines) <= {"bf16x3", "mfma", "valu"} and S.StreamingDCCRN(m, batch=B).conv_engines == ["valu"] * 12
    want = _stream(st, x, [L])
    chunkings = {"1then100": [1] * 700 + [100] * ((L - 700) // 100) + [(L - 700) % 100], "hop": _hops(L), "37": _hops(L, 37),
                 "random": _random_sizes(L, 3), "over_cap": [1500, L - 1500]}
    for name, sizes in chunkings.items():
        assert torch.equal(_stream(st, x, sizes), want), name
    fp32 = _stream(S.StreamingDCCRN(m, batch=B, frames_per_launch=8, conv="mfma"), x, [L])
    assert not torch.equal(want, fp32)                               # another arithmetic
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    o = O.dccrn_forward(x.cpu(), sd, np_, True, NFFT, HOP, WIN, SKIP)[0]
    print(f"base {base}: bf16x3 stream vs CPU oracle {relerr(want, o):.3e}, fp32 stream vs CPU oracle {relerr(fp32, o):.3e}, "
          f"bf16x3 vs fp32 stream {relerr(want, fp32):.3e}")
    assert want.shape == o.shape and relerr(want, o) < TOL


# ------------------------------------------------------------------------------------------------------- 5. sessions, save / load
def _signals(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(L, generator=g) * 0.1).cuda() for L in lengths]


def _lockstep(ref, slot, sig):
    """The signal whole in slot ``slot`` of the lock-step streamer ``ref`` (the other slots carry zeros), then flushed -> [1, m]."""
    x = torch.zeros(ref.B, len(sig), device="cuda")
    x[slot] = sig
    return torch.cat([ref.push(x), ref.flush()], dim=1)[slot:slot + 1]


def _serve(st, queues, starts, width, count_of):
    """Feeds ``queues[b]`` (the signals of slot b, one after the other, the first from call ``starts[b]``) through ``st`` with
    ``count_of(b, call, remaining)`` samples per call; a signal ends in the call that brings its last samples.  Every call's
    x[b, counts[b]:] is NaN.  Returns {(slot, index of the signal in its queue): output [1, samples]}."""
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
        y, m = st.push(x, counts, end)
        assert y.shape == (B, max(m)) and bool(torch.isfinite(y).all())
        for b in range(B):
            assert not bool(y[b, m[b]:].any())
            if cur[b] is not None:
                outs.setdefault((b, idx[b]), []).append(y[b:b + 1, :m[b]])
        for b in end:
            cur[b] = None
        ci += 1
    return {k: torch.cat(v, dim=1) for k, v in outs.items()}


def _staggered(st, seed=4):
    """The schedule of tests/test_gpu_stream_sessions.py: queues [[a], [b1, b2], [c]], starts at calls 0, 1, 3."""
    a, b1, b2, c = _signals([1234, 777, 401, 2345], 31)
    rng = random.Random(seed)
    got = _serve(st, [[a], [b1, b2], [c]], [0, 1, 3], 300, lambda b, ci, left: rng.choice([0, 0, 1, 37, 100, 250, 300]))
    assert st.positions == [0, 0, 0]
    return got, {(0, 0): a, (1, 0): b1, (1, 1): b2, (2, 0): c}


def test_sessions_equal_the_lockstep_streamer_of_the_engine():
    _, S, _, _, _ = _mods()
    m, np_ = _model(4, 21)
    st = S.StreamingSessions(m, slots=3, frames_per_launch=8, conv="bf16x3")
    assert st.conv_engines == _expected_engines(st) and st.conv_engines.count("bf16x3") == 7
    got, sigs = _staggered(st)
    ref = S.StreamingDCCRN(m, batch=3, frames_per_launch=8, conv="bf16x3")
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    for (slot, j), sig in sigs.items():
        want = _lockstep(ref, slot, sig)
        assert got[(slot, j)].shape == want.shape == (1, HOP * (len(sig) // HOP))
        assert torch.equal(got[(slot, j)], want), (slot, j)
        o = O.dccrn_forward(sig[None].cpu(), sd, np_, True, NFFT, HOP, WIN, SKIP)[0]
        assert relerr(got[(slot, j)], o) < TOL, (slot, j)


def _feed(st, slot, sig, sizes, end):
    """``sig`` into slot ``slot`` of the sessions object in pushes of ``sizes`` (the other slots idle); ``end``: the last push ends
    the signal -> the slot's output."""
    outs, n = [], 0
    for j, c in enumerate(sizes):
        x = torch.full((st.B, max(c, 1)), float("nan"), device="cuda")
        x[slot, :c] = sig[n:n + c]
        counts = [c if b == slot else 0 for b in range(st.B)]
        y, m = st.push(x, counts, [slot] if end and j == len(sizes) - 1 else [])
        outs.append(y[slot:slot + 1, :m[slot]])
        n += c
    assert n == len(sig)
    return torch.cat(outs, dim=1)


def test_save_load_continues_to_the_bit_and_into_an_fp32_engine_within_tolerance():
    _, S, _, _, _ = _mods()
    m, _ = _model(4, 21)
    a = _signals([2345], 33)[0]
    cut = 777
    want = _lockstep(S.StreamingDCCRN(m, batch=3, frames_per_launch=8, conv="bf16x3"), 2, a)
    want32 = _lockstep(S.StreamingDCCRN(m, batch=3, frames_per_launch=8, conv="mfma"), 2, a)
    st1 = S.StreamingSessions(m, slots=3, frames_per_launch=8, conv="bf16x3")
    head = _feed(st1, 2, a[:cut], [100, 250, 37, 300, 90], end=False)
    state = st1.save([2])[0]
    st1.drop([2])
    tail_sizes = [1, 99, 300, 13, 250, 300, 300, 205, 100]
    st2 = S.StreamingSessions(m, slots=3, frames_per_launch=8, conv="bf16x3")
    st2.load([0], [state])
    got = torch.cat([head, _feed(st2, 0, a[cut:], tail_sizes, end=True)], dim=1)
    assert got.shape == want.shape and torch.equal(got, want)
    st3 = S.StreamingSessions(m, slots=3, frames_per_launch=8, conv="mfma")          # the state is fp32 in every engine
    st3.load([1], [state])
    mixed = torch.cat([head, _feed(st3, 1, a[cut:], tail_sizes, end=True)], dim=1)
    print(f"bf16x3 head, fp32 tail: vs the bf16x3 stream {relerr(mixed, want):.3e}, vs the fp32 stream {relerr(mixed, want32):.3e}; "
          f"bf16x3 vs fp32 stream {relerr(want, want32):.3e}")
    assert mixed.shape == want.shape and not torch.equal(mixed, want)
    assert relerr(mixed, want) < TOL and relerr(mixed, want32) < TOL


# ------------------------------------------------------------------------------------------------------------------ 6. VAE kinds
def load_synth(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(O.synth_state_dict(shapes, seed), strict=True)
    return module.cuda()


def _vae_nets(base=4, zdim=16, ns=2, seed=40):
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    enc = load_synth(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2), seed + 1)
    mk = lambda sd: load_synth(pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP, False), sd)
    return enc, mk(seed + 2), mk(seed + 3)


def _vae_case(lock, sessions, offline_of):
    """Cut invariance of the lock-step streamer ``lock`` (batch 3), the sessions form against it, and the offline path with the
    same draws (``offline_of(x, st)``), at the tolerance of the fp32 VAE streaming tests."""
    B, L = 3, 1234
    x = (torch.randn(B, L, generator=torch.Generator().manual_seed(5)) * 0.1).cuda()
    assert lock.conv_engines == _expected_engines(lock) and "bf16x3" in lock.conv_engines
    whole = _stream(lock, x, [L])
    for sizes in (_hops(L), _hops(L, 37), _random_sizes(L, 3)):
        assert torch.equal(_stream(lock, x, sizes), whole)
    off = offline_of(x, lock)
    print(f"{type(lock).__name__} bf16x3 vs the offline path: {relerr(whole, off):.3e}")
    assert whole.shape == off.shape and relerr(whole, off) < TOL
    assert sessions.conv_engines == lock.conv_engines
    got, sigs = _staggered(sessions)
    for (slot, j), sig in sigs.items():
        assert torch.equal(got[(slot, j)], _lockstep(lock, slot, sig)), (slot, j)


def test_streaming_vae_and_its_sessions():
    _, S, _, _, inf = _mods()
    enc, dec, _ = _vae_nets()

    def offline(x, st):
        T = 1 + x.shape[1] // HOP
        g = torch.Generator().manual_seed(99)
        other = tuple(torch.randn(x.shape[0], 2, T, 16, generator=g).cuda() for _ in range(2))
        return inf.enhance_vae(enc, dec, x, eps=st.eps(0, T) + other, latent="speech")
    _vae_case(S.StreamingVAE(enc, dec, batch=3, seed=3, frames_per_launch=8, conv="bf16x3"),
              S.StreamingVAESessions(enc, dec, slots=3, seed=3, frames_per_launch=8, conv="bf16x3"), offline)


def test_streaming_vae_two_latents_and_its_sessions():
    _, S, _, _, inf = _mods()
    enc, ds, dn = _vae_nets()
    kw = dict(outtype="phase_mask", phase=2, seed=3, frames_per_launch=8, conv="bf16x3")
    offline = lambda x, st: inf.enhance_vae_two_latents(enc, ds, dn, x, "phase_mask", 2, eps=st.eps(0, 1 + x.shape[1] // HOP))
    _vae_case(S.StreamingVAETwoLatents(enc, ds, dn, batch=3, **kw), S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=3, **kw), offline)


# ------------------------------------------------------------------------------------------------------------------ 7. full width
def test_reference_parity_full_width(golden):
    """Against the reference's own output, and against the offline model's bf16x3 mode: the stream's deviation from the fp32 stream
    stays within twice the offline bf16x3 deviation from offline fp32 (which also splits the LSTM and the point-wise products)."""
    _, S, ops, _, _ = _mods()
    d = golden("dccrn_full_eval")
    m, _ = _model(int(d["base"]), int(d["seed"]))
    x = torch.from_numpy(np.asarray(d["x"])).cuda()
    sizes = _hops(x.shape[1], 160)
    st = S.StreamingDCCRN(m, batch=x.shape[0], conv="bf16x3")
    assert x.shape[0] == 2 and st.conv_engines == ["mfma"] + ["bf16x3"] * 10 + ["valu"]
    y = _stream(st, x, sizes)
    y32 = _stream(S.StreamingDCCRN(m, batch=x.shape[0], conv="mfma"), x, sizes)
    want = torch.from_numpy(np.asarray(d["clean"]))
    keep = ops.PRECISION
    try:
        with torch.no_grad():
            ops.set_precision("fp32")
            off32 = m(x, train=False)[0]
            ops.set_precision("bf16x3")
            off16 = m(x, train=False)[0]
    finally:
        ops.set_precision(keep)
    dev_stream, dev_offline = relerr(y, y32), relerr(off16, off32)
    print(f"full width: bf16x3 stream vs the reference {relerr(y, want):.3e}, fp32 stream vs the reference {relerr(y32, want):.3e}, "
          f"bf16x3 stream vs fp32 stream {dev_stream:.3e}, offline bf16x3 vs offline fp32 {dev_offline:.3e}")
    assert y.shape == want.shape and relerr(y, want) < TOL
    assert 0 < dev_stream <= 2 * dev_offline


# -------------------------------------------------------------------------------------------------------------- 8. unknown engines
def test_unknown_engine_is_refused_by_every_class():
    _, S, _, _, _ = _mods()
    m, _ = _model(4, 11)
    enc, ds, dn = _vae_nets()
    for make in (lambda c: S.StreamingDCCRN(m, 2, conv=c), lambda c: S.StreamingSessions(m, 2, conv=c),
                 lambda c: S.StreamingVAE(enc, ds, batch=2, conv=c), lambda c: S.StreamingVAESessions(enc, ds, slots=2, conv=c),
                 lambda c: S.StreamingVAETwoLatents(enc, ds, dn, batch=2, conv=c),
                 lambda c: S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=2, conv=c)):
        with pytest.raises(ValueError, match="conv"):
            make("bogus")
