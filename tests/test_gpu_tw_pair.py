"""Time-Winograd convs with two co tiles per workgroup (csrc/cgemm_tw.hip, csrc/cgemm_tw2.hip, NCT = 2; ops.TW_PAIR) against the
one-co-tile kernels (ops.TW_PAIR = 0).  Per co tile the paired kernels stage the same values, read the same weights, run the same
sequence of k-steps into each accumulator and the same epilogue, so every eval-mode output must be BIT-identical (torch.equal on the
whole planes, guard columns included); only the train-mode moment sums (double atomics, in another order) may differ, by the
rounding of a reordered double sum."""
import importlib

import numpy as np
import pytest
import torch

from conftest import relerr
from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # the oracle bound of tests/test_gpu_ops.py (_conv_case)
NFFT, HOP, WIN = 512, 100, 400
PAIR_ALL = 7


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class _Switches:
    """Every time-Winograd route on; ops.TW_PAIR and the launch log restored afterwards."""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        o = self.ops
        self.keep = o.WINO, o.TW, o.TW_CONV, o.TW_PAIR, o.LAUNCH_LOG
        o.WINO = o.TW = o.TW_CONV = True
        return self

    def __exit__(self, *exc):
        o = self.ops
        o.WINO, o.TW, o.TW_CONV, o.TW_PAIR, o.LAUNCH_LOG = self.keep
        return False


def _both(ops, fn):
    """fn() with the paired kernels and with the one-co-tile kernels -> (results, paired launches counted by the library)."""
    res, n = {}, {}
    for pair in (PAIR_ALL, 0):
        ops.TW_PAIR = pair
        ops.tw_pair_launches(reset=True)
        res[pair] = fn()
        torch.cuda.synchronize()
        n[pair] = ops.tw_pair_launches()
    assert n[0] == 0, "ops.TW_PAIR = 0 must run the one-co-tile kernels everywhere"
    return res[PAIR_ALL], res[0], n[PAIR_ALL]


def _conv_pair_case(ops, causal, transposed, cin, cout, F, T, B, seed, fold=False, slope=None, skip_c=0):
    """tests/test_gpu_ops.py's _conv_case on the time-Winograd route, paired and unpaired: planes equal, oracle bound kept."""
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, cin, F, T, 2, generator=g)
    shape = (cin + skip_c, cout, 5, 2) if transposed else (cout, cin + skip_c, 5, 2)
    wr, wi = torch.randn(shape, generator=g) * 0.2, torch.randn(shape, generator=g) * 0.2
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    xin, sk = x, None
    if skip_c:
        sk = torch.randn(B, skip_c, F, T, 2, generator=g)
        xin = torch.cat([x, sk], dim=1)
    if transposed:
        want = O.complex_conv_transpose2d(xin, wr, br, wi, bi, (2, 1), (2, 0), causal)
    else:
        want = O.complex_conv2d(xin, wr, br, wi, bi, (2, 1), (2, 1) if causal else (2, 0), causal)
    fold_t = None
    if fold:
        C = cout
        mom = torch.stack([torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1,
                           0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)])
        gam = [1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g)]
        bet = [0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)]
        want = O.cbn_whiten_affine(want, mom[0], mom[1], mom[2], mom[3], mom[4], gam[0], gam[1], gam[2], bet[0], bet[1])
        fold_t = ops.cbn_fold(mom.to(dev), *[t.to(dev) for t in gam], *[t.to(dev) for t in bet])
    slope_t = None
    if slope is not None:
        slope_t = torch.tensor([slope], device=dev)
        want = O.prelu(want, torch.tensor(slope))
    Tp = max(T, want.shape[3]) + 1
    xp = ops.Planar.from_tensor5(x.to(dev), Tp)
    skp = ops.Planar.from_tensor5(sk.to(dev), Tp) if sk is not None else None
    with _Switches(ops):
        g3 = ops.pack_cconv_gauss(wr.to(dev), wi.to(dev), br.to(dev), bi.to(dev), fold_t, transposed=transposed)
        ids = (ops.TW_CFG, ops.TW_CFG + 1) if transposed else (ops.TW_CFG + 2, ops.TW_CFG + 3)

        def run():
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=transposed, causal=causal, slope=slope_t, skip=skp, gauss=g3)
            assert [c for c, *_ in ops.LAUNCH_LOG if c in ids], "time-Winograd kernel not launched"
            return y
        yp, y1, npair = _both(ops, run)
    cotiles = (cout + 31) // 32
    # an even number of co tiles is paired (both row phases of the transposed form: two launches); an odd number is not
    assert npair == (0 if cotiles % 2 else (2 if transposed else 1)), (cotiles, npair)
    pp, p1 = yp.planes(), y1.planes()
    diff = float((pp - p1).abs().max())
    print(f"cotiles {cotiles} paired launches {npair} max |paired - unpaired| {diff:.3e}")
    assert torch.equal(pp, p1), f"paired and unpaired outputs differ (max {diff:.3e})"
    for y in (yp, y1):
        got = y.tensor5().cpu()
        assert got.shape == want.shape
        e = relerr(got, want)
        print(f"vs oracle: {e:.2e}")
        assert e < TOL
        pl = y.planes()
        assert float(pl[..., 0].abs().max()) == 0.0                      # guard column stays zero
        if pl.shape[-1] > y.T + 1:
            assert float(pl[..., y.T + 1:].abs().max()) == 0.0


@pytest.mark.parametrize("causal,cin,cout,F,T,B,skip_c,fold,slope", [
    (True, 8, 40, 9, 37, 3, 0, True, 0.2),          # two co tiles (ragged second: Cout = 40), odd row count: a half tile; fold + PReLU
    (True, 16, 128, 5, 30, 2, 0, False, None),      # four co tiles
    (True, 16, 256, 5, 30, 2, 0, False, 0.25),      # eight co tiles
    (True, 8, 40, 6, 30, 2, 8, False, None),        # even row count, skip concat (second source)
    (True, 6, 36, 2, 9, 2, 0, False, 0.1),          # ragged second co tile (Cout = 36), two input rows, channels below the pack granularity
    (True, 7, 36, 3, 45, 1, 0, True, None),         # odd channel count: ragged last K chunk; odd columns per utterance (Tp = 46)
    (False, 6, 40, 9, 9, 2, 0, False, None),        # non-causal taps (window column on the right)
    (True, 32, 64, 33, 645, 2, 32, False, 0.25),    # utterance-length columns, Tp = 646, column tail
    (True, 256, 64, 17, 70, 2, 0, True, 0.25),      # a real layer width (dec3's channels): one pair of co tiles
    (True, 16, 36, 4, 31, 3, 4, False, None),       # J = 96: not a multiple of 64; second source of 4 channels (ragged last chunk)
    (True, 16, 32, 9, 37, 2, 16, True, 0.25),       # ONE co tile (dec4's width): not paired, still runs and is equal
    (True, 8, 40, 6, 30, 3, 0, False, 0.2),         # ODD number of columns (B = 3, Tp = 31: J = 93)
    (True, 8, 160, 5, 30, 2, 0, False, None),       # five co tiles: an odd count runs on the one-co-tile kernels
])
def test_ctconv_pair(ops, causal, cin, cout, F, T, B, skip_c, fold, slope):
    assert ops.L.lib().idv_cconv_tw_supported(cin, skip_c, cout, F)
    _conv_pair_case(ops, causal, True, cin, cout, F, T, B, seed=61, fold=fold, slope=slope, skip_c=skip_c)


@pytest.mark.parametrize("causal,cin,cout,F,T,B,fold,slope", [
    (True, 64, 64, 129, 70, 2, False, None),        # two co tiles, odd output row count (65): a half tile
    (True, 64, 40, 65, 33, 2, True, 0.2),           # ragged second co tile (Cout = 40), fold + PReLU
    (True, 72, 128, 17, 40, 3, False, None),        # four co tiles, 72 input channels
    (True, 64, 256, 9, 30, 2, False, 0.25),         # eight co tiles
    (True, 67, 36, 9, 21, 2, False, 0.1),           # ragged second co tile (Cout = 36), odd channel count (ragged last K chunk)
    (False, 64, 40, 17, 9, 2, False, None),         # non-causal taps (x[t], x[t+1])
    (True, 64, 48, 5, 700, 1, False, None),         # many column tiles, 3 output rows, odd Tp
    (True, 128, 128, 33, 70, 2, True, 0.25),        # a real layer width (enc3)
    (True, 80, 32, 4, 30, 3, True, None),           # ONE co tile, even input row count, odd column count (J = 93): not paired
    (True, 136, 64, 4, 30, 3, True, None),          # two co tiles, even input row count (Fout = 2: one tile), J = 93
    (True, 130, 160, 9, 21, 2, False, 0.1),         # five co tiles: an odd count runs on the one-co-tile kernel
])
def test_cconv_pair(ops, causal, cin, cout, F, T, B, fold, slope):
    assert ops.L.lib().idv_cconv_tw2_supported(cin, cout, F)
    _conv_pair_case(ops, causal, False, cin, cout, F, T, B, seed=67, fold=fold, slope=slope)


@pytest.mark.parametrize("ns,B0,c0,c1,cout,F,T", [(2, 2, 16, 16, 40, 17, 21), (3, 1, 8, 8, 64, 9, 30)])
def test_ctconv_pair_addend(ops, ns, B0, c0, c1, cout, F, T):
    """The repeated-skip decoders: the skip half computed once per utterance and added in the paired kernel's epilogue."""
    g = torch.Generator().manual_seed(31 + ns)
    dev = "cuda"
    x = torch.randn(B0 * ns, c0, F, T, 2, generator=g)
    sk = torch.randn(B0, c1, F, T, 2, generator=g)
    wr, wi = torch.randn(c0 + c1, cout, 5, 2, generator=g) * 0.2, torch.randn(c0 + c1, cout, 5, 2, generator=g) * 0.2
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    want = O.complex_conv_transpose2d(torch.cat([x, sk.repeat_interleave(ns, dim=0)], dim=1), wr, br, wi, bi, (2, 1), (2, 0), True)
    mom = torch.stack([torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1, 0.5 + torch.rand(cout, generator=g),
                       0.1 * torch.randn(cout, generator=g), 0.5 + torch.rand(cout, generator=g)])
    gam = [1 + 0.1 * torch.randn(cout, generator=g), torch.randn(cout, generator=g), 1 + 0.1 * torch.randn(cout, generator=g)]
    bet = [0.1 * torch.randn(cout, generator=g), 0.1 * torch.randn(cout, generator=g)]
    want = O.prelu(O.cbn_whiten_affine(want, mom[0], mom[1], mom[2], mom[3], mom[4], gam[0], gam[1], gam[2], bet[0], bet[1]),
                   torch.tensor(0.2))
    fold = ops.cbn_fold(mom.to(dev), *[t.to(dev) for t in gam], *[t.to(dev) for t in bet])
    slope = torch.tensor([0.2], device=dev)
    xp, skp = ops.Planar.from_tensor5(x.to(dev), T + 1), ops.Planar.from_tensor5(sk.to(dev), T + 1)
    with _Switches(ops):
        g_skip = ops.pack_cconv_gauss_skip_part(wr.to(dev), wi.to(dev), c0)
        g_main = ops.pack_cconv_gauss(wr.to(dev), wi.to(dev), br.to(dev), bi.to(dev), fold, cin_used=c0, transposed=True)

        def run():
            y_skip = ops.cconv2d(skp, None, None, cout, transposed=True, gauss=g_skip)
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=True, slope=slope, gauss=g_main, addend=y_skip, addend_div=ns)
            assert [c for c, *_ in ops.LAUNCH_LOG if c in (ops.TW_CFG, ops.TW_CFG + 1)], "time-Winograd kernel not launched"
            return y
        yp, y1, npair = _both(ops, run)
    assert npair >= 2
    assert torch.equal(yp.planes(), y1.planes())
    assert relerr(yp.tensor5().cpu(), want) < TOL
    assert float(yp.planes()[..., 0].abs().max()) == 0.0


@pytest.mark.parametrize("transposed,cin,cout,F,skip_c", [
    (True, 136, 128, 6, 0), (True, 16, 64, 9, 16), (False, 128, 128, 17, 0), (False, 64, 64, 33, 0)])
def test_tw_pair_training_forward(ops, transposed, cin, cout, F, skip_c):
    """Train mode: outputs equal; the five moment sums per channel within the rounding of a reordered double sum.  The per-thread
    and per-half-wave partial sums are float and identical in both forms; only the order of the n double atomicAdds per channel
    (one per workgroup and phase that holds the channel, then the fold of the replicas) differs, so
        |delta| <= n * 2^-52 * sum |addend|.
    sum |addend| from the unpaired run: sum rr and sum ii are sums of non-negative terms (the sum itself); |sum of r i terms| <=
    (sum rr + sum ii) / 2 by |r i| <= (r^2 + i^2) / 2; the first-order sums by Cauchy-Schwarz, sum |y| <= sqrt(N * sum y^2) with N kept
    outputs per channel."""
    g = torch.Generator().manual_seed(9)
    dev = "cuda"
    B, T, Tp = 3, 37, 38
    x = torch.randn(B, cin, F, T, 2, generator=g)
    sk = torch.randn(B, skip_c, F, T, 2, generator=g) if skip_c else None
    shape = (cin + skip_c, cout, 5, 2) if transposed else (cout, cin, 5, 2)
    wr, wi = (torch.randn(shape, generator=g) * 0.1).to(dev), (torch.randn(shape, generator=g) * 0.1).to(dev)
    br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    xp = ops.Planar.from_tensor5(x.to(dev), Tp)
    skp = ops.Planar.from_tensor5(sk.to(dev), Tp) if sk is not None else None
    with _Switches(ops):
        g3 = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=transposed)
        ids = (ops.TW_CFG, ops.TW_CFG + 1) if transposed else (ops.TW_CFG + 2, ops.TW_CFG + 3)

        def run():
            st = torch.zeros(cout, 5, dtype=torch.float64, device=dev)
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=transposed, skip=skp, stats=st, gauss=g3)
            assert [c for c, *_ in ops.LAUNCH_LOG if c in ids], "time-Winograd kernel not launched"
            return y, st
        (yp, sp), (y1, s1), npair = _both(ops, run)
    assert npair == (2 if transposed else 1)
    assert torch.equal(yp.planes(), y1.planes())
    Fout = y1.F
    jtiles = (B * Tp + 63) // 64
    rowtiles = (F + 1) // 2 + F // 2 if transposed else (Fout + 1) // 2         # workgroups per column block that hold a channel
    n = jtiles * rowtiles + ops.STATS_REP
    N = Fout * B * y1.T
    s1c, spc = s1.cpu(), sp.cpu()
    mag = torch.stack([(N * s1c[:, 2]).sqrt(), (N * s1c[:, 3]).sqrt(), s1c[:, 2], s1c[:, 3], 0.5 * (s1c[:, 2] + s1c[:, 3])], dim=1)
    bound = n * 2.0 ** -52 * mag
    delta = (spc - s1c).abs()
    print(f"n = {n}, N = {N}: worst |delta| / bound = {float((delta / bound).max()):.3e}, worst |delta| = {float(delta.max()):.3e}")
    assert bool((delta <= bound).all())
    # and the sums are those of the outputs (the oracle of the statistics: the planes themselves, in double)
    t5 = y1.tensor5().double()
    r_, i_ = t5[..., 0], t5[..., 1]
    ref = torch.stack([r_.sum((0, 2, 3)), i_.sum((0, 2, 3)), (r_ * r_).sum((0, 2, 3)), (i_ * i_).sum((0, 2, 3)), (r_ * i_).sum((0, 2, 3))],
                      dim=1).cpu()
    assert relerr(s1c, ref) < 1e-5 and relerr(spc, ref) < 1e-5


def test_tw_pair_data_gradient(ops):
    """The data-gradient use (test_ctconv_time_winograd_adjoint's shapes, and the conv form as the adjoint of a transposed conv)."""
    g = torch.Generator().manual_seed(12)
    dev = "cuda"
    with _Switches(ops):
        for fwd_transposed, cin, cout, F in ((False, 128, 136, 17), (False, 40, 72, 9), (False, 24, 72, 9), (True, 128, 136, 6)):
            shape = (cin, cout, 5, 2) if fwd_transposed else (cout, cin, 5, 2)
            wr, wi = (torch.randn(shape, generator=g) * 0.1).to(dev), (torch.randn(shape, generator=g) * 0.1).to(dev)
            Fo = 2 * F - 1 if fwd_transposed else (F - 1) // 2 + 1
            dy = ops.Planar.from_tensor5(torch.randn(3, cout, Fo, 37, 2, generator=g).to(dev), 38)
            ga = ops.pack_cconv_gauss(wr, wi, None, None, None, adjoint_of=(cin, cout, cout, not fwd_transposed))
            dp, d1, npair = _both(ops, lambda: ops.cconv_dgrad(dy, None, None, cin, fwd_transposed, True, gauss=ga))
            if fwd_transposed:
                served = bool(ops.L.lib().idv_cconv_tw2_supported(cout, cin, Fo))
            else:
                served = bool(ops.L.lib().idv_cconv_tw_supported(cout, 0, cin, Fo))
            cotiles = (cin + 31) // 32
            print(f"dgrad {cout} -> {cin}: served {served}, co tiles {cotiles}, paired launches {npair}")
            assert npair == ((1 if fwd_transposed else 2) if served and cotiles % 2 == 0 else 0)
            assert torch.equal(dp.planes(), d1.planes())


def test_tw_pair_whole_model_batch_64(ops, golden):
    """DCCRN-CL at the headline shape (B = 64, 4 s; as tests/test_gpu_batch_sizes.py builds it): est and est_stft bit-identical with
    the switch on and off, and the library's own count says that the paired kernels ran (dec0-3 twice, enc2-5 once: 12 launches)."""
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    d = golden("dccrn_full_eval")
    B, rep = 64, 32
    np_ = O.net_params(True, int(d["base"]))
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, [0, 1, 2, 3, 4, 5], "mask", False, None, None)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(O.synth_state_dict(shapes, int(d["seed"])))
    m = m.cuda()
    x = T_(d["x"]).repeat(rep, 1).cuda()
    assert x.shape[0] == B
    with _Switches(ops), torch.no_grad():
        m(x, train=False)                                            # (weights packed, buffers allocated)

        def run():
            est, predict = m(x, train=False)
            return est.clone(), torch.view_as_real(predict).clone()
        (ep, pp), (e1, p1), npair = _both(ops, run)
    print(f"paired launches per forward: {npair}")
    assert npair >= 8, "the paired kernels did not run in the model"
    assert tuple(ep.shape) == (B, 64000)
    assert torch.equal(ep, e1) and torch.equal(pp, p1)
    want = T_(d["clean"]).cuda()
    for r in (0, 1, B - 1):
        assert relerr(ep[r], want[r % 2]) < 1e-4


def test_tw_pair_switch_roundtrip(ops):
    """idv_tw_pair sets and returns the mask; ops.TW_PAIR = None gives the library's own value back."""
    lib = ops.L.lib()
    with _Switches(ops):
        ops.TW_PAIR = None
        ops._sync_tw_pair()
        own = lib.idv_tw_pair(-1)
        ops.TW_PAIR = 5
        ops._sync_tw_pair()
        assert lib.idv_tw_pair(-1) == 5
        assert lib.idv_tw_pair(0xff) == 5 and lib.idv_tw_pair(-1) == PAIR_ALL      # unknown bits are dropped
        ops._tw_pair_pushed = PAIR_ALL
        ops.TW_PAIR = None
        ops._sync_tw_pair()
        assert lib.idv_tw_pair(-1) == own
