"""The two tap sides of the time-Winograd conv form (csrc/cgemm_tw2.hip, idv_cconv2d_tw_fwd) agree bit for bit.

tshift = -1 reads the time taps (x[t - 1], x[t]), tshift = 0 reads (x[t], x[t + 1]); both stage a window of five columns as one
16-byte load and one 4-byte load and differ only in where the window starts.  So the entry with tshift = -1 on x must equal the entry
with tshift = 0 on x shifted right by one frame inside each utterance: the products, the column pairs and the k order are the same.
Compared with torch.equal on all rows and on frames 1 .. T - 2 of every utterance (both runs keep the same T - 1 frames, so that the
train-mode moment sums are sums of the same outputs).  And on the tap-left side, two co tiles per workgroup equal one (torch.equal).

Shapes: the smallest that reach every copy of the K loop -- cin 64 and 67 (ragged last chunk: the masked window path); Fin 9 (edge
workgroups) and 8 (none); J = B Tp = 64, 128 and 129 (one, two and three column blocks, T <= 45); cout 32 and 160 (one co tile per
workgroup), 64 (two: the early and the late staging copies); eval with fold + PReLU, and train mode with moment sums.

Moment sums: equal within the rounding of the reordered double sum, as tests/test_gpu_tw_pair.py states it -- the per-thread and
per-half-wave partial sums are float and identical; only the order of the n double atomicAdds per channel differs, so
|delta| <= n * 2^-52 * sum |addend|, with sum |addend| bounded from the sums themselves (sum rr, sum ii: the sum; |sum ri| <= (sum rr +
sum ii) / 2; first-order sums by Cauchy-Schwarz with N kept outputs per channel)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
PAIR_ALL = 7

# cin, cout, Fin, T, B (J = B * (T + 1))
CASES = [
    (64, 32, 9, 31, 2),       # J = 64: one column block, the edge workgroup's second half empty; one co tile
    (67, 32, 8, 42, 3),       # J = 129; ragged last chunk; no edge workgroups
    (64, 160, 9, 42, 3),      # five co tiles, unpaired; three column blocks: the last edge workgroup half empty
    (67, 160, 8, 31, 2),
    (64, 64, 9, 31, 4),       # J = 128: two co tiles per workgroup, one full edge workgroup
    (67, 64, 9, 42, 3),       # paired, ragged last chunk, J = 129
    (64, 64, 8, 31, 2),       # paired, full tiles only
    (67, 64, 8, 31, 4),
]


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


class _Pair:
    """ops.TW_PAIR restored afterwards."""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        self.keep = self.ops.TW_PAIR
        return self

    def __exit__(self, *exc):
        self.ops.TW_PAIR = self.keep
        self.ops._sync_tw_pair()
        return False


def _layer(ops, cin, cout, F, T, B, train, seed):
    """-> (x, x shifted right by one frame, pack, slope)"""
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, cin, F, T, 2, generator=g)
    wr, wi = torch.randn(cout, cin, 5, 2, generator=g) * 0.2, torch.randn(cout, cin, 5, 2, generator=g) * 0.2
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    fold_t, slope = None, None
    if not train:
        C = cout
        mom = torch.stack([torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1,
                           0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)])
        gam = [1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g)]
        bet = [0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)]
        fold_t = ops.cbn_fold(mom.to(dev), *[t.to(dev) for t in gam], *[t.to(dev) for t in bet])
        slope = torch.tensor([0.25], device=dev)
    keep = ops.WINO, ops.TW, ops.TW_CONV
    try:
        ops.WINO = ops.TW = ops.TW_CONV = True
        pk = ops.pack_cconv_gauss(wr.to(dev), wi.to(dev), br.to(dev), bi.to(dev), fold_t, transposed=False)
    finally:
        ops.WINO, ops.TW, ops.TW_CONV = keep
    assert pk.tw is not None
    xp = ops.Planar.from_tensor5(x.to(dev), T + 1)
    xs = ops.Planar.empty(cin, F, B, T, T + 1, dev, zero=True)
    xs.planes()[..., 1:].copy_(xp.planes()[..., :-1])               # frame t of xs = frame t - 1 of x; frame 0 = the guard column
    assert float(xs.planes()[..., :2].abs().max()) == 0.0
    return xp, xs, pk, slope


def _run(ops, x, pk, cout, tshift, t_valid, slope, train, pair):
    """One launch of idv_cconv2d_tw_fwd -> (planes [2, Cout, Fout, B, Tp], moment sums | None, paired launches)"""
    i, p = ops.i, ops.p
    dev = "cuda"
    assert ops.L.lib().idv_cconv_tw2_supported(i(x.C), i(cout), i(x.F))
    out = ops.Planar.empty(cout, (x.F - 1) // 2 + 1, x.B, t_valid, x.Tp, dev, zero=True)
    stats = torch.zeros(cout, 5, dtype=torch.float64, device=dev) if train else None
    swork = ops._stats_work(stats, cout)
    ops.TW_PAIR = pair
    ops._sync_tw_pair()
    ops.tw_pair_launches(reset=True)
    ops.call("idv_cconv2d_tw_fwd", x.ptr(), i(x.C), p(pk.tw), p(pk.epi), i(pk.has_fold), p(slope), out.ptr(), p(stats), p(swork),
             i(ops.STATS_REP), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(t_valid), ops.stream_ptr())
    torch.cuda.synchronize()
    return out.planes().clone(), (stats.cpu() if train else None), ops.tw_pair_launches()


def _sums_agree(ops, s_ref, s_got, Fin, B, T, what):
    Fout, Tp = (Fin - 1) // 2 + 1, T + 1
    n = (B * Tp + 63) // 64 * ((Fout + 1) // 2) + ops.STATS_REP     # double atomicAdds per channel, at most
    N = Fout * B * (T - 1)                                          # kept outputs per channel
    mag = torch.stack([(N * s_ref[:, 2]).sqrt(), (N * s_ref[:, 3]).sqrt(), s_ref[:, 2], s_ref[:, 3], 0.5 * (s_ref[:, 2] + s_ref[:, 3])], dim=1)
    bound = n * 2.0 ** -52 * mag
    delta = (s_got - s_ref).abs()
    print(f"{what}: n = {n}, N = {N}: worst |delta| / bound = {float((delta / bound).max()):.3e}, worst |delta| = {float(delta.max()):.3e}")
    assert bool((delta <= bound).all())


@pytest.mark.parametrize("train", [False, True], ids=["eval_fold_prelu", "train_sums"])
@pytest.mark.parametrize("cin,cout,F,T,B", CASES)
def test_tap_sides_and_pairing_agree(ops, cin, cout, F, T, B, train):
    assert cin >= 64 and T <= 45 and B * (T + 1) in (64, 128, 129)
    xp, xs, pk, slope = _layer(ops, cin, cout, F, T, B, train, seed=90 + F + cout)
    paired = (cout + 31) // 32 % 2 == 0
    with _Pair(ops):
        left, s_left, n_left = _run(ops, xp, pk, cout, -1, T - 1, slope, train, PAIR_ALL)
        right, s_right, n_right = _run(ops, xs, pk, cout, 0, T - 1, slope, train, PAIR_ALL)
        left1, s_left1, n_left1 = _run(ops, xp, pk, cout, -1, T - 1, slope, train, 0)
    assert n_left == n_right == (1 if paired else 0) and n_left1 == 0
    assert float(left.abs().max()) > 0.1
    # planes [2, Cout, Fout, B, Tp], frame t at column t + 1: all rows, frames 1 .. T - 2 of every utterance
    a, b = left[..., 2:T], right[..., 2:T]
    assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(left, left1), float((left - left1).abs().max())
    if train:
        _sums_agree(ops, s_left1, s_right, F, B, T, "tap right vs tap left")
        _sums_agree(ops, s_left1, s_left, F, B, T, "paired vs unpaired")
        # and the sums are those of the outputs
        r_, i_ = left1[0].double().cpu(), left1[1].double().cpu()
        own = torch.stack([r_.sum((1, 2, 3)), i_.sum((1, 2, 3)), (r_ * r_).sum((1, 2, 3)), (i_ * i_).sum((1, 2, 3)), (r_ * i_).sum((1, 2, 3))], dim=1)
        assert float((s_left1 - own).norm() / own.norm()) < 1e-5
