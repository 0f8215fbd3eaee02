"""Edge workgroups of the time-Winograd transposed conv (csrc/cgemm_tw.hip): with an odd number of input rows the last even output
row, out[2 (Fin - 1)] = W4 x[Fin - 2] + W2 x[Fin - 1], is computed by workgroups of the even-row launch that serve TWO adjacent
column blocks with two raw-tap products each, in place of a half-empty row tile per column block.

Tiny shapes (cin <= 16, T <= 45) through ops.cconv2d(..., gauss=pack) on the time-Winograd route: every Fin in {3, 5, 9}; J = B Tp in
(0, 64] (the second half of the one edge workgroup is empty), (64, 128] and (128, 192] (the last edge workgroup is half empty), the
block boundaries 64 and 128 themselves and J that are no multiple of the four columns of a staging item; 32 (one co tile), 64 (paired)
and 40 (ragged second tile) output channels; causal and non-causal taps; a second source, with a ragged last K chunk; fold + PReLU.

Bounds: against the fp64 oracle the bound of tests/test_gpu_ops.py's _conv_case (which this file calls); against the kernel the layer
runs on without the time-Winograd route (cgemm_wino, or cgemm_gauss for one co tile) test_ctconv_time_winograd's 5e-6; addend path and
train-mode moment sums against cgemm_gauss within test_cconv_gauss_stats_and_adjoint's 1e-5."""
import pytest
import torch

from conftest import relerr
from test_gpu_ops import _conv_case

pytestmark = pytest.mark.gpu
PAIR_ALL = 7


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


class _Routes:
    """ops' route switches and launch log restored afterwards."""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        o = self.ops
        self.keep = o.WINO, o.TW, o.TW_PAIR, o.LAUNCH_LOG
        return self

    def __exit__(self, *exc):
        o = self.ops
        o.WINO, o.TW, o.TW_PAIR, o.LAUNCH_LOG = self.keep
        return False


def _tw_ran(ops):
    return bool([c for c, *_ in ops.LAUNCH_LOG if c in (ops.TW_CFG, ops.TW_CFG + 1)])


def _columns(causal, T, B):
    """J = B * Tp as _conv_case lays the input out (Tp = output frames + 1)."""
    return B * ((T if causal else T + 1) + 1)


# causal, cin, cout, F, T, B, skip_c, fold, slope, J
CASES = [
    (True, 8, 32, 3, 45, 1, 0, False, None, 46),       # one column block: the edge workgroup's second half is empty; ONE co tile
    (True, 8, 64, 3, 45, 2, 0, False, 0.25, 92),       # two column blocks: one full edge workgroup; paired co tiles
    (True, 8, 40, 3, 45, 3, 0, True, 0.2, 138),        # three column blocks (138 = 2 mod 4): the last edge workgroup half empty; ragged co tile
    (True, 16, 64, 5, 20, 2, 0, False, None, 42),
    (True, 16, 40, 5, 30, 3, 0, False, 0.1, 93),       # odd J: the last column pair is half empty
    (True, 8, 32, 5, 36, 4, 8, True, 0.25, 148),       # second source, one co tile
    (True, 8, 64, 9, 45, 1, 0, False, None, 46),
    (True, 7, 40, 9, 45, 2, 0, True, None, 92),        # odd channel count: ragged last K chunk
    (True, 16, 32, 9, 45, 3, 0, False, 0.25, 138),
    (False, 6, 40, 5, 44, 2, 0, False, None, 92),      # non-causal taps (window column on the right)
    (False, 8, 64, 9, 30, 5, 0, True, 0.2, 160),       # non-causal, three column blocks
    (False, 8, 32, 3, 19, 2, 0, False, None, 42),      # non-causal, one column block, one co tile
    (True, 8, 64, 5, 45, 3, 4, False, None, 138),      # second source of 4 channels: ragged last K chunk
    (True, 8, 40, 9, 45, 2, 4, True, 0.25, 92),        # the same behind a ragged second co tile
    (True, 8, 64, 3, 31, 2, 0, False, None, 64),       # J = 64: exactly one column block
    (True, 16, 40, 9, 31, 4, 0, False, 0.1, 128),      # J = 128: exactly one edge workgroup
    (True, 16, 64, 9, 42, 3, 0, False, None, 129),     # one column past 128
]


@pytest.mark.parametrize("causal,cin,cout,F,T,B,skip_c,fold,slope,J", CASES)
def test_edge_against_oracle_and_the_kernel_below(ops, causal, cin, cout, F, T, B, skip_c, fold, slope, J):
    assert cin + skip_c <= 16 and T <= 45 and F % 2 == 1
    assert _columns(causal, T, B) == J
    assert ops.L.lib().idv_cconv_tw_supported(cin, skip_c, cout, F)
    with _Routes(ops):
        ops.WINO = ops.TW = True
        ops.LAUNCH_LOG = []
        got = _conv_case(ops, causal, True, cin, cout, F, T, B, seed=71, fold=fold, slope=slope, skip_c=skip_c, gauss=True)   # (oracle bound)
        assert _tw_ran(ops), "time-Winograd kernel not launched"
        ops.TW = False
        ops.LAUNCH_LOG = []
        ref = _conv_case(ops, causal, True, cin, cout, F, T, B, seed=71, fold=fold, slope=slope, skip_c=skip_c, gauss=True)
        assert not _tw_ran(ops)
        wino = bool([c for c, *_ in ops.LAUNCH_LOG if c >= ops.WINO_CFG])
    e = relerr(got, ref)
    # the last even row on its own: a mistake there must not hide behind 2 Fin - 2 correct rows
    e_last = relerr(got[:, :, -1], ref[:, :, -1])
    print(f"J {J}: time-Winograd vs {'cgemm_wino' if wino else 'cgemm_gauss'}: all rows {e:.2e}, last even row {e_last:.2e}")
    assert e < 5e-6 and e_last < 5e-6


@pytest.mark.parametrize("F", [4])
@pytest.mark.parametrize("cout,T,B", [(64, 45, 3), (32, 45, 1), (40, 30, 3)])
def test_even_row_count_against_cgemm_wino(ops, F, cout, T, B):
    """An even Fin has no edge workgroup (tests/test_tw_edge_host.py enumerates the grid); its full tiles now number Fin / 2."""
    with _Routes(ops):
        ops.WINO = ops.TW = True
        ops.LAUNCH_LOG = []
        got = _conv_case(ops, True, True, 16, cout, F, T, B, seed=73, slope=0.2, gauss=True)
        assert _tw_ran(ops)
        ops.TW = False
        ops.LAUNCH_LOG = []
        ref = _conv_case(ops, True, True, 16, cout, F, T, B, seed=73, slope=0.2, gauss=True)
        assert not _tw_ran(ops)
    e = relerr(got, ref)
    print(f"even Fin {F}: time-Winograd vs the kernel below: {e:.2e}")
    assert e < 5e-6


def _inputs(F, T, B, c0, c1, cout, seed, skip_b=None):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, c0, F, T, 2, generator=g)
    sk = torch.randn(skip_b or B, c1, F, T, 2, generator=g) if c1 else None
    shape = (c0 + c1, cout, 5, 2)
    wr, wi = (torch.randn(shape, generator=g) * 0.2).to(dev), (torch.randn(shape, generator=g) * 0.2).to(dev)
    br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    return x, sk, wr, wi, br, bi


@pytest.mark.parametrize("F", [3, 5, 9])
def test_edge_paired_equals_unpaired(ops, F):
    """Two co tiles per workgroup run the one-co-tile program per co tile, edge workgroups included: planes bit-identical."""
    T, B, cout = 45, 3, 64
    x, sk, wr, wi, br, bi = _inputs(F, T, B, 8, 8, cout, seed=75 + F)
    slope = torch.tensor([0.25], device="cuda")
    xp, skp = ops.Planar.from_tensor5(x.cuda(), T + 1), ops.Planar.from_tensor5(sk.cuda(), T + 1)
    res = {}
    with _Routes(ops):
        ops.WINO = ops.TW = True
        pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=True)
        for pair in (PAIR_ALL, 0):
            ops.TW_PAIR = pair
            ops.tw_pair_launches(reset=True)
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=True, slope=slope, skip=skp, gauss=pk)
            torch.cuda.synchronize()
            assert _tw_ran(ops)
            assert ops.tw_pair_launches() == (2 if pair else 0)                 # still one launch per row phase
            res[pair] = y.planes().clone()
    assert torch.equal(res[PAIR_ALL], res[0]), float((res[PAIR_ALL] - res[0]).abs().max())


@pytest.mark.parametrize("ns,B0,T,cout,J", [(2, 1, 20, 64, 42), (3, 1, 30, 40, 93), (2, 2, 30, 32, 124)])
def test_edge_addend_and_moment_sums(ops, ns, B0, T, cout, J):
    """Fin = 5.  The repeated-skip addend (add_div = ns > 1: the addend's column is that of utterance b / ns) and the train-mode moment
    sums apply per column in an edge workgroup as in a full tile: against cgemm_gauss."""
    F, c0, c1 = 5, 8, 8
    B = B0 * ns
    assert B * (T + 1) == J
    x, sk, wr, wi, br, bi = _inputs(F, T, B, c0, c1, cout, seed=81 + ns, skip_b=B0)
    dev = "cuda"
    slope = torch.tensor([0.2], device=dev)
    xp, skp = ops.Planar.from_tensor5(x.to(dev), T + 1), ops.Planar.from_tensor5(sk.to(dev), T + 1)
    sk_rep = ops.Planar.from_tensor5(sk.repeat_interleave(ns, dim=0).to(dev), T + 1)
    res = {}
    with _Routes(ops):
        for tw in (True, False):
            ops.WINO = ops.TW = tw                                               # False: cgemm_gauss
            g_skip = ops.pack_cconv_gauss_skip_part(wr, wi, c0)
            g_main = ops.pack_cconv_gauss(wr, wi, br, bi, None, cin_used=c0, transposed=True)
            g_all = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=True)
            y_skip = ops.cconv2d(skp, None, None, cout, transposed=True, gauss=g_skip)
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=True, slope=slope, gauss=g_main, addend=y_skip, addend_div=ns)
            assert _tw_ran(ops) == tw
            st = torch.zeros(cout, 5, dtype=torch.float64, device=dev)
            ops.LAUNCH_LOG = []
            yt = ops.cconv2d(xp, None, None, cout, transposed=True, skip=sk_rep, stats=st, gauss=g_all)
            assert _tw_ran(ops) == tw
            assert not [c for c, *_ in ops.LAUNCH_LOG if c >= ops.WINO_CFG and c < ops.TW_CFG]
            torch.cuda.synchronize()
            res[tw] = (y.tensor5().cpu(), yt.tensor5().cpu(), st.cpu())
    for k, what in enumerate(("addend output", "train-mode output", "moment sums")):
        e = relerr(res[True][k], res[False][k])
        print(f"{what}: {e:.2e}")
        assert e < 1e-5
    e_last = relerr(res[True][0][:, :, -1], res[False][0][:, :, -1])
    print(f"addend output, last even row: {e_last:.2e}")
    assert e_last < 1e-5
    # the sums are those of the outputs
    t5 = res[True][1].double()
    r_, i_ = t5[..., 0], t5[..., 1]
    own = torch.stack([r_.sum((0, 2, 3)), i_.sum((0, 2, 3)), (r_ * r_).sum((0, 2, 3)), (i_ * i_).sum((0, 2, 3)), (r_ * i_).sum((0, 2, 3))], dim=1)
    assert relerr(res[True][2], own) < 1e-5
