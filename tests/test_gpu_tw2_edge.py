"""Edge workgroups of the time-Winograd conv form (csrc/cgemm_tw2.hip): with an odd number of output rows and Fin = 2 Fout - 1 the last
output row, out[Fout - 1] = W0 x[Fin - 3] + W1 x[Fin - 2] + W2 x[Fin - 1], is computed by workgroups of the one launch that serve TWO
adjacent column blocks with the three raw taps each, in place of a half-empty row tile per column block.

The smallest shapes the route serves (cin from 64: the gate of idv_cconv_tw2_supported; T <= 45) through ops.cconv2d(..., gauss=pack):
Fin in {5, 9, 17}; J = B Tp in (0, 64] (the second half of the one edge workgroup is empty), (64, 128] and (128, 192] (the last edge
workgroup half empty), the block boundaries 64, 128 and 129 themselves, an odd J and J that are no multiple of the four columns of a
staging item; 32 (one co tile), 64 (paired), 40 (ragged second co tile) and 160 (five co tiles, unpaired) output channels; cin = 67
(ragged last K chunk); causal and non-causal taps; fold + PReLU.

Bounds: against the fp64 oracle the bound of tests/test_gpu_ops.py's _conv_case (which this file calls); against the kernel the layer
runs on with ops.TW_CONV = False (cgemm_wino's conv form, or cgemm_gauss for one co tile) test_cconv_time_winograd's 5e-6; train-mode
outputs and moment sums against cgemm_gauss within test_cconv_gauss_stats_and_adjoint's 1e-5.  Every bound holds for all rows and for
the last output row alone."""
import pytest
import torch

from conftest import relerr
from oracle import idccrn_oracle as O
from test_gpu_ops import TOL, _conv_case

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
        self.keep = o.WINO, o.TW, o.TW_CONV, o.TW_PAIR, o.LAUNCH_LOG
        return self

    def __exit__(self, *exc):
        o = self.ops
        o.WINO, o.TW, o.TW_CONV, o.TW_PAIR, o.LAUNCH_LOG = self.keep
        return False


def _tw2_ran(ops):
    return bool([c for c, *_ in ops.LAUNCH_LOG if c in (ops.TW_CFG + 2, ops.TW_CFG + 3)])


def _oracle_last_row(causal, cin, cout, F, T, B, seed, fold, slope):
    """The last output row of _conv_case's oracle result (the same generator sequence), for the bound on that row alone."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, F, T, 2, generator=g)
    wr, wi = torch.randn(cout, cin, 5, 2, generator=g) * 0.2, torch.randn(cout, cin, 5, 2, generator=g) * 0.2
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    want = O.complex_conv2d(x, wr, br, wi, bi, (2, 1), (2, 1) if causal else (2, 0), causal)
    if fold:
        C = cout
        mom = torch.stack([torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1,
                           0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)])
        gam = [1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g)]
        bet = [0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)]
        want = O.cbn_whiten_affine(want, mom[0], mom[1], mom[2], mom[3], mom[4], gam[0], gam[1], gam[2], bet[0], bet[1])
    if slope is not None:
        want = O.prelu(want, torch.tensor(slope))
    return want[:, :, -1]


def _against_oracle_and_the_kernel_below(ops, causal, cin, cout, F, T, B, fold, slope, seed):
    assert ops.L.lib().idv_cconv_tw2_supported(cin, cout, F)
    with _Routes(ops):
        ops.WINO = ops.TW = ops.TW_CONV = True
        ops.LAUNCH_LOG = []
        got = _conv_case(ops, causal, False, cin, cout, F, T, B, seed=seed, fold=fold, slope=slope, gauss=True)      # (oracle bound)
        assert _tw2_ran(ops), "time-Winograd conv kernel not launched"
        ops.TW_CONV = False
        ops.LAUNCH_LOG = []
        ref = _conv_case(ops, causal, False, cin, cout, F, T, B, seed=seed, fold=fold, slope=slope, gauss=True)
        assert not _tw2_ran(ops)
    want_last = _oracle_last_row(causal, cin, cout, F, T, B, seed, fold, slope)
    e, e_last = relerr(got, ref), relerr(got[:, :, -1], ref[:, :, -1])
    o_last = relerr(got[:, :, -1], want_last)
    print(f"conv form vs the kernel below: all rows {e:.2e}, last row {e_last:.2e}; last row vs oracle {o_last:.2e}")
    # the last row on its own: a mistake there must not hide behind the correct rows
    assert o_last < TOL
    assert e < 5e-6 and e_last < 5e-6


# causal, cin, cout, F, T, B, fold, slope, J = B * (T + 1)
CASES = [
    (True, 64, 32, 5, 45, 1, False, None, 46),        # one column block: the edge workgroup's second half is empty; ONE co tile
    (True, 64, 64, 5, 45, 2, False, 0.25, 92),        # two column blocks: one full edge workgroup; paired co tiles
    (True, 64, 40, 5, 45, 3, True, 0.2, 138),         # three column blocks (138 = 2 mod 4): the last edge workgroup half empty; ragged co tile
    (True, 64, 160, 9, 20, 2, False, None, 42),       # five co tiles: unpaired
    (True, 67, 40, 9, 30, 3, False, 0.1, 93),         # ragged last K chunk; odd J: the last column pair is half empty
    (True, 64, 64, 9, 31, 2, False, None, 64),        # J = 64: exactly one column block
    (True, 64, 32, 17, 31, 4, True, 0.25, 128),       # J = 128: exactly one edge workgroup
    (True, 64, 64, 17, 42, 3, False, None, 129),      # one column past 128
    (False, 64, 40, 5, 44, 2, False, None, 90),       # non-causal taps (window column on the right)
    (False, 64, 64, 9, 31, 5, True, 0.2, 160),        # non-causal, three column blocks
    (False, 67, 32, 17, 19, 2, False, None, 40),      # non-causal, one column block, one co tile, ragged last K chunk
    (True, 67, 160, 17, 45, 3, True, 0.2, 138),       # five co tiles behind a ragged K chunk, fold + PReLU
    (True, 64, 64, 17, 45, 1, False, 0.1, 46),        # paired, the edge workgroup's second half empty
]


@pytest.mark.parametrize("causal,cin,cout,F,T,B,fold,slope,J", CASES)
def test_edge_against_oracle_and_the_kernel_below(ops, causal, cin, cout, F, T, B, fold, slope, J):
    assert cin >= 64 and T <= 45 and F % 2 == 1 and ((F + 1) // 2) % 2 == 1
    assert B * (T + 1) == J
    _against_oracle_and_the_kernel_below(ops, causal, cin, cout, F, T, B, fold, slope, seed=71)


@pytest.mark.parametrize("F,cout,T,B", [(4, 64, 45, 3), (8, 32, 45, 1), (8, 40, 30, 3), (6, 64, 45, 3), (6, 32, 31, 2), (6, 160, 30, 3)])
def test_no_edge_row_counts_stay_correct(ops, F, cout, T, B):
    """Fin = 4, 8: an even Fout, full tiles only.  Fin = 6: Fout = 3 is odd, but its last row has four real taps and stays a half tile
    (tests/test_tw2_edge_host.py enumerates the grids)."""
    _against_oracle_and_the_kernel_below(ops, True, 64, cout, F, T, B, False, 0.2, seed=73)


def _inputs(F, T, B, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, cin, F, T, 2, generator=g)
    shape = (cout, cin, 5, 2)
    wr, wi = (torch.randn(shape, generator=g) * 0.2).to(dev), (torch.randn(shape, generator=g) * 0.2).to(dev)
    br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    return x, wr, wi, br, bi


@pytest.mark.parametrize("F", [5, 9, 17])
def test_edge_paired_equals_unpaired(ops, F):
    """Two co tiles per workgroup run the one-co-tile program per co tile, edge workgroups included: planes bit-identical."""
    T, B, cin, cout = 45, 3, 64, 64
    x, wr, wi, br, bi = _inputs(F, T, B, cin, cout, seed=75 + F)
    slope = torch.tensor([0.25], device="cuda")
    xp = ops.Planar.from_tensor5(x.cuda(), T + 1)
    res = {}
    with _Routes(ops):
        ops.WINO = ops.TW = ops.TW_CONV = True
        pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=False)
        for pair in (PAIR_ALL, 0):
            ops.TW_PAIR = pair
            ops.tw_pair_launches(reset=True)
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=False, slope=slope, gauss=pk)
            torch.cuda.synchronize()
            assert _tw2_ran(ops)
            assert ops.tw_pair_launches() == (1 if pair else 0)                 # still one launch
            res[pair] = y.planes().clone()
    assert torch.equal(res[PAIR_ALL], res[0]), float((res[PAIR_ALL] - res[0]).abs().max())


@pytest.mark.parametrize("F,T,B,cout", [(5, 30, 3, 64), (9, 20, 2, 40), (9, 45, 3, 32)])
def test_edge_moment_sums(ops, F, T, B, cout):
    """The train-mode forward: outputs and the five moment sums per channel of an edge workgroup's columns as of a full tile's,
    against cgemm_gauss; and the sums are those of the returned outputs."""
    cin = 64
    x, wr, wi, br, bi = _inputs(F, T, B, cin, cout, seed=81 + F)
    dev = "cuda"
    xp = ops.Planar.from_tensor5(x.to(dev), T + 1)
    res = {}
    with _Routes(ops):
        for tw in (True, False):
            ops.WINO = ops.TW = ops.TW_CONV = tw                                 # False: cgemm_gauss
            pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=False)
            st = torch.zeros(cout, 5, dtype=torch.float64, device=dev)
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=False, stats=st, gauss=pk)
            torch.cuda.synchronize()
            assert _tw2_ran(ops) == tw
            assert tw or not [c for c, *_ in ops.LAUNCH_LOG if c >= ops.WINO_CFG]
            res[tw] = (y.tensor5().cpu(), st.cpu())
    for k, what in enumerate(("train-mode output", "moment sums")):
        e = relerr(res[True][k], res[False][k])
        print(f"{what}: {e:.2e}")
        assert e < 1e-5
    e_last = relerr(res[True][0][:, :, -1], res[False][0][:, :, -1])
    print(f"train-mode output, last row: {e_last:.2e}")
    assert e_last < 1e-5
    t5 = res[True][0].double()
    r_, i_ = t5[..., 0], t5[..., 1]
    own = torch.stack([r_.sum((0, 2, 3)), i_.sum((0, 2, 3)), (r_ * r_).sum((0, 2, 3)), (i_ * i_).sum((0, 2, 3)), (r_ * i_).sum((0, 2, 3))], dim=1)
    assert relerr(res[True][1], own) < 1e-5


@pytest.mark.parametrize("F,cin,cout", [(5, 64, 64), (3, 32, 72), (9, 40, 64)])
def test_edge_data_gradient(ops, F, cin, cout):
    """The data gradient of a transposed-conv block with F input rows is the conv form on 2 F - 1 rows: an odd F lands on the edge
    workgroups.  Against the kernel below, last row alone included."""
    g = torch.Generator().manual_seed(12 + F)
    dev = "cuda"
    wr, wi = (torch.randn(cin, cout, 5, 2, generator=g) * 0.1).to(dev), (torch.randn(cin, cout, 5, 2, generator=g) * 0.1).to(dev)
    Fo = 2 * F - 1
    assert ops.L.lib().idv_cconv_tw2_supported(cout, cin, Fo)
    dy = ops.Planar.from_tensor5(torch.randn(3, cout, Fo, 37, 2, generator=g).to(dev), 38)
    d = {}
    with _Routes(ops):
        ops.WINO = ops.TW = True
        for tw in (True, False):
            ops.TW_CONV = tw
            ga = ops.pack_cconv_gauss(wr, wi, None, None, None, adjoint_of=(cin, cout, cout, False))
            ops.LAUNCH_LOG = []
            d[tw] = ops.cconv_dgrad(dy, None, None, cin, True, True, gauss=ga).tensor5().cpu()
            assert _tw2_ran(ops) == tw
    assert d[True].shape[2] == F
    e, e_last = relerr(d[True], d[False]), relerr(d[True][:, :, -1], d[False][:, :, -1])
    print(f"data gradient on the conv form vs the kernel below: all rows {e:.2e}, last row {e_last:.2e}")
    assert e < 5e-6 and e_last < 5e-6
