"""Odd-row phase of the time-Winograd transposed conv (csrc/cgemm_tw.hip) on the vector weight layout: both row phases take their
weights as 16-byte loads from groups of [64 lanes][4 slots].

Pack layout.  idv_pack_cconv_tw on a buffer of distinct random floats in place of cgemm_wino's fragments, Cout = 40 (two co tiles, the
second ragged) and cin_used = 10 (channels 10 .. 15 of the pack granularity empty), against a numpy gather written here from the
definition in the kernel's header comment: per (co tile, channel pair u, wave w) slot k holds tile tw_tile(phase, w, k) = (frequency
product r, Gauss plane g, time product tau) with tau 0 / 1 / 2 = W_h0 / W_h0 + W_h1 / W_h1, lane = channel parity x 32 + co; slots 0 .. 7
as two groups of [64 lanes][4 slots], the even-row phase's slot 8 as [64 lanes]; zero in the odd-row phase's slot 7, in its wave 3's
slot 6 and for channels past cin_used; the third region the raw taps W4 (waves 0, 2) and W2 = product 1 - product 2 (waves 1, 3) in the
even-row phase's layout.  Element for element: the sums are single fp32 additions.

Conv.  Tiny shapes through ops.cconv2d(..., gauss=pack) with the time-Winograd route on and off (the kernel below: cgemm_wino, or
cgemm_gauss for one co tile): odd output rows on their own and all rows within test_ctconv_time_winograd's 5e-6.  Fin 2 (one odd row), 3
(a row tile whose second odd row is past the end), 5 (two row tiles); J = B Tp = 64 (one column block) and 129 (three, the last
ragged); 8 channels, 8 + a skip source of 3 (ragged second K chunk), 16; Cout 32 (one co tile per workgroup), 64 (paired), 40 (paired,
ragged second co tile); both tap sides; fold + PReLU; an addend; the train-mode moment sums.  Paired against unpaired: bit-identical."""
import numpy as np
import pytest
import torch

from conftest import relerr
from test_gpu_ops import _conv_case

pytestmark = pytest.mark.gpu
PAIR_ALL = 7
TOL = 5e-6


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


class _Routes:
    """ops' route switches, pair mask and launch log restored afterwards."""

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


# ---------------------------------------------------------------------------------------------------------------- pack layout
def _tw_tile(ph, w, k):
    """(r, plane) of slot k of wave w, or None: the kernel's header comment (tw_tile)."""
    if ph == 0:
        return (w, k)                                           # wave = frequency product, its nine planes
    if k >= 7:
        return None
    if w < 3:
        return (w, k if k < 6 else 8)                           # planes 0 .. 5 and 8 of product w
    return (k >> 1, 6 + (k & 1)) if k < 6 else None             # wave 3: planes 6, 7 of the three products


def _expected_pack(wino, cotiles, cpad, cin_used):
    """wino: [2 phases][cotiles][cpad * 3 units][4 slots][64 lanes = h * 32 + co] -> the three regions, flat."""
    UP = cpad // 2
    out = []
    for region in (0, 1, 2):                                    # even rows, odd rows, raw taps of the edge workgroups
        ph, raw = (1 if region == 1 else 0), region == 2
        ws = 8 if ph else 9
        reg = np.zeros((cotiles, UP, 4, ws * 64), dtype=np.float32)
        for ct in range(cotiles):
            for u in range(UP):
                for w in range(4):
                    for k in range(ws):
                        tile = _tw_tile(ph, w, k)
                        for ln in range(64):
                            ci, co = 2 * u + (ln >> 5), ln & 31
                            pos = (k >> 2) * 256 + ln * 4 + (k & 3) if k < 8 else 512 + ln
                            if tile is None or ci >= cin_used:
                                continue                        # zero taps
                            r, plane = tile
                            g, tau = plane // 3, plane % 3
                            src = wino[ph, ct, ci * 3 + g]      # [4 slots][64]
                            if raw:
                                w0, w1 = (src[1, co] - src[2, co], src[1, 32 + co] - src[2, 32 + co]) if (r & 1) else (src[0, co], src[0, 32 + co])
                            else:
                                w0, w1 = src[r, co], src[r, 32 + co]
                            reg[ct, u, w, pos] = w0 if tau == 0 else (np.float32(w0 + w1) if tau == 1 else w1)
        out.append(reg.reshape(-1))
    return out


def test_pack_layout_against_the_definition(ops):
    cout, cin_used = 40, 10
    cotiles, cpad = 2, 16
    lib = ops.L.lib()
    n_wino = int(lib.idv_cconv_wino_wfrag_floats(1, cout, cin_used))
    assert n_wino == 2 * cotiles * cpad * 3 * 4 * 64
    rng = np.random.default_rng(5)
    host = (rng.permutation(n_wino).astype(np.float32) + np.float32(0.5)) / np.float32(64.0) - np.float32(300.0)   # distinct, none zero, sums exact
    assert (host != 0).all()
    assert len(np.unique(host)) == n_wino
    wf = torch.from_numpy(host).cuda()
    n_tw = int(lib.idv_cconv_tw_wfrag_floats(cout, cin_used))
    n0, n1 = cotiles * (cpad // 2) * 36 * 64, cotiles * (cpad // 2) * 32 * 64
    assert n_tw == n0 + n1 + n0
    tw = torch.full((n_tw + 64,), 7.0, dtype=torch.float32, device="cuda")                       # (+ a guard behind the buffer)
    ops.call("idv_pack_cconv_tw", ops.p(wf), ops.i(cout), ops.i(cin_used), ops.p(tw), ops.stream_ptr())
    torch.cuda.synchronize()
    got = tw.cpu().numpy()
    assert (got[n_tw:] == 7.0).all()
    even, odd, raw = _expected_pack(host.reshape(2, cotiles, cpad * 3, 4, 64), cotiles, cpad, cin_used)
    for name, lo, want in (("odd-row phase", n0, odd), ("even-row phase", 0, even), ("raw taps", n0 + n1, raw)):
        part = got[lo:lo + want.size]
        bad = np.flatnonzero(part != want)
        assert bad.size == 0, (name, bad.size, bad[:8], part[bad[:8]], want[bad[:8]])
    # the odd-row phase's zero slots, seen directly: slot 7 of every wave, slot 6 of wave 3, channels 10 .. 15 (pairs 5 .. 7)
    o = got[n0:n0 + n1].reshape(cotiles, cpad // 2, 4, 2, 64, 4)
    assert (o[:, :, :, 1, :, 3] == 0).all() and (o[:, :, 3, 1, :, 2] == 0).all() and (o[:, 5:] == 0).all()
    assert (o[:, :5, :3, 0, :, 0] != 0).all()                                   # (slot 0, tau = 0: a source value as it is)


# ---------------------------------------------------------------------------------------------------------------- conv
def _shape(causal, J):
    """(T, B) with B * Tp = J as _conv_case lays the input out (Tp = output frames + 1)."""
    B = {64: 2, 129: 3}[J]
    Tp = J // B
    return (Tp - 1 if causal else Tp - 2), B


# causal, cin, skip_c, cout, F, J, fold, slope
CASES = [
    (True, 8, 0, 32, 2, 64, False, None),          # one odd row, one column block, one co tile per workgroup
    (True, 8, 0, 64, 2, 129, True, 0.25),          # ... three column blocks, paired
    (False, 8, 3, 40, 2, 64, False, 0.2),          # ... ragged second K chunk and second co tile, taps on the right
    (True, 8, 3, 32, 3, 129, True, 0.25),          # a row tile whose second odd row is past the end
    (True, 16, 0, 64, 3, 64, False, None),
    (False, 16, 0, 40, 3, 129, True, 0.1),
    (False, 8, 0, 32, 3, 64, True, 0.25),
    (True, 8, 3, 64, 3, 129, False, None),
    (True, 8, 0, 40, 5, 129, False, 0.2),          # two row tiles
    (True, 16, 0, 32, 5, 64, True, 0.25),
    (False, 8, 3, 64, 5, 129, True, 0.25),
    (True, 8, 3, 40, 5, 64, True, None),
    (False, 16, 0, 64, 5, 64, False, None),
    (False, 8, 0, 32, 5, 129, False, 0.2),
]


@pytest.mark.parametrize("causal,cin,skip_c,cout,F,J,fold,slope", CASES)
def test_odd_rows_against_the_kernel_below(ops, causal, cin, skip_c, cout, F, J, fold, slope):
    T, B = _shape(causal, J)
    assert ops.L.lib().idv_cconv_tw_supported(cin, skip_c, cout, F)
    with _Routes(ops):
        ops.WINO = ops.TW = True
        ops.LAUNCH_LOG = []
        got = _conv_case(ops, causal, True, cin, cout, F, T, B, seed=91, fold=fold, slope=slope, skip_c=skip_c, gauss=True)   # (oracle bound)
        assert _tw_ran(ops), "time-Winograd kernel not launched"
        ops.TW = False
        ops.LAUNCH_LOG = []
        ref = _conv_case(ops, causal, True, cin, cout, F, T, B, seed=91, fold=fold, slope=slope, skip_c=skip_c, gauss=True)
        assert not _tw_ran(ops)
    assert got.shape[2] == 2 * F - 1 and got.shape[0] * (max(T, got.shape[3]) + 1) == J
    e, e_odd = relerr(got, ref), relerr(got[:, :, 1::2], ref[:, :, 1::2])
    print(f"Fin {F} J {J}: time-Winograd vs the kernel below: all rows {e:.2e}, odd rows {e_odd:.2e}")
    assert e < TOL and e_odd < TOL


def _inputs(F, T, B, c0, c1, cout, seed, skip_b=None):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, c0, F, T, 2, generator=g)
    sk = torch.randn(skip_b or B, c1, F, T, 2, generator=g) if c1 else None
    shape = (c0 + c1, cout, 5, 2)
    wr, wi = (torch.randn(shape, generator=g) * 0.2).to(dev), (torch.randn(shape, generator=g) * 0.2).to(dev)
    br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    return x, sk, wr, wi, br, bi


@pytest.mark.parametrize("F,cout,J,c1", [(3, 64, 129, 8), (5, 40, 129, 3), (2, 64, 64, 8), (5, 40, 64, 8)])
def test_paired_equals_unpaired(ops, F, cout, J, c1):
    """Two co tiles per workgroup run the one-co-tile program per co tile, weights included: planes bit-identical."""
    T, B = _shape(True, J)
    x, sk, wr, wi, br, bi = _inputs(F, T, B, 8, c1, cout, seed=95 + F)
    slope = torch.tensor([0.25], device="cuda")
    xp, skp = ops.Planar.from_tensor5(x.cuda(), T + 1), ops.Planar.from_tensor5(sk.cuda(), T + 1)
    res = {}
    keep = ops.WINO, ops.TW, ops.TW_PAIR, ops.LAUNCH_LOG
    try:
        ops.WINO = ops.TW = True
        pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=True)
        for pair in (PAIR_ALL, 0):
            ops.TW_PAIR = pair
            ops.tw_pair_launches(reset=True)
            ops.LAUNCH_LOG = []
            y = ops.cconv2d(xp, None, None, cout, transposed=True, slope=slope, skip=skp, gauss=pk)
            torch.cuda.synchronize()
            assert _tw_ran(ops)
            assert ops.tw_pair_launches() == (2 if pair else 0)                 # one launch per row phase
            res[pair] = y.planes().clone()
    finally:
        ops.WINO, ops.TW, ops.TW_PAIR, ops.LAUNCH_LOG = keep
    assert torch.equal(res[PAIR_ALL], res[0]), float((res[PAIR_ALL] - res[0]).abs().max())


@pytest.mark.parametrize("F,ns,B0,T,cout", [(3, 3, 1, 42, 64), (5, 2, 1, 31, 40), (2, 3, 1, 42, 32), (5, 1, 3, 42, 64)])
def test_addend_and_moment_sums(ops, F, ns, B0, T, cout):
    """The repeated-skip addend (add_div = ns: the addend's column is that of utterance b / ns) and the train-mode moment sums, odd rows
    and all rows, against the kernel the layer runs on without the time-Winograd route."""
    c0, c1 = 8, 8
    B = B0 * ns
    assert B * (T + 1) in (64, 129)
    x, sk, wr, wi, br, bi = _inputs(F, T, B, c0, c1, cout, seed=101 + F + ns, skip_b=B0)
    dev = "cuda"
    slope = torch.tensor([0.2], device=dev)
    xp, skp = ops.Planar.from_tensor5(x.to(dev), T + 1), ops.Planar.from_tensor5(sk.to(dev), T + 1)
    sk_rep = ops.Planar.from_tensor5(sk.repeat_interleave(ns, dim=0).to(dev), T + 1)
    res = {}
    with _Routes(ops):
        ops.WINO = True
        for tw in (True, False):
            ops.TW = tw
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
            torch.cuda.synchronize()
            res[tw] = (y.tensor5().cpu(), yt.tensor5().cpu(), st.cpu())
    for k, what in enumerate(("addend output", "train-mode output", "moment sums")):
        e = relerr(res[True][k], res[False][k])
        print(f"{what}: {e:.2e}")
        assert e < TOL
    for k, what in enumerate(("addend output", "train-mode output")):
        e = relerr(res[True][k][:, :, 1::2], res[False][k][:, :, 1::2])
        print(f"{what}, odd rows: {e:.2e}")
        assert e < TOL
    # the sums are those of the outputs
    t5 = res[True][1].double()
    r_, i_ = t5[..., 0], t5[..., 1]
    own = torch.stack([r_.sum((0, 2, 3)), i_.sum((0, 2, 3)), (r_ * r_).sum((0, 2, 3)), (i_ * i_).sum((0, 2, 3)), (r_ * i_).sum((0, 2, 3))], dim=1)
    assert relerr(res[True][2], own) < TOL
