"""The weight-gradient kernels (csrc/wgrad.hip, csrc/wgrad_bf16.hip) against the float64 reference of their contraction
(tests/wgrad_ref.py, itself checked against oracle autograd in tests/test_wgrad_ref_host.py).  Every case calls the C-ABI entry
directly, so the test and not ops.PRECISION or the widths chooses the kernel, and runs twice:

  exact   integer inputs in [-3, 3].  Every Gauss sum, Winograd operand, product (<= 144), partial sum and the 1/2 of the Winograd
          unpack is exact in fp32 while sums stay below 2^24 (the largest case reaches about 2e6), and the integers are exact in
          a bf16 `hi` with `lo` = 0: the result must EQUAL the reference, for all five entries.  No tolerance: any wrong index,
          mask, sign, tap factor or split boundary changes an integer.
  normal  standard-normal inputs, relative L2 error of every (tap) x (re | im) x (16 S-side channels) x (16 L-side channels) block
          against that block's reference norm: GTOL = 2e-4 for the fp32 entries, 1e-3 for bf16x3 (the gradient tolerances of
          tests/test_gpu_backward.py).  The worst block is printed (DESIGN.md 3.5 carries the measured values).

In every case: dw is pre-filled (7.0, and -7.0 in the repeat call, so an entry no call writes differs between the two) and must
keep the fill outside [ci_off, ci_off + Cx); the workspace has exactly the sizer's size with 1024 sentinel floats behind it; one
float less is IDV_EINVAL with dw untouched; the pitch-padding columns [J, Jp) of both operands poisoned with 1e30 do not change a
bit; a second call returns the same bits.  The mid-tile cases assert, with the Python mirror of the split plan and the device's
compute-unit count, that a split boundary falls inside a column tile."""
import pytest
import torch

import wgrad_ref as R

pytestmark = pytest.mark.gpu
GTOL, BF16_TOL, CROSS_TOL = 2e-4, 1e-3, 2e-5          # GTOL / bf16x3 bound of test_gpu_backward.py; Gauss against four-product
SENTINEL, GUARD, POISON = -12345.0, 1024, 1e30
KINDS = ["exact", "normal"]


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def draw(kind, shape, g):
    if kind == "exact":
        return torch.randint(-3, 4, shape, generator=g, device="cuda").float()
    return torch.randn(shape, generator=g, device="cuda")


def ceil64(n):
    return (n + 63) // 64 * 64


# ----------------------------------------------------------------------------- conv entries
CONV_ENTRY = {"four": "idv_cconv2d_bwd_weight", "gauss": "idv_cconv2d_bwd_weight_gauss", "bf16": "idv_cconv2d_bwd_weight_bf16x3"}


def conv_work_floats(ops, entry, case, x, dy):
    L = ops.L
    transposed, cx, cout, _, _, fin, _, B, _ = case
    cs, cl = R.conv_geometry(case)[:2]
    if entry == "gauss":
        return int(ops._ll_fn("idv_cconv_wgrad_gauss_work_floats")(L.i(cx), L.i(cout), L.i(int(transposed)), L.i(fin), L.i(B), L.i(x.Tp),
                                                                   L.i(x.Jp), L.i(dy.Jp)))
    name = "idv_cconv_wgrad_bf16_work_floats" if entry == "bf16" else "idv_cconv_wgrad_work_floats"
    return int(ops._ll_fn(name)(L.i(cs), L.i(cl), L.i(B), L.i(x.Tp)))


def conv_call(ops, entry, case, x, dy, n, fill, short=0):
    """One call with a workspace of exactly n floats + sentinels -> (dw_re, dw_im); sentinels and untouched entries asserted.
    short: floats withheld from the size passed; the entry must then answer IDV_EINVAL and write nothing at all."""
    L = ops.L
    transposed, cx, cout, cin_total, ci_off, fin, _, B, causal = case
    tshift = -1 if (causal or transposed) else 0
    shape = (cin_total, cout, 5, 2) if transposed else (cout, cin_total, 5, 2)
    work = torch.full((n + GUARD,), SENTINEL, device="cuda")
    dwr, dwi = torch.full(shape, fill, device="cuda"), torch.full(shape, fill, device="cuda")
    args = (CONV_ENTRY[entry], x.ptr(), L.i(cx), L.i(ci_off), dy.ptr(), L.i(cout), L.i(cin_total), L.i(int(transposed)), L.i(tshift),
            L.i(fin), L.i(B), L.i(x.Tp), L.i(x.Jp), L.i(dy.Jp), L.p(work), L.ll(n - short), L.p(dwr), L.p(dwi), L.stream_ptr())
    if short:
        with pytest.raises(L.IdvError, match="status -1"):
            L.call(*args)
        torch.cuda.synchronize()
        assert bool((work == SENTINEL).all()) and bool((dwr == fill).all()) and bool((dwi == fill).all())
        return None
    L.call(*args)
    torch.cuda.synchronize()
    assert bool((work[n:] == SENTINEL).all()), "the entry wrote behind the workspace size its sizer returns"
    for dw in (dwr, dwi):
        rest = dw.clone()
        inside(rest, case).fill_(fill)
        assert bool((rest == fill).all()), "entries outside [ci_off, ci_off + Cx) were written"
    return dwr, dwi


def inside(dw, case):
    transposed, cx, ci_off = case[0], case[1], case[4]
    return dw[ci_off:ci_off + cx] if transposed else dw[:, ci_off:ci_off + cx]


def poison_padding(t, J):
    t.data.view(2 * t.C * t.F, t.Jp)[:, J:] = POISON


def conv_case(ops, entry, case, kind, tol, seed):
    """All the checks of one (entry, case, kind) -> (dw_re, dw_im) of the entry, sliced to the case's channels, the reference and
    the operands."""
    transposed, cx, cout, _, _, fin, T, B, causal = case
    _, _, _, fout, tout, tp, J = R.conv_geometry(case)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x5, dy5 = draw(kind, (B, cx, fin, T, 2), g), draw(kind, (B, cout, fout, tout, 2), g)
    x, dy = ops.Planar.from_tensor5(x5, tp), ops.Planar.from_tensor5(dy5, tp)
    assert x.Jp == dy.Jp == (J + 3) // 4 * 4 and x.B * x.Tp == J
    ref = R.conv_wgrad_ref(x5, dy5, transposed, causal)
    n = conv_work_floats(ops, entry, case, x, dy)
    first = conv_call(ops, entry, case, x, dy, n, 7.0)
    again = conv_call(ops, entry, case, x, dy, n, -7.0)
    for a, b in zip(first, again):
        assert torch.equal(inside(a, case), inside(b, case)), "a second call differs (or an entry is written by neither)"
    # one float less: IDV_EINVAL, nothing launched
    conv_call(ops, entry, case, x, dy, n, 7.0, short=1)
    if J % 4:
        poison_padding(x, J)
        poison_padding(dy, J)
        for a, b in zip(first, conv_call(ops, entry, case, x, dy, n, 7.0)):
            assert torch.equal(a, b), "the pitch-padding columns [J, Jp) reach the result"
    got = tuple(inside(a, case).double() for a in first)
    compare(f"{CONV_ENTRY[entry]} {kind}", got, ref, kind, tol)
    return got, ref, (x, dy)


def compare(what, got, ref, kind, tol):
    if kind == "exact":
        assert float(ref[0].abs().max()) < 2 ** 24 and float(ref[1].abs().max()) < 2 ** 24
        for part, a, b in zip(("re", "im"), got, ref):
            bad = (a != b).nonzero()
            assert bad.numel() == 0, f"{what} dw_{part}: {bad.shape[0]} of {a.numel()} entries differ, first at (s, l, kf, kt) = " \
                                     f"{bad[0].tolist()}: {float(a[tuple(bad[0])])} != {float(b[tuple(bad[0])])}"
        return
    worst = 0.0
    for a, b in zip(got, ref):
        w, stray = R.worst_block_error(a, b)
        assert stray == 0, f"{what}: {stray} non-zero entries where the reference block is exactly zero"
        worst = max(worst, w)
    print(f"{what}: worst block error {worst:.2e} (bound {tol:.0e})")
    assert worst <= tol, f"{what}: worst block error {worst:.3e} > {tol:.0e}"


def assert_mid_tile(name, entry, case, cus):
    args = R.conv_plan_args(entry, case)
    count = lambda a: R.mid_tile_boundaries(R.split_bounds(*R.plan_rounds(*a, cus), a[8]), a[8])
    if count(args) >= 1:
        return
    B, other = case[7], []
    for T in range(max(case[6] - 200, 8), case[6] + 200):
        if count(args[:2] + (B * (T + 1),) + args[3:]) >= 1:
            other.append(B * (T + 1))
    near = sorted(other, key=lambda j: abs(j - args[2]))[:4]
    pytest.fail(f"{name}: on {cus} compute units no split boundary of J = {args[2]} falls inside a column tile; use J in {near}")


def check_sizer_against_mirror(ops, entry, case, x, dy, cus):
    """The sizer's figure from the Python mirror of the plan at this device's compute-unit count."""
    args = R.conv_plan_args(entry, case)
    n = conv_work_floats(ops, entry, case, x, dy)
    cs, cl, fs = R.conv_geometry(case)[:3]
    SpPad, LpPad = -(-args[0] // 128) * 128, -(-args[1] // 32) * 32
    if entry == "four":
        assert n == R.plan_rounds(*args[:8], 0, cus)[0] * 10 * SpPad * LpPad
    else:
        planes = 14 if fs >= R.WINO_MIN_ROWS else 10
        assert n == 3 * R.plan_rounds(*args, cus)[0] * planes * SpPad * LpPad + ceil64(cs * fs * x.Jp) + ceil64(cl * (2 * fs - 1) * x.Jp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(R.FOUR_CASES))
def test_four_product_entry(ops, cus, name, kind):
    case = R.FOUR_CASES[name]
    if name in R.MID_TILE:
        assert_mid_tile(name, "four", case, cus)
    got, ref, (x, dy) = conv_case(ops, "four", case, kind, GTOL, 101)
    if R.conv_plan_args("four", case) is not None:
        check_sizer_against_mirror(ops, "four", case, x, dy, cus)
    if name in ("A7t", "A7c"):                          # one frequency row: every tap but kf = 2 is zero
        for a in got:
            assert float(a[:, :, [0, 1, 3, 4]].abs().max()) == 0.0 and float(a[:, :, 2].abs().max()) > 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(R.GAUSS_CASES))
def test_gauss_entry(ops, cus, name, kind):
    """Ten-product form below 8 S rows, the two Winograd kernels from 8 rows up; normal inputs: also block-wise against the
    four-product entry on the same operands (2e-5, the bound of test_wgrad_gauss_matches_four_product_kernel)."""
    L = ops.L
    case = R.GAUSS_CASES[name]
    cs, cl = R.conv_geometry(case)[:2]
    assert L.lib().idv_cconv_wgrad_gauss_supported(L.i(cs), L.i(cl))
    if name in R.MID_TILE:
        assert_mid_tile(name, "gauss", case, cus)
    got, ref, (x, dy) = conv_case(ops, "gauss", case, kind, GTOL, 202)
    check_sizer_against_mirror(ops, "gauss", case, x, dy, cus)
    if kind == "normal":
        # the same operands (padding columns still poisoned where J % 4 != 0)
        four = conv_call(ops, "four", case, x, dy, conv_work_floats(ops, "four", case, x, dy), 7.0)
        worst = 0.0
        for a, b in zip(got, four):
            w, stray = R.worst_block_error(a, inside(b, case).double())
            assert stray == 0
            worst = max(worst, w)
        print(f"Gauss entry against the four-product entry: worst block {worst:.2e} (bound {CROSS_TOL:.0e})")
        assert worst <= CROSS_TOL


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(R.BF16_CASES))
def test_split_bf16_entry(ops, name, kind):
    conv_case(ops, "bf16", R.BF16_CASES[name], kind, BF16_TOL, 303)


# ----------------------------------------------------------------------------- point-wise entries and the bias row sums
def pw_call(ops, fn, case, dout, x, Jp, n, dw0, short=0):
    L = ops.L
    M, K, J, shift, rowmap, H, accumulate, ldw = case
    work = torch.full((n + GUARD,), SENTINEL, device="cuda")
    dw = dw0.clone()
    args = (fn, L.p(dout), L.i(M), L.i(Jp), L.p(x), L.i(K), L.i(Jp), L.i(J), L.i(shift), L.p(work), L.ll(n - short), L.p(dw), L.i(ldw),
            L.i(rowmap), L.i(H), L.i(accumulate), L.stream_ptr())
    if short:
        with pytest.raises(L.IdvError, match="status -1"):
            L.call(*args)
        torch.cuda.synchronize()
        assert bool((work == SENTINEL).all()) and torch.equal(dw, dw0)
        return None
    L.call(*args)
    torch.cuda.synchronize()
    assert bool((work[n:] == SENTINEL).all()), "the entry wrote behind the workspace size its sizer returns"
    assert torch.equal(dw[:, K:], dw0[:, K:]), "columns [K, ldw) were written"
    return dw


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(R.PW_CASES))
@pytest.mark.parametrize("fn,tol", [("idv_pw_bwd_weight", GTOL), ("idv_pw_bwd_weight_bf16x3", BF16_TOL)])
def test_pointwise_entries(ops, fn, tol, name, kind):
    L = ops.L
    case = R.PW_CASES[name]
    M, K, J, shift, rowmap, H, accumulate, ldw = case
    Jp = (J + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(404)
    dout, x = torch.zeros(M, Jp, device="cuda"), torch.zeros(K, Jp, device="cuda")
    dout[:, :J], x[:, :J] = draw(kind, (M, J), g), draw(kind, (K, J), g)
    ref = R.pw_wgrad_ref(dout[:, :J], x[:, :J], shift, rowmap, H)
    n = int(ops._ll_fn("idv_pw_wgrad_work_floats")(L.i(M), L.i(K), L.i(J)))
    fills = [draw(kind, (M, ldw), g)] * 2 if accumulate else [torch.full((M, ldw), v, device="cuda") for v in (7.0, -7.0)]
    first, again = (pw_call(ops, fn, case, dout, x, Jp, n, f) for f in fills)
    assert torch.equal(first[:, :K], again[:, :K]), "a second call differs (or an entry is written by neither)"
    pw_call(ops, fn, case, dout, x, Jp, n, fills[0], short=1)
    if J % 4:
        dout[:, J:], x[:, J:] = POISON, POISON
        assert torch.equal(first, pw_call(ops, fn, case, dout, x, Jp, n, fills[0])), "the pitch-padding columns [J, Jp) reach the result"
    want = ref + fills[0][:, :K].double() if accumulate else ref
    got = first[:, :K].double()
    if kind == "exact":
        assert float(want.abs().max()) < 2 ** 24
        bad = (got != want).nonzero()
        assert bad.numel() == 0, f"{fn}: {bad.shape[0]} of {got.numel()} entries differ, first at (row, k) = {bad[0].tolist()}"
        return
    worst, stray = R.worst_block_error(got, want)
    print(f"{fn} normal: worst block error {worst:.2e} (bound {tol:.0e})")
    assert stray == 0 and worst <= tol


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,J", R.ROWSUM_CASES)
def test_planar_rowsum(ops, M, J, accumulate, kind):
    L = ops.L
    Jp = (J + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(505)
    x = torch.zeros(M, Jp, device="cuda")
    x[:, :J] = draw(kind, (M, J), g)
    out0 = draw(kind, (M + 8,), g)                      # eight floats behind the M rows must stay
    want = x[:, :J].double().sum(dim=1) + (out0[:M].double() if accumulate else 0.0)
    outs = []
    for poison in (False, True):
        if poison:
            x[:, J:] = POISON
        out = out0.clone()
        L.call("idv_planar_rowsum", L.p(x), L.i(M), L.i(Jp), L.i(J), L.i(accumulate), L.p(out), L.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out[M:], out0[M:])
        outs.append(out[:M])
    assert torch.equal(outs[0], outs[1]), "the pitch-padding columns [J, Jp) reach the result (or a second call differs)"
    if kind == "exact":
        assert torch.equal(outs[0].double(), want)
    else:
        err = float((outs[0].double() - want).norm() / want.norm())
        print(f"idv_planar_rowsum normal: relative error {err:.2e} (bound {GTOL:.0e})")
        assert err <= GTOL
