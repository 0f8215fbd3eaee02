"""tests/cbn_ref.py, the float64 reference that tests/test_gpu_cbn.py judges the batch-norm kernels by, checked on the CPU: its
forward against the oracle, its closed-form backward (the mirror of the three backward kernels) against torch autograd, and the
conditions that the drawn inputs meet by construction -- asserted here per case and seed, so that no GPU test has to mask an
element out."""
import pytest
import torch

import cbn_ref as R
from oracle import idccrn_oracle as O

NORMAL = [c for c in R.CASES + R.FINALIZE_CASES if c.kind == "normal"]
EXACT = [c for c in R.CASES if c.kind == "exact"]
ids = lambda cases: [c.name for c in cases]


def to5(v):
    """[2, C, F, B, T] -> the oracle's [B, C, F, T, 2]."""
    return v.permute(3, 1, 2, 4, 0)


@pytest.mark.parametrize("case", NORMAL, ids=ids(NORMAL))
def test_forward_matches_oracle(case):
    d = R.draw(case)
    y, slope = d["y"], case.slope
    m, run, fo = R.finalize(R.moment_sums(y), case.count, d["gam"], d["beta"])
    st = O.cbn_batch_stats(to5(y))
    for k, name in enumerate(("mean_r", "mean_i", "Vrr", "Vri", "Vii")):
        assert float((m[k] - st[k].reshape(-1)).abs().max()) < 1e-12, name
    assert torch.equal(run, m)                                              # the first call copies
    want = O.cbn_whiten_affine(to5(y), *st, *d["gam"], *d["beta"])
    if slope is not None:
        want = O.prelu(want, torch.tensor(slope, dtype=torch.float64))
    assert float((to5(R.apply(y, fo, slope)) - want).abs().max()) < 1e-12
    # the fold from the moments alone (idv_cbn_fold) is the same function
    assert torch.equal(R.fold(m, d["gam"], d["beta"]), fo)
    # a later call blends
    m2, run2, _ = R.finalize(R.moment_sums(R.draw(case, 1)["y"]), case.count, d["gam"], d["beta"], running=run, momentum=0.9)
    assert float((run2 - (0.9 * m + 0.1 * m2)).abs().max()) < 1e-12


@pytest.mark.parametrize("case", NORMAL, ids=ids(NORMAL))
def test_closed_form_backward_matches_autograd(case):
    d = R.draw(case)
    a = R.backward_closed(d["y"], d["dz"], d["gam"], d["beta"], case.slope)
    b = R.backward_autograd(d["y"], d["dz"], d["gam"], d["beta"], case.slope)
    for k, want in b.items():
        if want is None:
            assert a[k] is None
            continue
        scale = max(1.0, float(want.abs().max()))
        assert float((a[k] - want).abs().max()) < 1e-10 * scale, (k, float((a[k] - want).abs().max()))
    assert bool((a["coef"][:, 11] == 0).all())
    quarter = R.backward_closed(d["y"], d["dz"], d["gam"], d["beta"], case.slope, scale=0.25)
    assert torch.equal(quarter["dy"], a["dy"]) and torch.allclose(quarter["dgamma_ri"], 0.25 * a["dgamma_ri"], rtol=1e-15, atol=0)


@pytest.mark.parametrize("case", NORMAL, ids=ids(NORMAL))
@pytest.mark.parametrize("salt", [0, 1])
def test_normal_inputs_are_well_conditioned(case, salt):
    """Smaller eigenvalue of every channel's covariance >= 0.1, eigenvalue ratio <= 10 (the whitening gradient does not amplify
    rounding); Vri and the means are not zero; no |u| below 1e-4 (the fp32 u is within about 1e-6 of the float64 one, so no element
    can change its PReLU branch)."""
    d = R.draw(case, salt)
    m, _, fo = R.finalize(R.moment_sums(d["y"]), case.count, d["gam"], d["beta"])
    lo, hi = R.cov_eigen(m)
    assert float(lo.min()) >= 0.1 and float((hi / lo).max()) <= 10.0, (float(lo.min()), float((hi / lo).max()))
    assert float(m[3].abs().min()) > 1e-3 and float(d["gam"][1].abs().min()) >= 0.05
    if case.C > 1:
        assert float(m[:2].abs().max()) > 0.5
    if salt == 0:
        assert float(R.pre_activation(d["y"], fo).abs().min()) >= 1e-4


def _grid(t, step, limit):
    return bool((t * step == (t * step).round()).all()) and float(t.abs().max()) < limit


@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_exact_inputs_are_exact(case):
    """Every intermediate value and every sum of the exact kind is an integer below 2^24 in magnitude or a multiple of 1/4 below
    2^22, so fp32 and double arithmetic in any order, fused or not, give the same bits -- with one exception: the forward's
    slope * u is 1/4 of a multiple of 1/2, a multiple of 1/8, held below 2^21 instead.  Every PReLU case has kept elements with
    u == 0, u > 0 and u < 0."""
    d = R.draw(case)
    y, dz, fo, coef, slope = d["y"], d["dz"], d["fold"], d["coef"], case.slope
    assert _grid(y, 1, 4) and _grid(dz, 1, 4) and _grid(fo[:, :4], 2, 2.5) and _grid(fo[:, 4:], 1, 4) and _grid(coef, 1, 3)
    assert all(float(z) in R.Z_SET for z in fo[:, :4].reshape(-1)) and bool((coef[:, 11] == 0).all())
    u = R.pre_activation(y, fo)
    if slope is not None:
        assert slope == 0.25
        assert bool((u == 0).any()) and bool((u > 0).any()) and bool((u < 0).any())
    yr, yi = y[0], y[1]
    for k in (0, 1, 2, 3):                                       # the products and partial sums of u
        assert _grid(R._col(fo, k) * (yr if k % 2 == 0 else yi), 4, 2 ** 22)
    assert _grid(R._col(fo, 0) * yr + R._col(fo, 1) * yi, 4, 2 ** 22) and _grid(R._col(fo, 2) * yr + R._col(fo, 3) * yi, 4, 2 ** 22)
    assert _grid(u, 4, 2 ** 22) and _grid(R.apply(y, fo, slope), 8, 2 ** 21)
    assert _grid(R.moment_sums(y), 1, 2 ** 24)
    du = R.du_of(dz, u, slope)
    assert _grid(du, 4, 2 ** 22) and _grid(dz * u, 4, 2 ** 22)
    for a in du:
        for b in y:
            assert _grid(a * b, 4, 2 ** 22)
    assert _grid(R.bwd_sums(dz, y, fo, slope), 4, 2 ** 22)
    tr, ti = R.bwd_terms(dz, y, fo, coef, slope)
    for terms in (tr, ti):
        acc = torch.zeros_like(terms[0])
        for t in terms:                                          # every term and every partial sum, in the kernel's order
            acc = acc + t
            assert _grid(t, 4, 2 ** 22) and _grid(acc, 4, 2 ** 22)
    # what the split image holds in its hi plane alone: 8 significant bits
    for v in (R.apply(y, fo, slope), R.bwd_apply(dz, y, fo, coef, slope)):
        f = v.float()
        assert torch.equal((f.view(torch.int32) & 0xFFFF).count_nonzero(), torch.tensor(0))


def test_exact_conv_case_is_exact():
    d = R.draw_conv()
    out = R.cconv(d["x"], d["w_re"], d["w_im"], d["b_re"], d["b_im"])
    c = R.CONV
    assert out.shape == (2, c["cout"], (c["F"] - 1) // 2 + 1, c["B"], c["T"])
    assert _grid(out, 1, 2 ** 24) and _grid(R.moment_sums(out), 1, 2 ** 53)
    # against the oracle's conv
    x5 = to5(d["x"])
    want = O.complex_conv2d(x5, d["w_re"], d["b_re"], d["w_im"], d["b_im"], (2, 1), (2, 1), True)
    assert torch.equal(to5(out), want)
    # each channel's sums are told apart: no two channels share their five sums
    s = R.moment_sums(out)
    assert len({tuple(r.tolist()) for r in s}) == c["cout"]


def test_bias_grad_and_layout_helpers():
    s = torch.tensor([[1.0, 2.0, 0, 0, 0], [-3.0, 0.5, 0, 0, 0]], dtype=torch.float64)
    re, im = R.bias_grad(s)
    assert re.tolist() == [3.0, -2.5] and im.tolist() == [1.0, 3.5]
    case = R.BY_NAME["e_c5"]
    v = R.draw(case)["y"]
    plane = torch.full((2 * case.C * case.F + 2, case.Jp), 7.0, dtype=torch.float64)
    R.place(plane, v, case.Tp)
    assert torch.equal(R.read(plane, case.C, case.F, case.B, case.T, case.Tp), v)
    g = R.guard_mask(case.B, case.T, case.Tp)
    assert int(g.sum()) == case.B * (case.Tp - case.T) and bool((plane[:2 * case.C * case.F, :case.B * case.Tp][:, g] == 7.0).all())
    assert case.Jp >= case.B * case.Tp and case.Jp % 4 == 0 and R.BY_NAME["e_c4_t33"].Jp == 3 * 34 + 2 + 8


def test_case_tables_reach_every_mechanism():
    cs = R.CASES
    assert {c.C for c in cs} == {1, 4, 5} and {c.F for c in cs} == {1, 3} and {c.B for c in cs} == {1, 3}
    assert {1, 2, 33} <= {c.T for c in cs} and {c.pad for c in cs} == {1, 3} and {c.spare for c in cs} == {0, 8}
    assert R.BY_NAME["e_cap16"].Tp == 4100 > 16 * 256 and R.BY_NAME["e_cap64"].Tp == 16390 > 64 * 256
    assert R.BY_NAME["e_cap64_c4"].Tp == 16390 and R.BY_NAME["e_cap64_c4"].C == 4
    assert any(c.C > 256 for c in R.FINALIZE_CASES)
    for kind in ("exact", "normal"):
        assert any(c.kind == kind and not c.prelu for c in cs) and any(c.kind == kind and c.prelu and c.C == 4 for c in cs)
    assert all(c.count >= 9 for c in cs if c.kind == "normal")
