"""Global gradient norm, clipping and the non-finite guard on the bucket (csrc/bucket.hip idv_bucket_sqnorm / idv_bucket_clip_finalize /
idv_bucket_adam_clipped / idv_bucket_scale; optim.Adam(max_norm, skip_nonfinite), optim.clip_grad_norm_).

Parameters: the shapes of tests/test_gpu_optim.py -- a one-element tensor, padding behind a tensor, a partial last group, a tensor
that spans many workgroups -- plus a 1000-element gradient that starts 4 bytes into an allocation (the scalar path); parameter 4
never has a gradient.  Bounds:
  * integer gradients: every square and every partial sum is an integer below 2^53, so sumsq is exact;
  * random gradients: |norm - ref| <= n 2^-53 ref against tests/clip_ref.py, the worst case of a double sum of n exact squares
    (relative error (n - 1) 2^-53 on sumsq, half of it on the root), n = the element count; coef within one float32 ulp;
  * the Adam step against clip_grad_norm_ + torch.optim.Adam: the bars of test_gpu_optim.test_adam_matches_torch_adam, 2e-6 of
    the parameter scale and 1e-6 of the moments' scale."""
import importlib
import math

import pytest
import torch

import clip_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3, 5), (257,), (64, 32, 5, 2), (2,), (1024, 1280), (7, 1, 1), (1000,)]
NOGRAD = 4                                            # the parameter that never receives a gradient
UNALIGNED = 7                                         # its gradient is a view that starts 4 bytes into an allocation
NUMEL = sum(math.prod(s) for k, s in enumerate(SHAPES) if k != NOGRAD)
# (parameter, flat index) of a bad value: the last partial group of (257,), the unaligned tensor, the middle of (1024, 1280)
BAD_AT = {"partial_group": (2, 256), "unaligned": (UNALIGNED, 501), "middle": (5, 512 * 1280 + 640)}


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module("i-dccrn-vae_amd.optim")


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.3).cuda()) for s in SHAPES]


def _clone(ps):
    return [torch.nn.Parameter(q.detach().clone()) for q in ps]


def _host_grads(seed, integer=False):
    """CPU gradients of one step (None for NOGRAD), at the two magnitudes test_gpu_optim._set_grads uses."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, s in enumerate(SHAPES):
        x = torch.randint(-3, 4, s, generator=g).float() if integer else torch.randn(*s, generator=g) * (0.5 if k % 2 else 2e-3)
        out.append(None if k == NOGRAD else x)
    return out


def _put(ps, grads):
    for k, (q, x) in enumerate(zip(ps, grads)):
        if x is None:
            q.grad = None
        elif k == UNALIGNED:
            base = torch.empty(x.numel() + 1, device="cuda")
            base[1:].copy_(x)
            q.grad = base[1:]
            assert q.grad.data_ptr() % 16 != 0
        else:
            q.grad = x.cuda()


def _close(ours, ref, bar):
    ours, ref = ours.detach(), ref.detach()
    return float((ours - ref).abs().max()) <= bar * float(ref.abs().max())


def _check_against_torch(oa, a, ob, b, steps):
    for k, (q, r) in enumerate(zip(a, b)):
        assert _close(q, r, 2e-6), (k, float((q - r).abs().max()))
        if k == NOGRAD:
            assert torch.equal(q, r) and q not in oa.state
        else:
            assert _close(oa.state[q]["exp_avg"], ob.state[r]["exp_avg"], 1e-6), k
            assert _close(oa.state[q]["exp_avg_sq"], ob.state[r]["exp_avg_sq"], 1e-6), k
            assert float(oa.state[q]["step"]) == float(ob.state[r]["step"]) == float(steps)


def _norms(seeds):
    return [math.sqrt(clip_ref.sumsq(_host_grads(s))) for s in seeds]


def _between(norms, k):
    """A max_norm between the k-th and the (k+1)-th smallest norm: k steps stay as they are, the others clip."""
    s = sorted(norms)
    return 0.5 * (s[k - 1] + s[k])


# ------------------------------------------------------------------------------------------------ 1. exact
def test_integer_gradients_sum_exactly_and_padding_is_never_read(optim):
    ps = _params(1)
    grads = _host_grads(2, integer=True)
    _put(ps, grads)
    want = float(sum(int((x.long() ** 2).sum()) for x in grads if x is not None))
    tab = optim.TensorTable([q.numel() for q in ps], ps[0].device)
    dev_grads = [q.grad for q in ps]
    run = optim._NormPass(ps[0].device)
    gtable = tab.table(dev_grads)
    run.run([(gtable, gtable, None, tab.n, tab.total, 1.0)], None, False)
    first = run.record.buf.clone()
    assert float(run.record.sumsq) == want and abs(float(run.record.norm) - math.sqrt(want)) <= 2.0 ** -52 * math.sqrt(want)
    assert float(run.record.coef) == 1.0 and int(run.record.finite) == 1 and int(run.record.skipped) == 0
    run.run([(gtable, gtable, None, tab.n, tab.total, 1.0)], None, False)
    assert torch.equal(run.record.buf, first)
    # the same gradients times 4 in a bucket, scale 0.25; NaN in every padding element and in the absent parameter's range
    flat = tab.flat()
    optim.bucket_gather(tab, dev_grads, flat)
    flat.mul_(4.0)
    keep = torch.zeros(tab.total, dtype=torch.bool, device="cuda")
    for k, (o, n) in enumerate(zip(tab.offsets, tab.numels)):
        if k != NOGRAD:
            keep[o:o + n] = True
    assert int((~keep).sum()) == 3 + 1 + 3 + 4 + 1       # the padding behind the odd sizes and NOGRAD's whole group
    clean = flat.clone()
    flat[~keep] = float("nan")
    ptab = optim.TensorTable(tab.numels, ps[0].device)
    ptable = ptab.table([None if k == NOGRAD else q for k, q in enumerate(ps)])
    run2 = optim._NormPass(ps[0].device)
    run2.run([(ptable, None, flat, tab.n, tab.total, 0.25)], None, False)
    assert float(run2.record.sumsq) == want and int(run2.record.finite) == 1
    poisoned = run2.record.buf.clone()
    run2.run([(ptable, None, clean, tab.n, tab.total, 0.25)], None, False)
    assert torch.equal(run2.record.buf, poisoned) and torch.equal(run2.record.buf, first)


# ------------------------------------------------------------------------------------------------ 2. float64 parity
@pytest.mark.parametrize("seed", [3, 4])
def test_norm_and_coefficient_against_float64(optim, seed):
    ps = _params(1)
    grads = _host_grads(seed)
    _put(ps, grads)
    ref = math.sqrt(clip_ref.sumsq(grads))
    max_norm = 0.37 * ref
    tab = optim.TensorTable([q.numel() for q in ps], ps[0].device)
    gtable = tab.table([q.grad for q in ps])
    run = optim._NormPass(ps[0].device)
    run.run([(gtable, gtable, None, tab.n, tab.total, 1.0)], max_norm, False)
    norm, coef = float(run.record.norm), float(run.record.coef)
    print(f"norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.3e} bound {NUMEL * 2.0 ** -53:.3e}")
    assert abs(norm - ref) <= NUMEL * 2.0 ** -53 * ref
    c_ref = clip_ref.coef(ref, max_norm)
    ulp = 2.0 ** (math.floor(math.log2(c_ref)) - 23)
    print(f"coef {coef!r} ref {c_ref!r} ulp {ulp:.3e}")
    assert 0.36 < c_ref < 0.38 and abs(coef - c_ref) <= ulp


# ------------------------------------------------------------------------------------------------ 3. clipped Adam against torch
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_clipped_adam_matches_clip_grad_norm_and_torch_adam(optim, wd):
    seeds = [10 + k for k in range(6)]
    max_norm = _between(_norms(seeds), 3)                 # three steps clip, three do not
    a = _params(3)
    b = _clone(a)
    oa = optim.Adam(a, lr=1e-3, weight_decay=wd, max_norm=max_norm)
    ob = torch.optim.Adam(b, lr=1e-3, weight_decay=wd)
    sa = torch.optim.lr_scheduler.ReduceLROnPlateau(oa, 'min', factor=0.5, patience=0)
    sb = torch.optim.lr_scheduler.ReduceLROnPlateau(ob, 'min', factor=0.5, patience=0)
    clipped = kept = 0
    for step, seed in enumerate(seeds):
        grads = _host_grads(seed)
        _put(a, grads)
        _put(b, grads)
        before = [q.grad.clone() for k, q in enumerate(a) if k != NOGRAD]
        v0 = [q._version for q in a]
        oa.step()
        total = float(torch.nn.utils.clip_grad_norm_(b, max_norm))
        ob.step()
        clipped += total > max_norm
        kept += total < max_norm
        assert abs(float(oa.grad_norm) - total) <= 2.0 ** -20 * total
        assert all((q._version > v) == (k != NOGRAD) for q, v, k in zip(a, v0, range(len(a))))
        assert all(torch.equal(x, q.grad) for x, q in zip(before, [q for k, q in enumerate(a) if k != NOGRAD]))   # .grad is not modified
        sa.step(1.0 + step)
        sb.step(1.0 + step)
        assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
    assert (clipped, kept) == (3, 3) and oa.param_groups[0]["lr"] < 1e-3
    _check_against_torch(oa, a, ob, b, 6)
    assert oa.skipped_steps() == 0


def test_max_norm_above_every_norm_returns_the_bits_of_plain_adam(optim):
    seeds = [20, 21, 22]
    a = _params(5)
    b = _clone(a)
    oa = optim.Adam(a, lr=1e-3, weight_decay=1e-3, max_norm=2.0 * max(_norms(seeds)))
    ob = optim.Adam(b, lr=1e-3, weight_decay=1e-3)
    for seed in seeds:
        grads = _host_grads(seed)
        _put(a, grads)
        _put(b, grads)
        oa.step()
        ob.step()
        assert float(oa._norm.record.coef) == 1.0
    for k, (q, r) in enumerate(zip(a, b)):
        assert torch.equal(q, r), k
        if k != NOGRAD:
            assert torch.equal(oa.state[q]["exp_avg"], ob.state[r]["exp_avg"]) and torch.equal(oa.state[q]["exp_avg_sq"], ob.state[r]["exp_avg_sq"])


# ------------------------------------------------------------------------------------------------ 4. two parameter groups
def test_two_groups_share_the_global_norm(optim):
    seeds = [30, 31]
    max_norm = 0.5 * min(_norms(seeds))
    a = _params(7)
    b = _clone(a)
    split = lambda ps: [{"params": ps[:5]}, {"params": ps[5:], "lr": 3e-4}]
    oa = optim.Adam(split(a), lr=1e-3, weight_decay=1e-3, max_norm=max_norm)
    ob = torch.optim.Adam(split(b), lr=1e-3, weight_decay=1e-3)
    for seed in seeds:
        grads = _host_grads(seed)
        _put(a, grads)
        _put(b, grads)
        oa.step()
        total = float(torch.nn.utils.clip_grad_norm_(b, max_norm))      # over both lists
        ob.step()
        ref = math.sqrt(clip_ref.sumsq(grads))
        assert abs(float(oa.grad_norm) - ref) <= NUMEL * 2.0 ** -53 * ref
        assert abs(float(oa.grad_norm) - total) <= 2.0 ** -20 * total
    _check_against_torch(oa, a, ob, b, 2)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys() and sa["state"].keys() == sb["state"].keys()
    assert set(sa["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and "max_norm" not in sa["param_groups"][0]


# ------------------------------------------------------------------------------------------------ 5. the guard
@pytest.mark.parametrize("where", sorted(BAD_AT))
def test_guard_refuses_a_nonfinite_step(optim, where):
    """good, inf, good, NaN, good against a torch run of the three good steps alone."""
    k_bad, at = BAD_AT[where]
    seeds = [40, 41, 42]
    max_norm = _between(_norms(seeds), 1)                 # one step stays as it is, two clip
    a = _params(9)
    b = _clone(a)
    c = _clone(a)
    oa = optim.Adam(a, lr=1e-3, weight_decay=1e-3, max_norm=max_norm, skip_nonfinite=True)
    ob = torch.optim.Adam(b, lr=1e-3, weight_decay=1e-3)
    oc = optim.Adam(c, lr=1e-3, weight_decay=1e-3, max_norm=max_norm)     # no guard: the same input must poison it
    withgrad = [k for k in range(len(SHAPES)) if k != NOGRAD]
    skipped = 0
    for step, seed in enumerate(seeds):
        grads = _host_grads(seed)
        _put(a, grads)
        _put(b, grads)
        oa.step()
        torch.nn.utils.clip_grad_norm_(b, max_norm)
        ob.step()
        assert int(oa._norm.record.finite) == 1
        if step == 2:
            break
        bad = [None if x is None else x.clone() for x in _host_grads(50 + step)]
        bad[k_bad].view(-1)[at] = float("inf") if step == 0 else float("nan")
        _put(a, bad)
        snap = [(a[k].detach().clone(), oa.state[a[k]]["exp_avg"].clone(), oa.state[a[k]]["exp_avg_sq"].clone()) for k in withgrad]
        oa.step()
        skipped += 1
        for k, (q0, m0, v0) in zip(withgrad, snap):
            assert torch.equal(a[k], q0) and torch.equal(oa.state[a[k]]["exp_avg"], m0) and torch.equal(oa.state[a[k]]["exp_avg_sq"], v0), k
        assert int(oa._norm.record.finite) == 0 and not math.isfinite(float(oa.grad_norm))
        assert oa.skipped_steps() == skipped
        assert float(oa.state[a[0]]["step"]) == step + 1
        if step == 0:
            for q, r in zip(c, a):
                q.data.copy_(r.detach())
            _put(c, _host_grads(seed))
            oc.step()
            _put(c, bad)
            oc.step()
            assert not bool(torch.isfinite(oc.state[c[k_bad]]["exp_avg"]).all())
            assert not bool(torch.isfinite(oc.state[c[k_bad]]["exp_avg_sq"]).all())
    _check_against_torch(oa, a, ob, b, 3)
    assert oa.skipped_steps() == 2 and float(oa.state_dict()["state"][0]["step"]) == 3.0
    # guard without clipping: the norm is reported, nothing is scaled
    d_ = _clone(a)
    e_ = _clone(a)
    od, oe = optim.Adam(d_, lr=1e-3, skip_nonfinite=True), optim.Adam(e_, lr=1e-3)
    _put(d_, _host_grads(60))
    _put(e_, _host_grads(60))
    od.step()
    oe.step()
    assert float(od._norm.record.coef) == 1.0 and all(_close(q, r, 2e-6) for q, r in zip(d_, e_))


# ------------------------------------------------------------------------------------------------ 6. from a bucket
def test_clipped_adam_from_bucket(optim):
    a = _params(5)
    b = _clone(a)
    grads = _host_grads(6)
    _put(a, grads)
    _put(b, grads)
    ref = math.sqrt(clip_ref.sumsq(grads))
    oa = optim.Adam(a, lr=3e-4, weight_decay=1e-3, max_norm=0.5 * ref)
    ob = optim.Adam(b, lr=3e-4, weight_decay=1e-3, max_norm=0.5 * ref)
    tab = optim.TensorTable([q.numel() for q in a], a[0].device)
    flat = tab.flat()
    optim.bucket_gather(tab, [q.grad for q in a], flat)
    flat.mul_(4.0)                                         # a SUM over four ranks ...
    present = [k != NOGRAD for k in range(len(a))]
    oa.step(grad_bucket=(tab, flat, 0.25, present))        # ... averaged by the scale
    ob.step()
    assert torch.equal(oa.grad_norm, ob.grad_norm) and float(oa._norm.record.coef) < 0.51
    for q, r in zip(a, b):
        assert torch.equal(q, r)
    # a parameter marked absent is left alone (value, moments) and left out of the norm, whatever its range of the bucket holds
    keep = a[2].detach().clone(), oa.state[a[2]]["exp_avg"].clone()
    flat[tab.offsets[2]:tab.offsets[2] + tab.numels[2]] = float("nan")
    present[2] = False
    oa.step(grad_bucket=(tab, flat, 0.25, present))
    want = math.sqrt(clip_ref.sumsq([x for k, x in enumerate(grads) if k != 2]))
    assert abs(float(oa.grad_norm) - want) <= NUMEL * 2.0 ** -53 * want
    assert torch.equal(a[2], keep[0]) and torch.equal(oa.state[a[2]]["exp_avg"], keep[1]) and not torch.equal(a[3], b[3])
    assert all(bool(torch.isfinite(q).all()) for q in a)


# ------------------------------------------------------------------------------------------------ 7. functional
def test_clip_grad_norm_follows_torch(optim):
    a = _params(11)
    b = _clone(a)
    grads = _host_grads(12)
    ref = math.sqrt(clip_ref.sumsq(grads))
    for max_norm in (0.3 * ref, 2.0 * ref):
        _put(a, grads)
        _put(b, grads)
        got = optim.clip_grad_norm_(a, max_norm)
        want = torch.nn.utils.clip_grad_norm_(b, max_norm)
        assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
        assert abs(float(got) - ref) <= 2.0 ** -24 * ref * (1 + 2.0 ** -20) and abs(float(got) - float(want)) <= 2.0 ** -20 * float(want)
        for k, (q, r) in enumerate(zip(a, b)):
            if k == NOGRAD:
                assert q.grad is None
            else:
                # one ulp of the coefficient plus one of the product, relative to each element
                assert bool(((q.grad - r.grad).abs() <= 2.0 ** -22 * r.grad.abs()).all()), k
    assert float(optim.clip_grad_norm_(a[0], 1e9)) == float(a[0].grad.abs())            # a single tensor, as torch takes one
    bad = [None if x is None else x.clone() for x in grads]
    bad[5][7, 9] = float("nan")
    _put(a, bad)
    with pytest.raises(RuntimeError):
        optim.clip_grad_norm_(a, 1.0, error_if_nonfinite=True)
    assert math.isnan(float(optim.clip_grad_norm_(a, 1.0)))
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(a, 1.0, norm_type=float("inf"))


# ------------------------------------------------------------------------------------------------ 8. the adversarial fine-tune
class _WithMaxNorm:
    """Stands in for the optim module in test_gpu_adversarial.build_step: decoder optimiser first, distinguisher second."""

    def __init__(self, optim, max_norms):
        self.optim, self.max_norms = optim, list(max_norms)

    def Adam(self, params, **kw):
        return self.optim.Adam(params, max_norm=self.max_norms.pop(0), **kw)


def test_adversarial_step_with_clipping_optimisers(optim, golden):
    """adversarial.AdversarialFineTune needs no change: its two optimisers are the caller's.  One step on the mini configuration, both
    optimisers with max_norm = a tenth of the norm the unclipped step reports.  Adam's first update is lr g' / (|g'| + eps) per
    element with g' = coef g + wd p, nearly independent of the size of g: the change shrinks only through eps and the weight
    decay (measured: 0.298888 against 0.298904 for the decoder, 0.0162348 against 0.0162359 for the distinguisher)."""
    from test_gpu_adversarial import batch, build_step, params_of
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    adv = importlib.import_module("i-dccrn-vae_amd.adversarial")
    d = golden("grad_adv_mini")
    change = {}
    norms = None
    for run in ("unclipped", "clipped"):
        # first pass: a max_norm no gradient reaches, which only reports the norms
        opts = _WithMaxNorm(optim, [1e30, 1e30] if norms is None else [0.1 * n for n in norms])
        step, ye, de, D = build_step(pm, adv, opts, d)
        before = params_of(de), params_of(D)
        step.step(*batch(d, 0))
        change[run] = [math.sqrt(sum(float((p_.detach().double() - b[k].double()).pow(2).sum()) for k, p_ in m.named_parameters()))
                       for m, b in zip((de, D), before)]
        got = [float(step.opt_decoder.grad_norm), float(step.opt_dis.grad_norm)]
        assert all(math.isfinite(n) and n > 0 for n in got)
        print(run, "norms (decoder, distinguisher)", got, "parameter change", change[run])
        if norms is None:
            norms = got
            assert float(step.opt_decoder._norm.record.coef) == 1.0 and float(step.opt_dis._norm.record.coef) == 1.0
        else:
            # max_norm below the step's norm: both optimisers clipped
            assert got[0] > step.opt_decoder.max_norm and got[1] > step.opt_dis.max_norm
            assert float(step.opt_decoder._norm.record.coef) < 1.0 and abs(float(step.opt_dis._norm.record.coef) - 0.1) < 1e-3
    assert change["clipped"][0] < change["unclipped"][0] and change["clipped"][1] < change["unclipped"][1]
