"""tests/clip_ref.py (the float64 host definition the GPU clipping tests compare with) against stock torch on the CPU:
``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam`` on float64 parameters.  Both sides are float64 evaluations of the same
formulas in slightly different orders: 1e-12 relative to each tensor's scale."""
import math

import torch

import clip_ref

SHAPES = [(1,), (3, 5), (257,), (2,), (40, 33)]


def _grads(seed, skip=(3,)):
    g = torch.Generator().manual_seed(seed)
    return [None if k in skip else torch.randn(*s, generator=g) * (0.5 if k % 2 else 2e-3) for k, s in enumerate(SHAPES)]


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-30)


def test_norm_and_coefficient_follow_torch():
    gr = _grads(1)
    ps = [torch.nn.Parameter(torch.zeros(*s, dtype=torch.float64)) for s in SHAPES]
    for q, g in zip(ps, gr):
        q.grad = None if g is None else g.double()
    ss = clip_ref.sumsq(gr)
    norm = math.sqrt(ss)
    want = float(torch.nn.utils.clip_grad_norm_(ps, 0.5 * norm))
    assert abs(norm - want) <= 1e-14 * want
    c = clip_ref.coef(norm, 0.5 * norm)
    assert abs(c - 0.5) < 1e-6 and clip_ref.coef(norm, 2 * norm) == 1.0 and clip_ref.coef(norm, None) == 1.0
    for q, g in zip(ps, gr):
        if g is not None:
            assert _close(q.grad, g.double() * c)
    # the scale is applied in float32 before the square
    s3 = clip_ref.sumsq(gr, 1.0 / 3.0)
    want3 = sum(float(((g * torch.tensor(1.0 / 3.0)).double() ** 2).sum()) for g in gr if g is not None)
    assert abs(s3 - want3) <= 1e-14 * want3
    assert not math.isfinite(clip_ref.sumsq([torch.tensor([1.0, float("inf")])]))
    assert math.isnan(clip_ref.sumsq([torch.tensor([1.0, float("nan")])]))


def test_adam64_follows_torch_adam_with_clipping_and_skips_bad_steps():
    g = torch.Generator().manual_seed(7)
    init = [torch.randn(*s, generator=g) * 0.3 for s in SHAPES]
    norms = [math.sqrt(clip_ref.sumsq(_grads(10 + k))) for k in range(5)]
    max_norm = 0.5 * (sorted(norms)[2] + sorted(norms)[3])      # between the third and the fourth norm: two steps clip, three do not
    ps = [torch.nn.Parameter(q.double().clone()) for q in init]
    opt = torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-3)
    ref = clip_ref.Adam64(init, lr=1e-3, weight_decay=1e-3, max_norm=max_norm, skip_nonfinite=True)
    clipped = 0
    for k in range(5):
        gr = _grads(10 + k)
        if k == 2:                                    # a batch torch never sees: the reference must skip it
            bad = [None if x is None else x.clone() for x in gr]
            bad[2][100] = float("inf")
            assert ref.step(bad)[2] is False
        for q, x in zip(ps, gr):
            q.grad = None if x is None else x.double()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        norm, c, applied = ref.step(gr)
        assert applied and abs(norm - norms[k]) <= 1e-14 * norm
        clipped += c < 1.0
    assert clipped == 2 and ref.t == 5 and ref.skipped == 1
    for k, (q, r) in enumerate(zip(ps, ref.p)):
        assert _close(r, q.detach()), k
        if k == 3:
            assert torch.equal(r, init[k].double())
        else:
            assert _close(ref.m[k], opt.state[q]["exp_avg"]) and _close(ref.v[k], opt.state[q]["exp_avg_sq"]), k
            assert float(opt.state[q]["step"]) == ref.t
