"""Float64 host definition of the clipped, guarded Adam step (csrc/bucket.hip idv_bucket_sqnorm / idv_bucket_clip_finalize /
idv_bucket_adam_clipped), for tests/test_clip_host.py and tests/test_gpu_clip*.py.

  sumsq = sum over every gradient element of x^2, x = the FLOAT32 product g * scale widened to float64
  norm  = sqrt(sumsq)
  coef  = min(1, max_norm / (norm + 1e-6))         torch.nn.utils.clip_grad_norm_'s rule; 1 without a max_norm
  Adam  = torch.optim.Adam's update (L2 weight decay, no amsgrad) in float64, with one step count per optimiser and a "skip"
          branch: a step whose sumsq is not finite changes nothing and does not advance the count.
"""
import math

import torch


def sumsq(grads, scale=1.0):
    """grads: float32 tensors (None: absent).  Exact squares of the float32 products, summed in float64."""
    s = torch.zeros((), dtype=torch.float64)
    sc = torch.tensor(scale, dtype=torch.float32)
    for g in grads:
        if g is not None:
            x = (g.detach().cpu().float() * sc).double()
            s = s + (x * x).sum()
    return float(s)


def coef(norm, max_norm):
    if max_norm is None or not max_norm > 0.0:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return 1.0 if c > 1.0 else c


class Adam64:
    """params: float32 tensors, copied to float64.  step(grads, scale) -> (norm, coef, applied)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, skip_nonfinite=False):
        self.p = [q.detach().cpu().double().clone() for q in params]
        self.m = [torch.zeros_like(q) for q in self.p]
        self.v = [torch.zeros_like(q) for q in self.p]
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.max_norm, self.skip_nonfinite = max_norm, skip_nonfinite
        self.t = 0
        self.skipped = 0

    def step(self, grads, scale=1.0):
        ss = sumsq(grads, scale)
        norm = math.sqrt(ss) if ss == ss else float("nan")
        if self.skip_nonfinite and not math.isfinite(ss):
            self.skipped += 1
            return norm, coef(norm, self.max_norm), False
        c = coef(norm, self.max_norm)
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2s = 1.0 - b1 ** self.t, math.sqrt(1.0 - b2 ** self.t)
        sc = torch.tensor(scale, dtype=torch.float32)
        for k, g in enumerate(grads):
            if g is None:
                continue
            x = (g.detach().cpu().float() * sc).double() * c + self.wd * self.p[k]
            self.m[k] = self.m[k] + (x - self.m[k]) * (1.0 - b1)
            self.v[k] = b2 * self.v[k] + (1.0 - b2) * x * x
            self.p[k] = self.p[k] - (self.lr / bc1) * (self.m[k] / (self.v[k].sqrt() / bc2s + self.eps))
        return norm, c, True
