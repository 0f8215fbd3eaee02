"""Time of the optimiser step with and without the global gradient norm / clipping / non-finite guard (optim.Adam(max_norm,
skip_nonfinite), csrc/bucket.hip) on the parameter set of the full-width NSVAE noisy encoder (about 25 M elements).

    python profiles/tools/measure_clip.py [--iters 20] [--warmup 5] [--rounds 2] [--out profiles/clip/measure.json]

All variants run in one process, in turn, ``--rounds`` times; each is the mean device time of one call over ``--iters`` calls after
``--warmup`` untimed ones, HIP events around every call:
  a  adam            optim.Adam.step() without the new arguments
  b  torch_clip      torch.nn.utils.clip_grad_norm_(params, max_norm) followed by a: what one GPU allowed before
  c  fused           optim.Adam(max_norm=...).step()
  d  fused_guard     optim.Adam(max_norm=..., skip_nonfinite=True).step()
  e  functional      optim.clip_grad_norm_(params, max_norm) followed by a
The gradients are N(0, 1e-3) and max_norm is half their norm, so that every variant does clip on its first call.  Reported per
round and as the minimum over the rounds: the five times, c - a, d - c, and whether c <= b.
Fails without a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)

NFFT, HOP, WIN = 512, 100, 400


def parameters(base, zdim, ns):
    from oracle import idccrn_oracle as O
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    m = pm.nsvae_pvae_dccrn_encoder_twophase(O.net_params(True, base), True, "cuda", zdim, NFFT, HOP, WIN, ns, 2)
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter((0.1 * torch.randn(*q.shape, generator=g)).cuda()) for q in m.parameters() if q.requires_grad]
    grads = [(1e-3 * torch.randn(*q.shape, generator=g)).cuda() for q in ps]
    return ps, grads


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for k in range(iters):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    return sum(ev[k].elapsed_time(ev[k + 1]) for k in range(iters)) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", type=int, default=32)
    ap.add_argument("--zdim", type=int, default=128)
    ap.add_argument("--ns", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clip", "measure.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_clip.py measures on the GPU; there is nothing to report without one")
    optim = importlib.import_module("i-dccrn-vae_amd.optim")
    ps, grads = parameters(a.base, a.zdim, a.ns)
    numel = sum(q.numel() for q in ps)
    max_norm = 0.5 * float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))

    def fresh():
        for q, g in zip(ps, grads):
            q.grad = g.clone()

    def variant(name):
        kw = dict(lr=1e-3, weight_decay=1e-3)
        if name == "adam":
            opt = optim.Adam(ps, **kw)
            return opt.step
        if name == "torch_clip":
            opt = optim.Adam(ps, **kw)
            return lambda: (torch.nn.utils.clip_grad_norm_(ps, max_norm), opt.step())
        if name == "functional":
            opt = optim.Adam(ps, **kw)
            return lambda: (optim.clip_grad_norm_(ps, max_norm), opt.step())
        opt = optim.Adam(ps, max_norm=max_norm, skip_nonfinite=name == "fused_guard", **kw)
        return opt.step

    names = ("adam", "torch_clip", "fused", "fused_guard", "functional")
    rounds = []
    for _ in range(a.rounds):
        r = {}
        for name in names:
            fresh()
            r[name] = timed(variant(name), a.iters, a.warmup)
        rounds.append(r)
    best = {n: min(r[n] for r in rounds) for n in names}
    res = {"device": torch.cuda.get_device_name(0), "tensors": len(ps), "elements": numel, "max_norm": max_norm, "iters": a.iters,
           "warmup": a.warmup, "ms_per_round": rounds, "ms": best, "fused_minus_adam_ms": best["fused"] - best["adam"],
           "guard_minus_fused_ms": best["fused_guard"] - best["fused"], "torch_clip_minus_adam_ms": best["torch_clip"] - best["adam"],
           "fused_not_slower_than_torch_clip": all(r["fused"] <= r["torch_clip"] for r in rounds)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
