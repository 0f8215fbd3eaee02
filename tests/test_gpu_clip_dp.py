"""Clipping in the data-parallel step (parallel.GradAllReduce.reduce(into_grads=False) + optim.Adam.step(grad_bucket=...) with
max_norm / skip_nonfinite): two spawned ranks on the one GPU over gloo, different gradients per rank, three steps
of which the second has an inf on rank 1 only.  The reduced bucket holds the same bits on both ranks and the norm is summed in a
fixed order, so parameters, moments, the norm and the count of refused steps must be bit-equal across the ranks with no further
collective -- and within the bars of tests/test_gpu_clip.py (2e-6 of the parameter scale, 1e-6 of the moments' scale) of one
process that steps with clip_grad_norm_ + torch.optim.Adam on the averaged gradients of the two finite steps."""
import importlib
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import clip_ref
from test_gpu_clip import NOGRAD, SHAPES, _host_grads

pytestmark = pytest.mark.gpu
STEPS = 3
BAD_STEP = 1
RANK_LIMIT = 120                                      # seconds per rank


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init():
    g = torch.Generator().manual_seed(77)
    return [torch.randn(*s, generator=g) * 0.3 for s in SHAPES]


def _rank_grads(step, rank):
    grads = _host_grads(100 + 10 * step + rank)
    if step == BAD_STEP and rank == 1:
        grads[5][300, 17] = float("inf")
    return grads


def _average(step):
    return [None if x is None else (x + y) * 0.5 for x, y in zip(_rank_grads(step, 0), _rank_grads(step, 1))]


def _max_norm():
    """Between the norms of the two finite steps' averaged gradients: one of them clips, the other does not."""
    n = [math.sqrt(clip_ref.sumsq(_average(s))) for s in range(STEPS) if s != BAD_STEP]
    return 0.5 * (n[0] + n[1]), n


def _run_rank(rank, world):
    optim = importlib.import_module("i-dccrn-vae_amd.optim")
    par = importlib.import_module("i-dccrn-vae_amd.parallel")
    ps = [torch.nn.Parameter(q.cuda()) for q in _init()]
    opt = optim.Adam(ps, lr=1e-3, weight_decay=1e-3, max_norm=_max_norm()[0], skip_nonfinite=True)
    red = par.GradAllReduce(ps)
    norms = []
    for step in range(STEPS):
        for q, x in zip(ps, _rank_grads(step, rank)):
            q.grad = None if x is None else x.cuda()
        red.reduce(into_grads=False)
        opt.step(grad_bucket=red.bucket())
        norms.append(float(opt.grad_norm))
    torch.cuda.synchronize()
    out = {"skipped": opt.skipped_steps(), "norms": norms, "step": float(opt.state[ps[0]]["step"])}
    for k, q in enumerate(ps):
        out[f"p{k}"] = q.detach().cpu().numpy()
        if k != NOGRAD:
            out[f"m{k}"] = opt.state[q]["exp_avg"].cpu().numpy()
            out[f"v{k}"] = opt.state[q]["exp_avg_sq"].cpu().numpy()
    return out


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        try:
            q.put((rank, _run_rank(rank, world)))
        except BaseException:            # the parent must not sit in q.get() until its time-out: hand the failure over
            import traceback
            q.put((rank, "error", traceback.format_exc()))
            raise
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _stop(procs):
    for p in procs:
        p.join(timeout=10)
        if p.is_alive():
            p.terminate()


def test_two_ranks_clip_and_skip_alike():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = {}
    for _ in procs:
        try:
            r = q.get(timeout=RANK_LIMIT)
        except Exception:
            _stop(procs)
            pytest.fail("a rank did not answer within its time limit")
        if len(r) == 3 and r[1] == "error":
            _stop(procs)
            pytest.fail(f"rank {r[0]} failed:\n{r[2]}")
        out[r[0]] = r[1]
    for p in procs:
        p.join(timeout=RANK_LIMIT)
        if p.is_alive():
            _stop(procs)
            pytest.fail("a rank did not end within its time limit")
        assert p.exitcode == 0
    a, b = out[0], out[1]
    assert a["skipped"] == b["skipped"] == 1 and a["step"] == b["step"] == 2.0
    assert a["norms"] == b["norms"] and math.isinf(a["norms"][BAD_STEP])
    for k in a:
        if k[0] in "pmv" and k[1:].isdigit():
            assert np.array_equal(a[k], b[k]), k
    # one process on the averaged gradients of the two finite steps, on the device as in tests/test_gpu_clip.py (the float32 norm of
    # torch's CPU kernels is 2e-5 off at this size, which is more than the bars allow the coefficient)
    max_norm, want_norms = _max_norm()
    ps = [torch.nn.Parameter(x.cuda()) for x in _init()]
    opt = torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-3)
    clipped = 0
    for step in range(STEPS):
        if step == BAD_STEP:
            continue
        for p_, x in zip(ps, _average(step)):
            p_.grad = None if x is None else x.cuda()
        clipped += float(torch.nn.utils.clip_grad_norm_(ps, max_norm)) > max_norm
        opt.step()
    assert clipped == 1
    finite = [n for s, n in enumerate(a["norms"]) if s != BAD_STEP]
    n_el = sum(math.prod(s) for k, s in enumerate(SHAPES) if k != NOGRAD)
    assert all(abs(n - w) <= n_el * 2.0 ** -53 * w for n, w in zip(finite, want_norms))
    for k, p_ in enumerate(ps):
        ref = p_.detach().cpu().numpy()
        assert np.abs(a[f"p{k}"] - ref).max() <= 2e-6 * np.abs(ref).max(), k
        if k != NOGRAD:
            for key, name in (("m", "exp_avg"), ("v", "exp_avg_sq")):
                ref = opt.state[p_][name].cpu().numpy()
                assert np.abs(a[f"{key}{k}"] - ref).max() <= 1e-6 * np.abs(ref).max(), (k, name)
