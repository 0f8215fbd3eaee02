"""Multi-tensor pieces of the train step on the HIP path (csrc/bucket.hip): the flat gradient bucket and Adam.

Reference: every trainer does ``loss.backward(); optimizer.step()`` with ``torch.optim.Adam(params, lr, weight_decay=0.001)``
(supervised_dccrn/train.py:109, 239-243; i_dccrn_vae/nsvae_dccrn/train_nsvae.py:200, 557-561;
i_dccrn_vae/nsvae_dccrn/train_second_phase_decoder.py:420-433; i_dccrn_vae/pretrained_vaes/train.py:296-301).

``Adam`` here IS a ``torch.optim.Adam`` (same constructor, ``param_groups``, ``state_dict()`` keys ``step`` / ``exp_avg`` /
``exp_avg_sq``, so the reference's ``*_optim_dict`` checkpoints load and save unchanged and ``ReduceLROnPlateau`` drives it)
whose ``step()`` is ONE kernel launch per parameter group over a pointer table instead of torch's per-tensor / foreach
kernels; the moments live in one flat buffer per group, the per-parameter state tensors are views of it.

``Adam(max_norm=..., skip_nonfinite=...)`` and ``clip_grad_norm_`` add the global gradient norm, clipping and a refused step
on a NaN / inf gradient on the same tables: per-workgroup double partials, one finalise launch that writes a
32-byte device record, and kernels that read the coefficient and the skip decision from that record -- no host read.
"""
from __future__ import annotations

import math
import weakref
from typing import List, Optional, Sequence

import torch

from . import _lib as L
from ._lib import call, p, i, f, d, ll, stream_ptr


class TensorTable:
    """Bucket layout of a list of tensors (see include/idccrn_hip.h, "bucket layout"): offsets padded to 4 floats, and the
    device-side pointer table, re-uploaded only when a pointer changed (``.grad`` tensors are re-allocated by
    ``zero_grad(set_to_none=True)``)."""

    def __init__(self, numels: Sequence[int], device):
        self.device = device
        self.numels = [int(n) for n in numels]
        self.offsets: List[int] = []
        o = 0
        for n in self.numels:
            self.offsets.append(o)
            o += (n + 3) // 4 * 4
        self.total = max(o, 4)
        self.n = len(self.numels)
        self._ptrs: Optional[tuple] = None
        self._dev: Optional[torch.Tensor] = None

    def flat(self, zero: bool = True) -> torch.Tensor:
        return (torch.zeros if zero else torch.empty)(self.total, dtype=torch.float32, device=self.device)

    def views(self, flat: torch.Tensor, shapes) -> List[torch.Tensor]:
        return [flat[o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, shapes)]

    def table(self, tensors: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
        """Device table for these tensors (None -> absent).  Every tensor must be fp32, contiguous, on the device."""
        ptrs = []
        for t, n in zip(tensors, self.numels):
            if t is None:
                ptrs.append(0)
                continue
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
                raise RuntimeError("TensorTable: tensors must be contiguous fp32 device tensors of the registered sizes")
            ptrs.append(t.data_ptr())
        ptrs = tuple(ptrs)
        if ptrs != self._ptrs:
            rows = [[q, o, n] for q, o, n in zip(ptrs, self.offsets, self.numels)]
            host = torch.tensor(rows, dtype=torch.int64).pin_memory()
            if self._dev is None:
                self._dev = torch.empty(self.n, 3, dtype=torch.int64, device=self.device)
            # stream-ordered upload: kernels already queued on this stream keep reading the old rows until they finish
            self._dev.copy_(host, non_blocking=True)
            self._host = host                       # pinned source stays alive until the next upload
            self._ptrs = ptrs
        return self._dev


def bucket_gather(tab: TensorTable, tensors, flat: torch.Tensor):
    call("idv_bucket_gather", p(tab.table(tensors)), i(tab.n), ll(tab.total), p(flat), stream_ptr())


def bucket_scatter(tab: TensorTable, tensors, flat: torch.Tensor, scale: float = 1.0):
    call("idv_bucket_scatter", p(tab.table(tensors)), i(tab.n), ll(tab.total), p(flat), f(scale), stream_ptr())


# The device record of a norm pass: byte offsets of its fields (IDV_CLIP_* of include/idccrn_hip.h) and its size.
CLIP_FIELD = {"sumsq": 0, "norm": 8, "coef": 16, "finite": 20, "skipped": 24}
CLIP_RECORD_BYTES = 32


class ClipRecord:
    """The 32-byte record ``idv_bucket_clip_finalize`` writes, as views of one device buffer: ``sumsq`` / ``norm`` (float64),
    ``coef`` (float32), ``finite`` (int32), ``skipped`` (int64), each a 0-dim tensor.  Reading one is the caller's sync."""

    def __init__(self, device):
        self.buf = torch.zeros(CLIP_RECORD_BYTES // 8, dtype=torch.int64, device=device)
        f64, f32, i32 = self.buf.view(torch.float64), self.buf.view(torch.float32), self.buf.view(torch.int32)
        self.sumsq, self.norm = f64[CLIP_FIELD["sumsq"] // 8], f64[CLIP_FIELD["norm"] // 8]
        self.coef, self.finite = f32[CLIP_FIELD["coef"] // 4], i32[CLIP_FIELD["finite"] // 4]
        self.skipped = self.buf[CLIP_FIELD["skipped"] // 8]


def sqnorm_partials(total: int) -> int:
    """Partials one table of padded length ``total`` takes (one per 4096 floats)."""
    n = int(L.lib().idv_bucket_sqnorm_partials(int(total)))
    if n < 0:
        raise L.IdvError(f"idv_bucket_sqnorm_partials refuses total = {total}")
    return n


class _NormPass:
    """Partials buffer + record of one set of tables: ``run(jobs, max_norm, guard)`` launches one ``idv_bucket_sqnorm`` per job
    = (ptable, gtable, gflat, n, total, grad_scale) and one ``idv_bucket_clip_finalize`` over all of them."""

    def __init__(self, device):
        self.record = ClipRecord(device)
        self.partials = None

    def run(self, jobs, max_norm, guard: bool):
        counts = [sqnorm_partials(j[4]) for j in jobs]
        if self.partials is None or self.partials.numel() < sum(counts):
            self.partials = torch.empty(sum(counts), dtype=torch.float64, device=self.record.buf.device)
        first = 0
        for (ptable, gtable, gflat, n, total, gscale), c in zip(jobs, counts):
            call("idv_bucket_sqnorm", p(ptable), p(gtable), p(gflat), i(n), ll(total), f(gscale), p(self.partials), ll(first), stream_ptr())
            first += c
        call("idv_bucket_clip_finalize", p(self.partials), i(first), d(0.0 if max_norm is None else max_norm), i(1 if guard else 0),
             p(self.record.buf), stream_ptr())


class _GuardedState(dict):
    """Per-parameter state of a guarded optimiser: ``["step"]`` is the APPLIED step count, which the host only knows after one
    device read of the record's ``skipped`` counter (Adam._rebase); everything else is the plain dict torch expects."""

    def __init__(self, opt, *a):
        super().__init__(*a)
        self._opt = weakref.ref(opt)

    def __getitem__(self, k):
        if k == "step":
            o = self._opt()
            if o is not None:
                o._rebase()
        return super().__getitem__(k)


class Adam(torch.optim.Adam):
    """torch.optim.Adam with a one-launch ``step()`` (csrc/bucket.hip ``idv_bucket_adam``).

    ``step(grad_bucket=(table, flat, scale, present))``: take the gradients of group 0 straight from an all-reduced bucket with
    the same layout (parallel.GradAllReduce hands it over), so that the scatter back into ``.grad`` disappears; ``present[k]``
    False = parameter k had no gradient (skipped, as torch skips it).

    ``max_norm``: clip the gradients of ALL groups to this global 2-norm, by torch's ``clip_grad_norm_`` rule
    (coef = min(1, max_norm / (norm + 1e-6))), inside the step: one ``idv_bucket_sqnorm`` per group over the tables the step uses
    anyway (group 0 from the bucket when ``grad_bucket`` is given), one ``idv_bucket_clip_finalize`` over all of them, one
    ``idv_bucket_adam_clipped`` per group that reads the coefficient from the device record.  ``.grad`` is not modified.
    ``skip_nonfinite``: a step whose gradients hold a NaN or inf is refused on the device -- parameters, moments and the bias
    correction's step count keep their values -- and counted (``skipped_steps()``); ``max_norm=None`` then guards without clipping.
    ``grad_norm``: the norm of the last step as a 0-dim float64 device tensor (a view of the record: the next step overwrites it;
    reading it is the caller's sync).  Both arguments are attributes, not ``param_groups`` keys: ``state_dict()`` keeps exactly
    torch's keys.  With the guard ``state[p]["step"]`` and ``state_dict()`` report the applied count, at the cost of one device
    read when they are asked for.  The count of refused steps is one per optimiser: a group that has no gradient at all on a refused
    step but has some on others would be corrected with a count one too small (no trainer of the reference has such a group)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_norm=None,
                 skip_nonfinite=False, **kw):
        if amsgrad or kw.get("maximize") or kw.get("capturable") or kw.get("differentiable"):
            raise NotImplementedError("i-dccrn-vae_amd.optim.Adam: plain Adam (+ L2 weight decay) only, as every reference trainer uses")
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError("i-dccrn-vae_amd.optim.Adam: max_norm must be a positive number or None")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, fused=False)
        self._g = {}                                    # group index -> (params, TensorTable p, TensorTable g, m, v, step)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._norm: Optional[_NormPass] = None
        self._skipped = 0                               # refused steps the host has already taken out of every group's count
        self._unread = False                            # a guarded step ran since the device counter was last read
        self.grad_norm: Optional[torch.Tensor] = None

    # ---- flat state ---------------------------------------------------------------------------------------------------
    def _group_state(self, gi: int, group):
        params = [q for q in group["params"] if q.requires_grad]
        ent = self._g.get(gi)
        if ent is not None and ent["ids"] == tuple(id(q) for q in params):
            return ent
        if not params:
            return None
        dev = params[0].device
        for q in params:
            if not q.is_cuda or q.dtype != torch.float32 or not q.is_contiguous():
                raise RuntimeError("i-dccrn-vae_amd.optim.Adam runs on the MI355X: parameters must be contiguous fp32 device tensors")
        ptab = TensorTable([q.numel() for q in params], dev)
        gtab = TensorTable([q.numel() for q in params], dev)
        m, v = ptab.flat(), ptab.flat()
        shapes = [q.shape for q in params]
        mv, vv = ptab.views(m, shapes), ptab.views(v, shapes)
        t = 0
        for q, a, b in zip(params, mv, vv):
            st = self.state.get(q)
            if st and "exp_avg" in st:                  # state restored by load_state_dict (or an earlier layout): adopt it
                a.copy_(st["exp_avg"])
                b.copy_(st["exp_avg_sq"])
                t = max(t, int(float(st["step"])))
                st["exp_avg"], st["exp_avg_sq"] = a, b
        ent = {"ids": tuple(id(q) for q in params), "params": params, "ptab": ptab, "gtab": gtab, "m": m, "v": v, "mv": mv,
               "vv": vv, "t": t}
        self._g[gi] = ent
        return ent

    def load_state_dict(self, state_dict):
        self._rebase()                                  # refused steps still on the device belong to the OLD counts
        super().load_state_dict(state_dict)
        self._g = {}                                    # the loaded moment tensors are adopted on the next step

    # ---- the guard's step count ---------------------------------------------------------------------------------------
    def _rebase(self):
        """Take the refused steps the device has counted out of every group's step count (one device read), zero the device
        counter, and write the applied count into ``state[p]["step"]``."""
        if not self._unread:
            return
        self._unread = False
        k = int(self._norm.record.skipped)
        if k:
            self._norm.record.skipped.zero_()
            self._skipped += k
            for ent in self._g.values():
                ent["t"] = max(ent["t"] - k, 0)
        for ent in self._g.values():
            stp = torch.tensor(float(ent["t"]))
            for q in ent["params"]:
                st = self.state.get(q)
                if st is not None and "exp_avg" in st:
                    dict.__setitem__(st, "step", stp)

    def skipped_steps(self) -> int:
        """Steps the guard has refused so far (one device read)."""
        self._rebase()
        return self._skipped

    def state_dict(self):
        self._rebase()
        sd = super().state_dict()
        sd["state"] = {k: dict(v) for k, v in sd["state"].items()}
        return sd

    def _gradients(self, gi: int, group, grad_bucket):
        """(ent, has, gtable, gflat, gscale) of one group for this step, or None when it has no parameter or no gradient."""
        ent = self._group_state(gi, group)
        if ent is None:
            return None
        params = ent["params"]
        gflat, gscale, gtable = None, 1.0, None
        if grad_bucket is not None and gi == 0:
            btab, gflat, gscale, has = grad_bucket
            if btab.offsets != ent["ptab"].offsets or btab.numels != ent["ptab"].numels:
                raise RuntimeError("grad_bucket layout differs from the optimiser's parameter group")
            has = list(has)
            if not any(has):
                return None
        else:
            grads = [q.grad for q in params]
            has = [g_ is not None for g_ in grads]
            if not any(has):
                return None
            grads = [None if g_ is None else (g_ if g_.is_contiguous() else g_.contiguous()) for g_ in grads]
            gtable = ent["gtab"].table(grads)
        return ent, has, gtable, gflat, gscale

    @torch.no_grad()
    def step(self, closure=None, grad_bucket=None):
        """One Adam step.  As in torch, a parameter without a gradient is skipped and keeps no state; unlike torch, the
        parameters of a group share ONE step count for the bias correction (they do in every trainer of the reference, where
        a parameter either gets a gradient on every step or on none)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = self.max_norm is not None or self.skip_nonfinite
        work = []
        for gi, group in enumerate(self.param_groups):
            got = self._gradients(gi, group, grad_bucket)
            if got is None:
                continue
            ent, has, gtable, gflat, gscale = got
            # a parameter without a gradient is absent from the table (NULL row): the kernels leave it and its moments alone
            ptable = ent["ptab"].table([q if h else None for q, h in zip(ent["params"], has)])
            work.append((group, ent, has, ptable, gtable, gflat, gscale))
        if clip and work:
            if self._norm is None:
                self._norm = _NormPass(work[0][1]["params"][0].device)
                self.grad_norm = self._norm.record.norm
            self._norm.run([(ptable, gtable, gflat, ent["ptab"].n, ent["ptab"].total, gscale)
                            for _, ent, _, ptable, gtable, gflat, gscale in work], self.max_norm, self.skip_nonfinite)
            self._unread = self.skip_nonfinite
        for group, ent, has, ptable, gtable, gflat, gscale in work:
            params = ent["params"]
            t = ent["t"] = ent["t"] + 1
            b1, b2 = group["betas"]
            if clip:
                # with the guard t counts the refused steps too: the kernel takes the record's `skipped` off it
                call("idv_bucket_adam_clipped", p(ptable), p(gtable), p(gflat), p(ent["m"]), p(ent["v"]), i(ent["ptab"].n),
                     ll(ent["ptab"].total), f(group["lr"]), d(b1), d(b2), f(group["eps"]), f(group["weight_decay"]), f(1.0 - b1 ** t),
                     f(math.sqrt(1.0 - b2 ** t)), f(gscale), p(self._norm.record.buf), i(1 if self.skip_nonfinite else 0), ll(t),
                     stream_ptr())
            else:
                call("idv_bucket_adam", p(ptable), p(gtable), p(gflat), p(ent["m"]), p(ent["v"]), i(ent["ptab"].n),
                     ll(ent["ptab"].total), f(group["lr"]), d(b1), d(b2), f(group["eps"]), f(group["weight_decay"]), f(1.0 - b1 ** t),
                     f(math.sqrt(1.0 - b2 ** t)), f(gscale), stream_ptr())
            stp = torch.tensor(float(t))
            for q, h, a, b in zip(params, has, ent["mv"], ent["vv"]):
                if h:
                    st = self.state[q]
                    if self.skip_nonfinite and not isinstance(st, _GuardedState):
                        st = self.state[q] = _GuardedState(self, st)
                    st["step"] = stp
                    if st.get("exp_avg") is not a:
                        st["exp_avg"], st["exp_avg_sq"] = a, b
            _bump_versions([q for q, h in zip(params, has) if h])
        return loss


_CLIP_CACHE: dict = {}                                  # tuple of parameter ids -> (weak references, TensorTable, _NormPass)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` on the bucket kernels, for use in front of a stock optimiser or of several optimisers:
    the ``.grad`` tensors are scaled in place by min(1, max_norm / (norm + 1e-6)), three launches whatever the number of tensors
    (``idv_bucket_sqnorm``, ``idv_bucket_clip_finalize``, ``idv_bucket_scale``) and no host read.  Returns the total 2-norm as a
    0-dim float32 device tensor.  ``norm_type`` other than 2 raises NotImplementedError; ``error_if_nonfinite`` reads the record's
    flag (a sync) and raises RuntimeError as torch does; ``foreach`` is accepted and ignored."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("i-dccrn-vae_amd.optim.clip_grad_norm_: the 2-norm only")
    if not float(max_norm) > 0.0:
        raise ValueError("i-dccrn-vae_amd.optim.clip_grad_norm_: max_norm must be a positive number")
    params = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    if not any(q.grad is not None for q in params):
        return torch.tensor(0.0, device=params[0].device if params else None)
    key = tuple(id(q) for q in params)
    ent = _CLIP_CACHE.get(key)
    if ent is None or any(r() is not q for r, q in zip(ent[0], params)):
        if len(_CLIP_CACHE) >= 16:
            _CLIP_CACHE.clear()
        dev = next(q.grad.device for q in params if q.grad is not None)
        ent = _CLIP_CACHE[key] = ([weakref.ref(q) for q in params], TensorTable([q.numel() for q in params], dev), _NormPass(dev))
    _, tab, norm = ent
    with torch.no_grad():
        for q in params:
            if q.grad is not None and not q.grad.is_contiguous():
                q.grad = q.grad.contiguous()             # scaled in place below: the copy becomes the gradient
        table = tab.table([q.grad for q in params])
        norm.run([(table, table, None, tab.n, tab.total, 1.0)], float(max_norm), False)
        if error_if_nonfinite and int(norm.record.finite) == 0:
            raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped")
        call("idv_bucket_scale", p(table), i(tab.n), ll(tab.total), p(norm.record.buf), stream_ptr())
        return norm.record.norm.to(torch.float32)


def _bump_versions(params):
    """Raw-pointer writes bypass torch's version counter, on which the packed-weight caches key (complex_progress._PackCache):
    an in-place no-op per parameter would cost a launch each, so the counters are bumped directly."""
    torch._C._autograd._unsafe_set_version_counter(tuple(params), tuple(q._version + 1 for q in params))
