"""Streaming enhancement with a causal DCCRN (DCCRN-CL): chunked ``push`` / ``flush`` on the HIP kernels.

    st = StreamingDCCRN(model, batch=B)     # model: model.pvae_module.DCCRN_ with causal=True, parameters on the GPU
    y = st.push(x)                          # x: [B, n] float32 on the GPU, n >= 0 -> [B, m]: the samples that became final
    y = st.flush()                          # end of all B signals -> the remaining samples; the streamer is then reset

Concatenating every ``push`` output and the ``flush`` output gives ``model(x_full, train=False)[0]``.  Every block of the causal
model reads one frame of history, the LSTM is unidirectional and eval-mode batch norm is a per-channel affine map, so the only
look-ahead is the STFT window: frame t reads samples [hop*t - win/2, hop*t + win/2).  :class:`StreamPlan` holds the frame and
emission bookkeeping from which every kernel launch takes its ranges.

:class:`StreamingSessions` runs one such stream per slot, each starting and ending on its own; :class:`StreamingVAE` streams
the I-DCCRN-VAE pair (noisy encoder, latent draw, fine-tuned decoder with the noisy skips) under the same contract,
:class:`StreamingVAESessions` runs that pair one stream per slot, and :class:`StreamingVAETwoLatents` streams the two-latent
evaluation: speech and noise decoder on one encoder pass, then a mask estimator.  :class:`StreamingResampler` /
:class:`StreamingResamplerSessions` resample a stream under the same contract, bit-identical to ``inference.resample``, and
:class:`AtRate` / :class:`SessionsAtRate` put one in front of and one behind any of the streamers for signals at 48 or 44.1 kHz.
Every sessions class takes a slot's stream out as a :class:`SlotState` (``save``) and puts it into any slot of any object of the
same shape (``load``): moving, compacting, parking and persisting streams.
"""
from __future__ import annotations

import json
import struct
from collections.abc import Iterable, Sequence
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._lib import call, i, ll, p, stream_ptr
from .inference import OUTTYPES
from .ops import Planar


class Chunk(NamedTuple):
    """One launch group of a push: frames t0 .. t0+k-1 (k may be 0 at flush), output samples e0 .. e1-1, padded OLA positions
    up to p_end, carried overlap lengths in and out, and the history parity it reads (it writes 1 - parity)."""
    t0: int
    k: int
    e0: int
    e1: int
    p_end: int
    carry_in: int
    carry_out: int
    parity: int


class StreamPlan:
    """Frame and sample bookkeeping of a lock-step stream (host side only; no tensors).

    With half = n_fft/2 and left = (n_fft - win)/2, frame t reads original samples s = hop*t + lo + i, i in [0, win), lo = left -
    half, mirrored at the start (x[-s] = x[s]) and, at flush, at the end (x[L-1+j] = x[L-1-j]).  Before the end is known, frame t
    is computable once every sample it reads has arrived, the mirrored ones included; output sample m is final once every frame
    t with hop*t + left <= m + half is done."""

    def __init__(self, n_fft: int, hop: int, win: int, cap: int = 64):
        if not (0 < win <= n_fft and hop > 0 and cap > 0):
            raise ValueError("StreamPlan: need 0 < win <= n_fft, hop > 0, cap > 0")
        self.n_fft, self.hop, self.win, self.cap = n_fft, hop, win, cap
        self.half = n_fft // 2
        self.left = (n_fft - win) // 2
        self.lo = self.left - self.half              # first sample of frame 0 (before mirroring)
        self.hi = self.lo + win                      # one past its last sample
        self.ring = n_fft                            # input samples kept from push to push
        self.carry_cap = n_fft + win                 # overlap-add positions kept from push to push
        self.reset()

    def reset(self):
        self.n = 0            # samples received
        self.k = 0            # frames computed
        self.emitted = 0      # output samples returned
        self.carry = 0        # overlap-add positions carried
        self.parity = 0

    # -- formulas
    def frames_ready(self, n: int) -> int:
        """k(n): frames computable from the first n samples before the end is known."""
        need0 = max(self.hi, 1 - self.lo)            # frame 0: its last sample and its deepest start-mirror sample
        if n < need0:
            return 0
        return (n - self.hi) // self.hop + 1

    def final_samples(self, k: int) -> int:
        """Output samples final once frames 0 .. k-1 are done (before the end is known)."""
        return max(0, self.hop * k + self.lo)

    def total_frames(self, L: int) -> int:
        return 1 + L // self.hop

    def total_samples(self, L: int) -> int:
        return self.hop * (self.total_frames(L) - 1)

    def check_flush(self, L: int):
        if L <= self.half:
            raise ValueError(f"flush: {L} samples in total, but torch.stft's reflect padding needs more than n_fft/2 = {self.half}")

    # -- schedules (advance the state)
    def _chunks(self, k_to: int, L_end: Optional[int]) -> List[Chunk]:
        out = []
        while self.k < k_to or (L_end is not None and not out):
            kc = min(self.cap, k_to - self.k)
            t0 = self.k
            e1 = self.final_samples(t0 + kc)
            if L_end is not None:
                e1 = self.total_samples(L_end) if t0 + kc == k_to else min(e1, self.total_samples(L_end))
            p_start = self.half + self.emitted
            p_end = p_start + self.carry
            if kc > 0:
                p_end = max(p_end, self.hop * (t0 + kc - 1) + self.left + self.win)
            p_end = max(p_end, self.half + e1)
            carry_out = p_end - (self.half + e1)
            if carry_out > self.carry_cap:
                raise RuntimeError("StreamPlan: overlap-add carry exceeds its capacity")
            out.append(Chunk(t0, kc, self.emitted, e1, p_end, self.carry, carry_out, self.parity))
            self.k, self.emitted, self.carry = t0 + kc, e1, carry_out
            self.parity ^= 1
        return out

    def push(self, n_new: int) -> List[Chunk]:
        if n_new < 0:
            raise ValueError("push: negative sample count")
        k_to = self.frames_ready(self.n + n_new)
        chunks = self._chunks(k_to, None)
        self.n += n_new
        return chunks

    def flush(self) -> List[Chunk]:
        self.check_flush(self.n)
        return self._chunks(self.total_frames(self.n), self.n)


# One row of a launch group's table, as include/idccrn_hip.h lays it out (IDV_ROW_*)
ROW_FIELDS = ("n_prev", "count", "L_end", "t0", "k", "parity", "e0", "e1", "p_end", "carry_in", "T_total", "y_off")
NF = len(ROW_FIELDS)


class Group(NamedTuple):
    """One launch group of a sessions push: ``rows[b]`` is slot b's row of the table (ROW_FIELDS), ``k`` = max_b k_b sizes the
    launches (Tp = k + 1), ``span`` = the longest overlap-add range of a slot, ``flush``: the group reads from the ring only."""
    rows: List[List[int]]
    k: int
    span: int
    flush: bool


class SessionCall(NamedTuple):
    """What one ``push(counts, end)`` does: the launch groups (push phase first; the ring update follows the push phase), the
    number of output samples of each slot and the slots whose state is zeroed at the end."""
    groups: List[Group]
    m: List[int]
    zero: List[int]


class SessionPlan:
    """Host-side bookkeeping of ``slots`` independent streams in one batch (no tensors): every slot owns a :class:`StreamPlan`.

    Group g of the push phase holds chunk g of every slot that has one; after the ring update, the flush phase holds the flush
    chunks of the slots that end, read from the ring only (n_prev = L).  A slot without work in a group has k = 0 and e0 = e1:
    the kernels read and write nothing of it, and its parity does not flip, so no history has to be copied through."""

    def __init__(self, slots: int, n_fft: int, hop: int, win: int, cap: int = 64):
        if isinstance(slots, bool) or not isinstance(slots, int) or slots <= 0:
            raise ValueError("SessionPlan: slots must be a positive int")
        self.plans = [StreamPlan(n_fft, hop, win, cap) for _ in range(slots)]

    @property
    def positions(self) -> List[int]:
        return [pl.n for pl in self.plans]

    def snapshot(self):
        return [(pl.n, pl.k, pl.emitted, pl.carry, pl.parity) for pl in self.plans]

    def restore(self, snap):
        for pl, v in zip(self.plans, snap):
            pl.n, pl.k, pl.emitted, pl.carry, pl.parity = v

    def slot_state(self, b: int):
        """Slot b's host integers (n, k, emitted, carry, parity): its row of ``snapshot()``."""
        pl = self.plans[b]
        return (pl.n, pl.k, pl.emitted, pl.carry, pl.parity)

    def set_slot_state(self, b: int, v):
        self.check_slot_state(v)
        pl = self.plans[b]
        pl.n, pl.k, pl.emitted, pl.carry, pl.parity = v

    def check_slot_state(self, v):
        """The guard on a slot's host integers that come from outside (``load``): k, emitted and carry are functions of n alone
        (the frames that are ready, the samples they make final, the overlap behind them), so a fresh :class:`StreamPlan` that is
        pushed n samples must arrive at them; the parity counts launch groups and is only held to {0, 1}."""
        if (not isinstance(v, (tuple, list)) or len(v) != 5 or any(isinstance(q, bool) or not isinstance(q, int) for q in v)
                or v[0] < 0):
            raise ValueError("a slot's plan is five ints (n, k, emitted, carry, parity) with n >= 0")
        n, k, emitted, carry, parity = v
        one = self.plans[0]
        replay = StreamPlan(one.n_fft, one.hop, one.win, max(1, one.frames_ready(n)))      # one chunk, wherever the stream is
        replay.push(n)
        if (k, emitted, carry) != (replay.k, replay.emitted, replay.carry) or parity not in (0, 1):
            raise ValueError(f"a slot's plan (n, k, emitted, carry, parity) = {tuple(v)} is not one a stream of {n} samples "
                             f"reaches: k, emitted, carry must be {(replay.k, replay.emitted, replay.carry)} and parity 0 or 1")

    def check(self, counts: List[int], end: List[int]):
        """Every guard of a push, before anything changes."""
        for b in end:
            L_total = self.plans[b].n + counts[b]
            if L_total > 0:
                self.plans[b].check_flush(L_total)

    def push(self, counts: List[int], end: List[int]) -> SessionCall:
        self.check(counts, end)
        snap = self.snapshot()
        try:
            return self._push(counts, end)
        except Exception:
            self.restore(snap)
            raise

    def drop(self, slots: List[int]):
        for b in slots:
            self.plans[b].reset()

    def _group(self, chunks, n_prev, counts, ends, y_off, flush: bool) -> Group:
        rows, k, span = [], 0, 0
        for b, pl in enumerate(self.plans):
            c = chunks[b]
            if c is None:       # the slot sits this group out; its row states where it stands
                rows.append([n_prev[b], counts[b], -1, pl.k, 0, pl.parity, pl.emitted, pl.emitted, pl.half + pl.emitted + pl.carry,
                             pl.carry, -1, y_off[b]])
                continue
            if c.k == 0 and c.e0 == c.e1:
                raise RuntimeError("SessionPlan: a chunk without frames and without output")
            L_end = ends[b] if flush else -1
            rows.append([n_prev[b], counts[b], L_end, c.t0, c.k, c.parity, c.e0, c.e1, c.p_end, c.carry_in,
                         pl.total_frames(L_end) if flush else -1, y_off[b]])
            y_off[b] += c.e1 - c.e0
            k = max(k, c.k)
            span = max(span, c.p_end - (pl.half + c.e0))
        return Group(rows, k, span, flush)

    def _push(self, counts, end) -> SessionCall:
        S = len(self.plans)
        n_prev = [pl.n for pl in self.plans]
        chunks = [pl.push(counts[b]) for b, pl in enumerate(self.plans)]
        y_off = [0] * S
        groups = []
        # a call that brings samples has a push group even when no frame completes: the ring update reads its table
        for g in range(max(max(len(c) for c in chunks), 1 if any(counts) else 0)):
            groups.append(self._group([c[g] if g < len(c) else None for c in chunks], n_prev, counts, None, y_off, False))
        ending = sorted(b for b in set(end) if self.plans[b].n > 0)
        if ending:
            L_total = [pl.n for pl in self.plans]
            fl = [self.plans[b].flush() if b in ending else [] for b in range(S)]
            for g in range(max(len(c) for c in fl)):
                groups.append(self._group([c[g] if g < len(c) else None for c in fl], L_total, [0] * S, L_total, y_off, True))
            for b in ending:
                self.plans[b].reset()
        return SessionCall(groups, y_off, ending)


def check_model(model, batch) -> None:
    """The construction guards of StreamingDCCRN (host only, before any GPU work)."""
    from .model.pvae_module import DCCRN_
    if not isinstance(model, DCCRN_):
        raise ValueError("StreamingDCCRN takes a model.pvae_module.DCCRN_")
    net = model.std_DCCRN
    if not net.causal or any(e.conv._cfg[2][1] != 1 for e in net.encoders):
        raise ValueError("StreamingDCCRN needs a causal model (encoder time padding 1): with time padding 0 frame t needs x[t+1]")
    if model.recon_type not in ("mask", "real_imag"):
        raise ValueError(f"StreamingDCCRN: unknown recon_type {model.recon_type!r} (mask or real_imag)")
    if isinstance(batch, bool) or not isinstance(batch, int) or batch <= 0:
        raise ValueError("StreamingDCCRN: batch must be a positive int")
    if any(not q.is_cuda for q in model.parameters()) or any(not b.is_cuda for b in model.buffers()):
        raise RuntimeError("StreamingDCCRN runs on the MI355X only: move the model to the GPU first (there is no CPU path)")


def check_input(x, batch: int, device=None) -> None:
    """The guards of StreamingDCCRN.push (host only)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("push: x must be a tensor [batch, n]")
    if x.shape[0] != batch:
        raise ValueError(f"push: expected {batch} streams, got {x.shape[0]}")
    if not x.is_cuda:
        raise RuntimeError("StreamingDCCRN.push: pass a GPU (ROCm) tensor; there is no CPU path")
    if device is not None and x.device != device:
        raise RuntimeError(f"push: input on {x.device}, model on {device}")


def check_counts(counts, slots: int, n: int) -> List[int]:
    """The guards on the per-slot sample counts of StreamingSessions.push (host only) -> list of ints."""
    if counts is None:
        return [n] * slots
    if isinstance(counts, torch.Tensor):
        if counts.is_cuda:
            raise ValueError("counts must be a python sequence or a CPU integer tensor: they plan the launches on the host, and a "
                             "GPU tensor would have to be fetched with a synchronisation")
        if counts.dim() != 1 or counts.is_floating_point() or counts.is_complex() or counts.dtype == torch.bool:
            raise ValueError("counts must be a 1-D integer tensor")
        counts = counts.tolist()
    elif isinstance(counts, (str, bytes)) or not isinstance(counts, Sequence):
        raise ValueError("counts must be a python sequence or a CPU integer tensor")
    if any(isinstance(v, bool) or not isinstance(v, int) for v in counts):
        raise ValueError("counts must be integers (sample counts)")
    if len(counts) != slots:
        raise ValueError(f"{len(counts)} counts for {slots} slots")
    for b, v in enumerate(counts):
        if not 0 <= v <= n:
            raise ValueError(f"counts[{b}] = {v}: a count lies in 0 .. {n}, the width of x")
    return list(counts)


def check_slots(which, slots: int) -> List[int]:
    """A collection of slot numbers (``end=`` / ``drop``) -> sorted list without repeats (host only)."""
    if isinstance(which, torch.Tensor) or isinstance(which, (str, bytes)) or not isinstance(which, Iterable):
        raise ValueError("slots must be given as a python collection of ints")
    which = list(which)
    if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < slots for v in which):
        raise ValueError(f"slot numbers lie in 0 .. {slots - 1}")
    return sorted(set(which))


CONV_ENGINES = ("valu", "mfma", "bf16x3")


def check_conv(conv) -> str:
    """The guard on the ``conv=`` argument of both streamers (host only): the engine of the conv blocks."""
    if not isinstance(conv, str) or conv not in CONV_ENGINES:
        raise ValueError(f"conv must be one of {CONV_ENGINES} (vector-ALU, fp32-MFMA or split-bf16 MFMA streaming conv), got {conv!r}")
    return conv


def _fold_and_slope(block):
    return block.bn.eval_fold(), block.prelu.weight.detach().reshape(1).float().contiguous()


class _ConvPack:
    # engine: "valu" (idv_stream_cconv*), "mfma" (idv_stream_cconv_mfma*) or "bf16x3" (idv_stream_cconv_bf16*); w is the weight
    # pack of that engine
    __slots__ = ("w", "bias", "fold", "slope", "transposed", "C0", "C1", "Cout", "Fin", "Fout", "nsplit", "engine")


class _Launch(NamedTuple):
    """What the network needs of a sessions launch group: k_launch and the device pointer of its row table."""
    k: int
    rows: object


class _StreamBase:
    """What every streamer shares, whatever network it runs: the conv block packs of either engine (``_conv``, the batch an
    argument), the lock-step conv call, framing, ring update and overlap-add, and the list of per-stream state buffers."""

    _name = "StreamingDCCRN"       # in messages

    def reset(self):
        for t in self.state:
            t.zero_()

    def _conv(self, conv, blk, C0, C1, Fin, B, zero_skip=False):
        """``zero_skip``: a transposed block whose skip input is all zeros is packed with the first C0 input channels of its
        weights only (C1 = 0): the other channels would multiply zeros, and no zero buffer is ever read."""
        cp = _ConvPack()
        cp.transposed = conv._transposed
        re, im = conv._re, conv._im
        if zero_skip and (C1 != 0 or not cp.transposed or C0 > conv.in_channel):
            raise ValueError(f"{self._name}: a zero skip belongs to a transposed block called with C1 = 0")
        cin = C0 if zero_skip else (conv.in_channel if C1 == 0 else C0 + C1)
        cp.Cout = conv.out_channel
        cp.C0, cp.C1, cp.Fin = C0, C1, Fin
        cp.Fout = 2 * Fin - 1 if cp.transposed else (Fin - 1) // 2 + 1
        # the engine of a block is fixed here, from the constructor's choice and the block's shape alone
        # (conv="bf16x3": a block the split-bf16 entries do not serve gets what conv="mfma" would give it)
        tr = i(1 if cp.transposed else 0)
        bf16 = self.conv == "bf16x3" and L.lib().idv_stream_cconv_bf16_supported(tr, i(cin), i(cp.Cout)) == 1
        mfma = not bf16 and self.conv != "valu" and L.lib().idv_stream_cconv_mfma_supported(tr, i(cin), i(cp.Cout)) == 1
        cp.engine = "bf16x3" if bf16 else ("mfma" if mfma else "valu")
        cp.bias = torch.empty(2 * cp.Cout, dtype=torch.float32, device=self.device)
        # transposed-conv weights are [Cin][Cout][5][2]: the first cin input channels are a prefix
        wsrc = (p(re.weight.detach().float()[:cin if zero_skip else None].contiguous()),
                p(im.weight.detach().float()[:cin if zero_skip else None].contiguous()),
                p(re.bias.detach().float().contiguous()), p(im.bias.detach().float().contiguous()))
        if bf16:
            cp.w = torch.empty(int(L.lib().idv_stream_cconv_bf16_wfloats(i(cin), i(cp.Cout))), dtype=torch.float32, device=self.device)
            call("idv_stream_pack_cconv_bf16", wsrc[0], wsrc[1], wsrc[2], wsrc[3], i(cin), i(cp.Cout), i(1 if cp.transposed else 0),
                 p(cp.w), p(cp.bias), stream_ptr())
        elif mfma:
            cp.w = torch.empty(int(L.lib().idv_stream_cconv_mfma_wfloats(i(cin), i(cp.Cout))), dtype=torch.float32, device=self.device)
            call("idv_stream_pack_cconv_mfma", wsrc[0], wsrc[1], wsrc[2], wsrc[3], i(cin), i(cp.Cout), i(1 if cp.transposed else 0),
                 p(cp.w), p(cp.bias), stream_ptr())
        else:
            L.lib().idv_stream_cconv_wfloats.restype = L._L
            cp.w = torch.empty(int(L.lib().idv_stream_cconv_wfloats(i(cin), i(cp.Cout))), dtype=torch.float32, device=self.device)
            call("idv_stream_pack_cconv", wsrc[0], wsrc[1], wsrc[2], wsrc[3], i(cin), i(cp.Cout), i(1 if cp.transposed else 0),
                 p(cp.w), p(cp.bias), stream_ptr())
        cp.fold, cp.slope = _fold_and_slope(blk)
        cp.fold = cp.fold.clone()
        cp.nsplit = int(L.lib().idv_stream_cconv_splits(i(1 if cp.transposed else 0), i(cin), i(cp.Cout), i(Fin), i(B)))
        if cp.nsplit <= 0:
            raise ValueError(f"{self._name}: unsupported block shape")
        return cp

    def _pack_lstm(self, lstm, K: int):
        """The two-layer ComplexLSTM as the stream LSTM entries read it: the layer-0 projection for idv_pw_gemm (lstm_ih), the
        transposed W_hh0 / W_ih1 / W_hh1 of both parts (lstm_wt) and b_ih1 + b_hh1 (lstm_b1)."""
        self.H = lstm.hidden_size
        self.K = K
        sd = {k: v.detach().float().contiguous() for k, v in lstm.named_parameters()}
        H = self.H
        wih = torch.empty(ops.mtiles_alloc(8 * H) * ((K + 7) // 8 * 4) * 64, dtype=torch.float32, device=self.device)
        bih = torch.empty(ops.mtiles_alloc(8 * H) * 32, dtype=torch.float32, device=self.device)
        call("idv_pack_lstm_ih", p(sd["lstm_re.weight_ih_l0"]), p(sd["lstm_re.bias_ih_l0"]), p(sd["lstm_re.bias_hh_l0"]),
             p(sd["lstm_im.weight_ih_l0"]), p(sd["lstm_im.bias_ih_l0"]), p(sd["lstm_im.bias_hh_l0"]), i(H), i(K), p(wih), p(bih),
             stream_ptr())
        self.lstm_ih = (wih, bih)
        mats = []
        for part in ("lstm_re", "lstm_im"):
            for name in ("weight_hh_l0", "weight_ih_l1", "weight_hh_l1"):
                mats.append(sd[f"{part}.{name}"].t().contiguous())
        self.lstm_wt = torch.stack(mats).contiguous()
        self.lstm_b1 = torch.stack([sd[f"{part}.bias_ih_l1"] + sd[f"{part}.bias_hh_l1"] for part in ("lstm_re", "lstm_im")]).contiguous()

    def _conv_call(self, cp: _ConvPack, x0, h0, x1, h1, out, hist_out, x0hist_out, B, k, Tp, Jp):
        # one call per engine, each with its entry's name as a literal: the static check of the call sites against the header
        # (tests/test_host_cpu.py) reads literal names only, and a name picked at run time would go unchecked
        if cp.engine == "mfma":
            call("idv_stream_cconv_mfma", x0, p(h0), i(cp.C0), x1 if x1 is not None else p(None), p(h1), i(cp.C1), p(cp.w), p(cp.bias),
                 p(cp.fold), p(cp.slope), out, p(hist_out), x0hist_out, p(self.work), i(cp.nsplit), i(1 if cp.transposed else 0),
                 i(cp.Cout), i(cp.Fin), i(B), i(k), i(Tp), i(Jp), stream_ptr())
            return
        if cp.engine == "bf16x3":
            call("idv_stream_cconv_bf16", x0, p(h0), i(cp.C0), x1 if x1 is not None else p(None), p(h1), i(cp.C1), p(cp.w), p(cp.bias),
                 p(cp.fold), p(cp.slope), out, p(hist_out), x0hist_out, p(self.work), i(cp.nsplit), i(1 if cp.transposed else 0),
                 i(cp.Cout), i(cp.Fin), i(B), i(k), i(Tp), i(Jp), stream_ptr())
            return
        call("idv_stream_cconv", x0, p(h0), i(cp.C0), x1 if x1 is not None else p(None), p(h1), i(cp.C1), p(cp.w), p(cp.bias),
             p(cp.fold), p(cp.slope), out, p(hist_out), x0hist_out, p(self.work), i(cp.nsplit), i(1 if cp.transposed else 0),
             i(cp.Cout), i(cp.Fin), i(B), i(k), i(Tp), i(Jp), stream_ptr())

    def _conv_call_rows(self, cp: _ConvPack, x0, h0, x1, h1, out, hist, x0hist, B, k, Tp, Jp, rows):
        """The sessions form: the [2][...] histories whole (row b reads half parity_b and writes the other) and the table."""
        if cp.engine == "mfma":                  # a literal call site per engine, as in _conv_call
            call("idv_stream_cconv_mfma_rows", x0, p(h0), i(cp.C0), x1 if x1 is not None else p(None), p(h1), i(cp.C1), p(cp.w),
                 p(cp.bias), p(cp.fold), p(cp.slope), out, p(hist), p(x0hist), p(self.work), i(cp.nsplit),
                 i(1 if cp.transposed else 0), i(cp.Cout), i(cp.Fin), i(B), i(k), i(Tp), i(Jp), rows, stream_ptr())
            return
        if cp.engine == "bf16x3":
            call("idv_stream_cconv_bf16_rows", x0, p(h0), i(cp.C0), x1 if x1 is not None else p(None), p(h1), i(cp.C1), p(cp.w),
                 p(cp.bias), p(cp.fold), p(cp.slope), out, p(hist), p(x0hist), p(self.work), i(cp.nsplit),
                 i(1 if cp.transposed else 0), i(cp.Cout), i(cp.Fin), i(B), i(k), i(Tp), i(Jp), rows, stream_ptr())
            return
        call("idv_stream_cconv_rows", x0, p(h0), i(cp.C0), x1 if x1 is not None else p(None), p(h1), i(cp.C1), p(cp.w), p(cp.bias),
             p(cp.fold), p(cp.slope), out, p(hist), p(x0hist), p(self.work), i(cp.nsplit), i(1 if cp.transposed else 0), i(cp.Cout),
             i(cp.Fin), i(B), i(k), i(Tp), i(Jp), rows, stream_ptr())

    # ------------------------------------------------------------------ the lock-step signal ends (scalars, one StreamPlan)
    @staticmethod
    def _pitched(x: torch.Tensor, B: int):
        """push's input as the kernels read it: float32 rows at any pitch (a column slice of a longer signal costs no copy);
        anything else is made contiguous -> (x, row pitch, samples)."""
        x = x.float()
        n_new = int(x.shape[1])
        if (n_new > 1 and x.stride(1) != 1) or (B > 1 and x.stride(0) < n_new):
            x = x.contiguous()
        return x, (x.stride(0) if B > 1 else n_new), n_new

    def _lock_frames(self, c: Chunk, io, frames, Tp: int, Jp: int):
        x, ldx, n_new, n_prev, L_end = io
        call("idv_stream_frames", p(self.ring), i(self.plan.ring), p(x) if x is not None else p(None), ll(ldx), i(n_new), ll(n_prev),
             ll(L_end if L_end is not None else -1), i(self.B), i(self.n_fft), i(self.win), i(self.hop), ll(c.t0), i(c.k), frames,
             i(Tp), i(Jp), stream_ptr())

    def _lock_ring(self, x, ldx: int, n_new: int, n_prev: int):
        if n_new:
            call("idv_stream_ring", p(self.ring), i(self.plan.ring), p(x), ll(ldx), i(n_new), ll(n_prev), i(self.B), stream_ptr())

    def _lock_ola(self, c: Chunk, frames, carry, B: int, T_total: int, y, m: int, y_off: int):
        """Overlap-add of chunk c's inverse-DFT frames (``frames``: a Planar, None when c.k == 0) for B rows; carry [2][B * cap]."""
        pin = c.parity
        Tp = c.k + 1
        Jp = Planar.jp_for(B, Tp)
        call("idv_stream_ola", frames.ptr() if frames is not None else p(None), i(Tp), i(Jp), p(carry[pin]), i(c.carry_in),
             p(carry[1 - pin]), i(self.plan.carry_cap), i(B), i(self.n_fft), i(self.win), i(self.hop), ll(c.t0), i(c.k),
             ll(T_total), ll(c.e0), ll(c.e1), ll(c.p_end), p(y) if m else p(None), i(max(m, 1)), ll(y_off), stream_ptr())


class _Streamer(_StreamBase):
    """What both DCCRN streamers share: the construction guards, the packed weights, the activation and state buffers, and the
    network over the frames of one launch group.  A subclass supplies the framing, the conv block and the LSTM of its kind
    (scalars for lock-step streams, a row table for sessions)."""

    def __init__(self, model, batch: int, frames_per_launch: int = 64, max_columns: int = 4096, conv: str = "valu"):
        self.conv = check_conv(conv)
        check_model(model, batch)
        net = model.std_DCCRN
        params = list(model.parameters())
        if len(net.lstms) != 1 or not L.lib().idv_stream_lstm_supported(i(net.lstms[0].hidden_size)) or net.lstms[0].num_layer != 2:
            raise ValueError("StreamingDCCRN: one two-layer ComplexLSTM with hidden size 128 is supported")
        for blk in list(net.encoders) + list(net.decoders):
            (blk.conv if hasattr(blk, "conv") else blk.transconv)._check_supported()
        self.model, self.B = model, batch
        self.device = params[0].device
        st = model.stft
        self.n_fft, self.hop, self.win = st.n_fft, st.hop_length, st.win_length
        self.F = self.n_fft // 2 + 1
        self.cap = max(1, min(frames_per_launch, max_columns // batch))
        self.plan = StreamPlan(self.n_fft, self.hop, self.win, self.cap)
        self.skip_to_use = list(net.skip_to_use)
        with torch.no_grad(), torch.cuda.device(self.device):
            self._pack(model)
            self._alloc()
        self.reset()

    # ------------------------------------------------------------------ construction
    def _pack(self, model):
        net = model.std_DCCRN
        F = self.F
        self.enc = []
        ch, Fin = 1, F
        self.enc_shapes = []                       # (C, F) of every encoder output
        for blk in net.encoders:
            cp = self._conv(blk.conv, blk, ch, 0, Fin, self.B)
            self.enc.append(cp)
            ch, Fin = cp.Cout, cp.Fout
            self.enc_shapes.append((ch, Fin))
        self.top = (ch, Fin)
        self.dec = []
        n = len(net.encoders)
        dch = net.dense.out_channel // Fin
        if dch * Fin != net.dense.out_channel:
            raise ValueError("StreamingDCCRN: dense output does not match the top encoder shape")
        c, f = dch, Fin
        for di, blk in enumerate(net.decoders):
            c1 = self.enc_shapes[n - 1 - di][0] if di in self.skip_to_use else 0
            if c + c1 != blk.transconv.in_channel:
                raise ValueError("StreamingDCCRN: decoder input channels do not match")
            cp = self._conv(blk.transconv, blk, c, c1, f, self.B)
            self.dec.append(cp)
            c, f = cp.Cout, cp.Fout
        if (c, f) != (1, F):
            raise ValueError("StreamingDCCRN: the last decoder must give one channel of n_fft/2 + 1 bins")
        self.conv_engines = [cp.engine for cp in self.enc + self.dec]      # enc0 .. then dec0 ..: nothing falls back unseen
        self._pack_lstm(net.lstms[0], ch * Fin)
        dn = net.dense
        self.dense = [ops.pack_pw(dn.linear_read.weight.detach().float(), dn.linear_read.bias.detach().float()),
                      ops.pack_pw(dn.linear_imag.weight.detach().float(), dn.linear_imag.bias.detach().float())]
        self.dense_out = (dch, Fin)
        dft = ops.DftPlan(self.n_fft, self.win, self.hop, 1, self.device)
        self.dft_fwd, self.dft_inv = dft.fwd, dft.inv
        self.datanorm = model.datanorm
        if self.datanorm:
            self.mean = model.data_mean.reshape(-1).float().contiguous().clone()
            self.std = model.data_std.reshape(-1).float().contiguous().clone()
        self.recon = model.recon_type

    def _alloc(self):
        B, dev = self.B, self.device
        Tp = self.cap + 1
        self.Jp_max = Planar.jp_for(B, Tp)
        mk = lambda C, F: Planar.empty(C, F, B, self.cap, Tp, dev, zero=True)
        self.fr = mk(1, self.win // 2)                       # frames [win][Jp]
        self.X = mk(1, self.F)
        self.N = mk(1, self.F) if self.datanorm else self.X
        self.enc_out = [mk(c, f) for c, f in self.enc_shapes]
        self.lat = mk(self.H, 1)
        self.dense_buf = mk(*self.dense_out)
        self.dec_out = [mk(cp.Cout, cp.Fout) for cp in self.dec]
        self.pred = mk(1, self.F)
        self.pred2 = mk(1, self.F) if self.datanorm else None
        self.pc = torch.empty(B * self.F * self.cap * 2, dtype=torch.float32, device=dev)
        self.ifr = mk(1, self.win // 2)
        J = B * self.cap
        self.G = torch.empty(2 * J * 8 * self.H, dtype=torch.float32, device=dev)
        self.hout = torch.empty(4 * J * self.H, dtype=torch.float32, device=dev)
        work = max([cp.nsplit * 2 * cp.Cout * cp.Fout * J for cp in self.enc + self.dec if cp.nsplit > 1] + [0])
        self.work = torch.empty(max(work, 1), dtype=torch.float32, device=dev)
        # per-stream state
        hist = lambda C, F: torch.zeros(2, 2 * C * F * B, dtype=torch.float32, device=dev)
        self.h_in = hist(1, self.F)
        self.h_enc = [hist(c, f) for c, f in self.enc_shapes]
        self.h_dense = hist(*self.dense_out)
        self.h_dec = [hist(cp.Cout, cp.Fout) for cp in self.dec[:-1]]
        self.lstm_state = torch.zeros(4 * 4 * B * self.H, dtype=torch.float32, device=dev)
        self.ring = torch.zeros(B * self.plan.ring, dtype=torch.float32, device=dev)
        self.carry = torch.zeros(2, B * self.plan.carry_cap, dtype=torch.float32, device=dev)
        self.state = [self.h_in, self.h_dense, self.lstm_state, self.ring, self.carry] + self.h_enc + self.h_dec

    # ------------------------------------------------------------------ the network over one launch group
    def _network(self, c, io):
        """Frames -> spectrum -> encoders -> LSTM -> dense -> decoders -> mask -> windowed inverse-DFT frames (self.ifr) for the
        c.k columns per stream of launch group c; ``io`` is what the subclass's framing needs."""
        B, k = self.B, c.k
        Tp = k + 1
        Jp = Planar.jp_for(B, Tp)
        s = stream_ptr()
        ptr = lambda pl, plane=0: L._P(pl.buf.data_ptr() + 4 * (ops.SLACK + plane * pl.F * Jp))
        self._frames(c, io, ptr(self.fr), Tp, Jp)
        ops.pw_gemm(ptr(self.fr), self.win, self.dft_fwd[0], self.dft_fwd[1], 2 * self.F, B, Tp, Jp, k, ptr(self.X))
        if self.datanorm:
            call("idv_datanorm", ptr(self.X), p(self.mean), p(self.std), i(self.F), i(B), i(k), i(Tp), i(Jp), ptr(self.N), s)
        # encoders
        src, hsrc = self.N, self.h_in
        for e, cp in enumerate(self.enc):
            out = self.enc_out[e]
            self._block(cp, c, ptr(src), hsrc, None, None, ptr(out), self.h_enc[e], self.h_in if e == 0 else None, Tp, Jp)
            src, hsrc = out, self.h_enc[e]
        # LSTM: layer-0 projection of both input parts (idv_pw_gemm as offline), then the stateful recurrence
        H, K = self.H, self.K
        wih, bih = self.lstm_ih
        top = self.enc_out[-1]
        for z in range(2):
            ops.pw_gemm(ptr(top, z * top.C), K, wih, bih, 8 * H, B, Tp, Jp, k,
                        L._P(self.G.data_ptr() + 4 * z * k * B * 8 * H), swap=True, ldo=8 * H)
        self._lstm(c, ptr(self.lat), Tp, Jp)
        # dense
        dc, df = self.dense_out
        for ri, pk in enumerate(self.dense):
            ops.pw_gemm(ptr(self.lat, ri * H), H, pk[0], pk[1], dc * df, B, Tp, Jp, k, ptr(self.dense_buf, ri * dc))
        # decoders
        src, hsrc = self.dense_buf, self.h_dense
        n = len(self.enc)
        for di, cp in enumerate(self.dec):
            out = self.dec_out[di]
            skip = n - 1 - di if di in self.skip_to_use else None
            x1 = ptr(self.enc_out[skip]) if skip is not None else None
            h1 = self.h_enc[skip] if skip is not None else None
            hout = self.h_dec[di] if di < len(self.h_dec) else None      # nothing reads the last block's history
            self._block(cp, c, ptr(src), hsrc, x1, h1, ptr(out), hout, self.h_dense if di == 0 else None, Tp, Jp)
            if di < len(self.h_dec):
                src, hsrc = out, self.h_dec[di]
        mask = self.dec_out[-1]
        if self.recon == "mask":
            call("idv_mask_apply", ptr(mask), ptr(self.N), i(1), i(Jp), ptr(self.pred), p(None), i(self.F), i(B), i(k), i(Tp), i(Jp), s)
            pred = self.pred
        else:
            pred = mask
        if self.datanorm:
            call("idv_datadenorm", ptr(pred), p(self.mean), p(self.std), i(self.F), i(B), i(k), i(Tp), i(Jp), ptr(self.pred2),
                 p(self.pc), s)
            pred = self.pred2
        ops.pw_gemm(ptr(pred), 2 * self.F, self.dft_inv[0], self.dft_inv[1], self.win, B, Tp, Jp, k, ptr(self.ifr))

class StreamingDCCRN(_Streamer):
    """Lock-step streaming inference of a causal ``DCCRN_`` (DCCRN-CL) for ``batch`` signals.

    ``push(x)`` takes the next ``n >= 0`` samples of every stream (``x``: ``[batch, n]`` float32 on the model's GPU) and returns
    the ``[batch, m]`` output samples that became final; ``flush()`` ends the signals, returns the rest and resets the streamer for
    the next signals.  All pushes and the flush together return exactly what ``model(x_full, train=False)[0]`` returns
    (``hop * floor(L / hop)`` samples, eval-mode semantics with the batch norm folded).  Output sample m is returned by the push
    that delivers input sample m + 300 ... m + 399 at n_fft 512, win 400, hop 100.

    ``conv`` names the engine of the conv blocks: ``"valu"`` (default, vector ALU) or ``"mfma"`` (fp32 matrix cores for every
    block with at least 16 output channels, the others stay on the vector ALU; ``conv_engines`` lists the engine per block,
    enc0 .. then dec0 ..).  The engine is fixed at construction and both give the same bits, so outputs of the two can be mixed.
    ``"bf16x3"`` runs every block with at least 16 output and 4 input channels in split-bf16 arithmetic on the bf16 matrix cores
    (three MFMAs per product, fp32 accumulation and fp32 state; the other blocks get what ``"mfma"`` would give them).  Its
    result is the same bits however the signal is cut into pushes, but not the bits of the fp32 engines: it stands within the
    streaming tolerance (1e-4 relative) of them.

    Without ``conv="bf16x3"`` the streamer runs in exact fp32; ``ops.PRECISION`` is never read.  Weights are packed once, at
    construction: later changes of the model's parameters are not seen by an existing streamer.
    """

    def reset(self):
        """Zero every per-stream state buffer and the bookkeeping (done by construction and by flush)."""
        super().reset()
        self.plan.reset()

    # ------------------------------------------------------------------ push / flush
    def push(self, x: torch.Tensor) -> torch.Tensor:
        check_input(x, self.B, self.device)
        x, ldx, n_new = self._pitched(x, self.B)
        n_prev = self.plan.n
        with torch.cuda.device(self.device):
            chunks = self.plan.push(n_new)
            y = self._run(chunks, x, ldx, n_new, n_prev, None)
            self._lock_ring(x, ldx, n_new, n_prev)
        return y

    def flush(self) -> torch.Tensor:
        L_total = self.plan.n
        self.plan.check_flush(L_total)
        with torch.cuda.device(self.device):
            chunks = self.plan.flush()
            y = self._run(chunks, None, 0, 0, L_total, L_total)
            self.reset()
        return y

    def _run(self, chunks: List[Chunk], x, ldx: int, n_new: int, n_prev: int, L_end: Optional[int]) -> torch.Tensor:
        m = (chunks[-1].e1 - chunks[0].e0) if chunks else 0
        y = torch.empty(self.B, m, dtype=torch.float32, device=self.device)
        T_total = self.plan.total_frames(L_end) if L_end is not None else -1
        for c in chunks:
            if c.k > 0:
                self._network(c, (x, ldx, n_new, n_prev, L_end))
            self._lock_ola(c, self.ifr if c.k > 0 else None, self.carry, self.B, T_total, y, m, c.e0 - chunks[0].e0)
        return y

    # ------------------------------------------------------------------ the lock-step kernels of the network
    def _frames(self, c: Chunk, io, frames, Tp: int, Jp: int):
        self._lock_frames(c, io, frames, Tp, Jp)

    def _block(self, cp: _ConvPack, c: Chunk, x0, h0, x1, h1, out, hist, x0hist, Tp: int, Jp: int):
        """One conv block: histories are read from half c.parity of the [2][...] buffers and written to the other half."""
        P = c.parity
        self._conv_call(cp, x0, h0[P], x1, h1[P] if h1 is not None else None, out, hist[1 - P] if hist is not None else None,
                        p(x0hist[1 - P]) if x0hist is not None else p(None), self.B, c.k, Tp, Jp)

    def _lstm(self, c: Chunk, out, Tp: int, Jp: int):
        call("idv_stream_clstm", p(self.G), p(self.lstm_wt), p(self.lstm_b1), p(self.lstm_state), p(self.hout), out, i(self.H),
             i(self.B), i(c.k), i(Tp), i(Jp), stream_ptr())


STATE_KINDS = ("dccrn", "vae", "two_latents", "resampler", "at_rate")
_STATE_MAGIC = b"IDVSLOT\x00"
_STATE_VERSION = 1


def _as_tuple(v):
    """JSON gives lists back where tuples went in."""
    return tuple(_as_tuple(q) for q in v) if isinstance(v, (list, tuple)) else v


class SlotState:
    """The stream of one slot of a sessions object, as ``save`` returns it and ``load`` takes it.

    ``kind``: the class family, one of ``STATE_KINDS``; ``layout``: a tuple that fingerprints what the floats mean (n_fft, hop,
    win, the (outer, inner) of every state view in order, for the VAE kinds also ns, zdim, H, latent or outtype / phase, average;
    for resamplers up, down, H); ``plan``: the slot's host integers (``SessionPlan.slot_state``: n, k, emitted, carry, parity; a
    resampler's: n, parity); ``seed`` / ``draw_slot``: the key and the slot number a VAE stream draws with (else None); ``data``:
    the slot's record, float32 ``[per_slot]`` on a device or on the CPU.  A state of kind ``"at_rate"`` has no floats of its own:
    ``stages`` holds the states of its three stages (down-resampler, network, up-resampler).

    ``kind`` and ``layout`` say nothing about the weights: loading a state into a streamer with other weights of the same layout
    is not detected and gives the output of neither model.
    """

    __slots__ = ("kind", "layout", "plan", "seed", "draw_slot", "data", "stages")

    def __init__(self, kind, layout, plan, data, seed=None, draw_slot=None, stages=None):
        self.kind, self.layout, self.plan, self.data = kind, _as_tuple(layout), _as_tuple(plan), data
        self.seed, self.draw_slot, self.stages = seed, draw_slot, (tuple(stages) if stages is not None else None)

    def __repr__(self):
        return f"SlotState(kind={self.kind!r}, plan={self.plan}, floats={self.data.numel()}, device={self.data.device})"

    def to(self, device) -> "SlotState":
        """The same state with its floats on ``device`` (a copy only where they are elsewhere)."""
        return SlotState(self.kind, self.layout, self.plan, self.data.to(device), self.seed, self.draw_slot,
                         [s.to(device) for s in self.stages] if self.stages is not None else None)

    def cpu(self) -> "SlotState":
        return self.to("cpu")

    def tobytes(self) -> bytes:
        """Magic, version (uint32), header length (uint32), a JSON header, then the payload: the floats as little-endian
        float32, or for an ``at_rate`` state the bytes of its stages one after the other (their lengths in the header)."""
        if self.stages is not None:
            parts = [s.tobytes() for s in self.stages]
            payload = b"".join(parts)
        else:
            parts = None
            payload = self.data.detach().cpu().contiguous().numpy().astype("<f4", copy=False).tobytes()
        head = json.dumps({"kind": self.kind, "layout": self.layout, "plan": self.plan, "seed": self.seed,
                           "draw_slot": self.draw_slot, "floats": None if parts is not None else int(self.data.numel()),
                           "stages": [len(q) for q in parts] if parts is not None else None}).encode()
        return _STATE_MAGIC + struct.pack("<II", _STATE_VERSION, len(head)) + head + payload

    @staticmethod
    def frombytes(b) -> "SlotState":
        """The state ``tobytes`` wrote (its floats on the CPU); ``ValueError`` for anything else: every length is checked."""
        if not isinstance(b, (bytes, bytearray, memoryview)):
            raise ValueError("SlotState.frombytes takes bytes")
        b = bytes(b)
        fixed = len(_STATE_MAGIC) + 8
        if len(b) < fixed or b[:len(_STATE_MAGIC)] != _STATE_MAGIC:
            raise ValueError("not a SlotState: the magic is missing")
        version, hlen = struct.unpack("<II", b[len(_STATE_MAGIC):fixed])
        if version != _STATE_VERSION:
            raise ValueError(f"SlotState version {version}; this package reads version {_STATE_VERSION}")
        if hlen > len(b) - fixed:
            raise ValueError("SlotState: truncated header")
        try:
            head = json.loads(b[fixed:fixed + hlen].decode())
        except (UnicodeDecodeError, ValueError):
            raise ValueError("SlotState: the header is not JSON") from None
        if not isinstance(head, dict) or set(head) != {"kind", "layout", "plan", "seed", "draw_slot", "floats", "stages"}:
            raise ValueError("SlotState: the header does not have the fields of this version")
        is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
        if (head["kind"] not in STATE_KINDS or not isinstance(head["layout"], list) or not isinstance(head["plan"], list)
                or not all(is_int(v) for v in head["plan"])
                or not all(v is None or is_int(v) for v in (head["seed"], head["draw_slot"]))):
            raise ValueError("SlotState: a header field has the wrong type")
        payload = b[fixed + hlen:]
        floats, lens = head["floats"], head["stages"]
        if (floats is None) == (lens is None) or (lens is None) == (head["kind"] == "at_rate"):
            raise ValueError("SlotState: a state holds either floats or, for kind 'at_rate', stages")
        if lens is None:
            if not is_int(floats) or floats < 0 or len(payload) != 4 * floats:
                raise ValueError(f"SlotState: the header announces {floats} floats, the payload has {len(payload)} bytes")
            data = torch.from_numpy(np.frombuffer(payload, dtype="<f4").astype(np.float32))
            stages = None
        else:
            if not isinstance(lens, list) or not all(is_int(v) and v >= 0 for v in lens) or sum(lens) != len(payload):
                raise ValueError("SlotState: the stage lengths do not add up to the payload")
            stages, at = [], 0
            for n in lens:
                stages.append(SlotState.frombytes(payload[at:at + n]))
                at += n
            data = torch.empty(0, dtype=torch.float32)
        return SlotState(head["kind"], head["layout"], head["plan"], data, head["seed"], head["draw_slot"], stages)


def _slot_list(which, slots: int, what: str) -> List[int]:
    """Slot numbers of ``save`` / ``load`` in the caller's order (state j belongs to slot j of the list); no slot twice."""
    if isinstance(which, torch.Tensor) or isinstance(which, (str, bytes)) or not isinstance(which, Iterable):
        raise ValueError(f"{what}: slots must be given as a python collection of ints")
    which = list(which)
    if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < slots for v in which):
        raise ValueError(f"{what}: slot numbers lie in 0 .. {slots - 1}")
    if len(set(which)) != len(which):
        raise ValueError(f"{what}: a slot appears twice")
    return which


class _Slots:
    """What every sessions class shares (``self.B`` slots on ``self.device``): the per-slot host plan ``self.sessions``,
    ``positions``, ``drop`` / ``reset``, the one pinned copy that takes a call's tables to the device, and the zeroing of the
    slots that end; ``self._zero_views`` lists the state buffers as (buffer, outer, inner) of a [outer][slots][inner] view.
    For the sessions classes of the network, mixed in in front of their streamer: ``push``, written once, and the framing.  Such
    a class supplies what differs: ``_tables`` (the host layout of a call's tables), ``_launch`` (what its network needs of a
    launch group), ``_ola_site`` (where the overlap-add runs) and ``_finish`` (what follows it)."""

    def _init_slots(self):
        """The plan and the tables of a network's sessions: one row table (ROW_FIELDS) per launch group."""
        if int(L.lib().idv_stream_row_fields()) != NF:
            raise L.IdvError("libidccrn_hip.so and streaming.ROW_FIELDS disagree about the row table")
        self._init_tables(SessionPlan(self.B, self.n_fft, self.hop, self.win, self.cap), 4 * self.B * NF)

    def _init_tables(self, sessions, table_min: int = 0):
        self.sessions = sessions    # the host plan: positions, snapshot / restore, push(counts, end), drop(slots)
        self._table_min = table_min
        self._table = None          # device int64 buffer of the call's tables; it only grows
        self._staging = []          # [(pinned int64 buffer, event of the copy that last read it)] * 2
        self._turn = 0
        self._state_tab = None      # (host view table, its device copy, floats per slot) of save / load, built at first use

    @property
    def positions(self) -> List[int]:
        return self.sessions.positions

    # ------------------------------------------------------------------ save / load of a slot's stream
    def _state_views(self):
        """The view table of idv_stream_state_gather / _scatter from ``_zero_views`` -> (host int64 [n_views][4], its device
        copy, floats per slot).  Built once: the state buffers are allocated at construction and never move."""
        if self._state_tab is None:
            rows, off = [], 0
            for buf, outer, inner in self._zero_views:
                if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.numel() != outer * self.B * inner:
                    raise L.IdvError("a state view does not cover its buffer as [outer][slots][inner] float32")
                rows += [buf.data_ptr(), outer, inner, off]
                off += outer * inner
            host = torch.tensor(rows, dtype=torch.int64)
            self._state_tab = (host, host.to(self.device), off)
        return self._state_tab

    def _state_layout(self):
        return self._state_head() + (tuple((int(o), int(n)) for _, o, n in self._zero_views),) + self._state_extra()

    def _state_head(self):
        return (self.n_fft, self.hop, self.win)

    def _state_extra(self):
        return ()

    def _state_of(self, b: int, data: torch.Tensor) -> "SlotState":
        return SlotState(self._state_kind, self._state_layout(), self.sessions.slot_state(b), data)

    def _state_table_check(self, slots: List[int], what: str):
        """A bad table never reaches a kernel: both host tables are held to idv_stream_state_check."""
        host, _, per = self._state_views()
        sl = torch.tensor(slots, dtype=torch.int64)
        rc = L.lib().idv_stream_state_check(L._P(host.data_ptr()), host.numel() // 4, self.B, L._P(sl.data_ptr()), len(slots), per)
        if rc != 0:
            raise ValueError(f"{what}: idv_stream_state_check refused the tables (status {rc})")
        return sl

    def save(self, slots) -> List["SlotState"]:
        """The streams of these slots as they stand, one :class:`SlotState` per slot in the order given: one gather launch on
        the current stream and no host synchronisation; the ``data`` of the states are rows of one device tensor.  The slots
        are untouched: saving is a fork, and a caller that means a move ``drop``s them afterwards.

        A state may be loaded into ANY slot of any sessions object of the same kind and layout (``load``), on any device, with
        any conv engine and any ``frames_per_launch``.  Into an object with the same number of slots and the same arithmetic
        (``"valu"`` and ``"mfma"`` are one arithmetic, ``"bf16x3"`` another) the stream continues bit for bit as if it had never
        moved; into one with another number of slots it continues within the streaming tolerance (1e-4 relative), because the K
        split of the conv blocks depends on the batch, and so it does between ``"bf16x3"`` and an fp32 engine: the state is fp32
        in both, the products are not.  The weights are the
        caller's to match: nothing in a state identifies them."""
        slots = _slot_list(slots, self.B, "save")
        if not slots:
            return []
        sl = self._state_table_check(slots, "save")
        _, views, per = self._state_views()
        with torch.cuda.device(self.device):
            out = torch.empty(len(slots), per, dtype=torch.float32, device=self.device)
            table = self._upload(sl)
            call("idv_stream_state_gather", p(views), i(views.numel() // 4), i(self.B), L._P(table.data_ptr()), i(len(slots)), p(out),
                 ll(per), stream_ptr())
        return [self._state_of(b, out[j]) for j, b in enumerate(slots)]

    def load(self, slots, states, overwrite: bool = False):
        """Put ``states[j]`` (from ``save``, possibly by way of ``.cpu()`` / ``tobytes()`` / another device) into slot
        ``slots[j]``, which then continues that stream.  Every guard runs on the host before any GPU work and before any
        bookkeeping changes (``ValueError``): as many states as slots, no slot twice, ``kind`` and ``layout`` equal to this
        object's, a plan that a stream of its n samples reaches, and a target at position 0 unless ``overwrite=True`` (the
        stream it served is then abandoned without output).  Then one upload (states on the CPU travel with the slot list in
        the one pinned copy), one scatter launch, and the slots' plans are set.

        The conv engine is no part of a state: every engine keeps its state in fp32.  A state saved by a ``conv="bf16x3"``
        object continues in an fp32-engine object (and the other way round) within the streaming tolerance, not bit for bit."""
        slots = self._load_check(slots, states, overwrite)
        self._load_apply(slots, states)

    def _load_check(self, slots, states, overwrite: bool) -> List[int]:
        """Every guard of ``load``; nothing changes -> the slot list."""
        slots = _slot_list(slots, self.B, "load")
        if isinstance(states, SlotState) or not isinstance(states, Iterable):
            raise ValueError("load: states must be a list of SlotState, one per slot")
        states = list(states)
        if len(states) != len(slots):
            raise ValueError(f"load: {len(states)} states for {len(slots)} slots")
        if not slots:
            return slots
        layout, per = self._state_layout(), self._state_views()[2]
        pos = self.positions
        for b, st in zip(slots, states):
            if not isinstance(st, SlotState):
                raise ValueError("load: states must be a list of SlotState, one per slot")
            if st.kind != self._state_kind:
                raise ValueError(f"load: a state of kind {st.kind!r} does not fit {type(self).__name__} (kind {self._state_kind!r})")
            if st.layout != layout:
                raise ValueError(f"load: the state's layout {st.layout} is not this object's {layout}: another model shape, "
                                 "n_fft / hop / win or class options")
            d = st.data
            if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or d.dim() != 1 or d.numel() != per:
                raise ValueError(f"load: a state's data must be a float32 tensor of {per} floats")
            self.sessions.check_slot_state(st.plan)
            self._state_check_extra(st)
            if pos[b] and not overwrite:
                raise ValueError(f"load: slot {b} is {pos[b]} samples into a signal; end or drop it first, or pass overwrite=True")
        self._state_table_check(slots, "load")
        return slots

    def _state_check_extra(self, st: "SlotState"):
        pass

    def _load_apply(self, slots: List[int], states):
        if not slots:
            return
        states = list(states)
        _, views, per = self._state_views()
        n = len(slots)
        with torch.cuda.device(self.device):
            if all(st.data.device.type == "cpu" for st in states):
                # the slot list and the records in one pinned copy: the floats ride behind the slots, two to an int64
                host = torch.zeros(n + (n * per + 1) // 2, dtype=torch.int64)
                host[:n] = torch.tensor(slots, dtype=torch.int64)
                host[n:].view(torch.float32)[:n * per].copy_(torch.cat([st.data for st in states]))
                table = self._upload(host)
                rec = L._P(table.data_ptr() + 8 * n)
            else:
                first = states[0].data
                rows = all(st.data.device == self.device and st.data.is_contiguous() and
                           st.data.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and
                           st.data.data_ptr() == first.data_ptr() + 4 * per * j for j, st in enumerate(states))
                # rows of one tensor on this device, in order (what save returned): read where they lie; else gathered here
                keep = first if rows else torch.stack([st.data.to(self.device) for st in states])
                table = self._upload(torch.tensor(slots, dtype=torch.int64))
                rec = p(keep)
            call("idv_stream_state_scatter", p(views), i(views.numel() // 4), i(self.B), L._P(table.data_ptr()), i(n), rec, ll(per),
                 stream_ptr())
        for b, st in zip(slots, states):
            self.sessions.set_slot_state(b, st.plan)
            self._state_set_extra(b, st)

    def _state_set_extra(self, b: int, st: "SlotState"):
        pass

    def _ended(self, slots: List[int]):
        """Hook: these slots' signals have ended or were dropped (their state is zeroed)."""

    def reset(self):
        """Zero every slot's state and bookkeeping."""
        super().reset()
        if hasattr(self, "sessions"):
            self.sessions.drop(range(self.B))
            self._ended(list(range(self.B)))

    def drop(self, slots):
        """Abandon the signals of these slots: nothing is returned for them and their state is zeroed; their next samples begin
        a new signal."""
        slots = check_slots(slots, self.B)
        if not slots:
            return
        self.sessions.drop(slots)
        self._ended(slots)
        with torch.cuda.device(self.device):
            table = self._upload(torch.tensor(slots, dtype=torch.int64))
            self._zero(L._P(table.data_ptr()), len(slots))

    def _upload(self, host: torch.Tensor) -> torch.Tensor:
        """One host-to-device copy of a call's tables through a pinned staging buffer."""
        n = host.numel()
        if self._table is None or self._table.numel() < n:
            size = max(1 << (n - 1).bit_length(), self._table_min)
            self._table = torch.empty(size, dtype=torch.int64, device=self.device)
            self._staging = [(torch.empty(size, dtype=torch.int64).pin_memory(), torch.cuda.Event()) for _ in range(2)]
        stage, ev = self._staging[self._turn]
        self._turn ^= 1
        ev.synchronize()            # the copy that read this buffer two calls ago; an event never recorded does not wait
        stage[:n].copy_(host)
        self._table[:n].copy_(stage[:n], non_blocking=True)
        ev.record()
        return self._table

    def _zero(self, slots_ptr, n: int):
        if n:
            for buf, outer, inner in self._zero_views:
                call("idv_stream_zero_rows", p(buf), ll(outer), i(self.B), ll(inner), slots_ptr, i(n), stream_ptr())

    # ------------------------------------------------------------------ push of a network's sessions
    def push(self, x: torch.Tensor, counts=None, end=()):
        check_input(x, self.B, self.device)
        n = int(x.shape[1])
        counts = check_counts(counts, self.B, n)
        end = check_slots(end, self.B)
        snap = self.sessions.snapshot()
        plan = self.sessions.push(counts, end)
        B, R, cap = self.B, self.plan.ring, self.plan.carry_cap
        ldy = max(plan.m)
        x, ldx, _ = self._pitched(x, B)
        ints, per = self._tables(plan)               # per: the ints of one launch group, its slots' table [B][NF] first
        host = torch.tensor(ints, dtype=torch.int64)
        for gi, g in enumerate(plan.groups):         # a bad table never reaches a kernel
            rc = L.lib().idv_stream_rows_check(L._P(host.data_ptr() + 8 * gi * per), B, R, 0 if g.flush else n, self.n_fft, self.win,
                                               self.hop, cap, g.k, g.k + 1, ldy, g.span)
            if rc != 0:
                self.sessions.restore(snap)
                raise L.IdvError(f"idv_stream_rows_check refused the table of launch group {gi} (status {rc})")
        with torch.cuda.device(self.device):
            s = stream_ptr()
            rows_y, frames, side = self._ola_site()
            y = torch.zeros(rows_y, ldy, dtype=torch.float32, device=self.device)
            if plan.groups or plan.zero:
                table = self._upload(host).data_ptr()
                zero = table + 8 * len(plan.groups) * per
                ring_due = any(counts)
                for gi, g in enumerate(plan.groups):
                    if g.flush and ring_due:         # the flush phase reads this call's samples from the ring
                        call("idv_stream_ring_rows", p(self.ring), i(R), p(x), ll(ldx), i(n), L._P(table), i(B), s)
                        ring_due = False
                    c = self._launch(g, table + 8 * gi * per, zero + 8 * len(plan.zero))
                    if g.k > 0:
                        self._network(c, (None, 0) if g.flush else (x if n else None, ldx))
                    Tp = g.k + 1
                    call("idv_stream_ola_rows", frames.ptr() if g.k > 0 else p(None), i(Tp), i(Planar.jp_for(rows_y, Tp)),
                         p(self.carry), i(cap), getattr(c, side), i(rows_y), i(self.n_fft), i(self.win), i(self.hop), i(g.k),
                         ll(g.span), p(y) if ldy else p(None), ll(ldy), s)
                if ring_due:
                    call("idv_stream_ring_rows", p(self.ring), i(R), p(x), ll(ldx), i(n), L._P(table), i(B), s)
                self._zero(L._P(zero), len(plan.zero))
                self._ended(plan.zero)
            return self._finish(y, ldy), plan.m

    def _tables(self, plan: SessionCall):
        """(the ints of the one copy a call makes, the ints per launch group): the groups' tables, then the slots to zero."""
        return [v for g in plan.groups for r in g.rows for v in r] + plan.zero, self.B * NF

    def _launch(self, g: Group, tables: int, behind: int):
        """What the network needs of launch group g, whose tables start at device address ``tables``; ``behind`` is the address
        behind the slots to zero."""
        return _Launch(g.k, L._P(tables))

    def _ola_site(self):
        """Where the overlap-add runs: (rows of y, the Planar of the inverse-DFT frames, the launch's table of those rows)."""
        return self.B, self.ifr, "rows"

    def _finish(self, y: torch.Tensor, ldy: int) -> torch.Tensor:
        return y

    def _frames(self, c, io, frames, Tp: int, Jp: int):
        x, ldx = io
        call("idv_stream_frames_rows", p(self.ring), i(self.plan.ring), p(x), ll(ldx), c.rows, i(self.B), i(self.n_fft), i(self.win),
             i(self.hop), i(c.k), frames, i(Tp), i(Jp), stream_ptr())


class StreamingSessions(_Slots, _Streamer):
    """Streaming inference of a causal ``DCCRN_`` for ``slots`` independent signals in one batch: every slot starts, receives
    samples and ends on its own.

        y, m = st.push(x, counts=None, end=())   # x: [slots, n] float32 on the model's GPU
        st.drop(slots)                           # abandon the signals of these slots: no output, state zeroed
        st.positions                             # samples received per slot for its current signal (host list)
        states = st.save(slots)                  # the streams of these slots as SlotState values; the slots go on untouched
        st.load(slots, states, overwrite=False)  # continue those streams in these slots (of this or another object)

    ``counts[b]`` (host ints, 0 .. n; None: n for all) says how many leading samples of row b are new for slot b; nothing at or
    past ``x[b, counts[b]]`` is read.  ``end`` names the slots whose signal ends after this call's samples ("push, then flush"):
    over its calls a signal of L samples returns ``hop * floor(L / hop)`` samples, the slot is zeroed on the device and its next
    samples begin a new signal.  Ending a slot that has received nothing is a no-op; ending one with 0 < L <= n_fft/2 raises
    ``ValueError``.  Every guard runs on the host before any GPU work and before any bookkeeping changes.

    ``y`` is ``[slots, max(m)]`` with ``m[b]`` valid samples in row b and zeros behind them; ``m`` comes from the host plan.
    A slot's samples are bit-identical to what ``StreamingDCCRN(model, batch=slots)`` returns for the same signal in the same
    slot, whatever the other slots do.  One table per launch group tells the kernels what each slot does (:class:`SessionPlan`);
    all tables of a call go to the device in one copy from a pinned staging buffer, whose reuse waits on the event of the copy
    that last read it (two buffers alternate, so that copy is two calls back).
    """

    _state_kind = "dccrn"

    def __init__(self, model, slots: int, frames_per_launch: int = 64, max_columns: int = 4096, conv: str = "valu"):
        super().__init__(model, slots, frames_per_launch, max_columns, conv)
        self._init_slots()
        # state buffers as [outer][slots][inner] for idv_stream_zero_rows
        self._zero_views = [(self.ring, 1, self.plan.ring), (self.carry, 2, self.plan.carry_cap), (self.lstm_state, 16, self.H)]
        self._zero_views += [(h, h.numel() // slots, 1) for h in [self.h_in, self.h_dense] + self.h_enc + self.h_dec]

    # ------------------------------------------------------------------ the per-row kernels of the network
    def _block(self, cp: _ConvPack, c, x0, h0, x1, h1, out, hist, x0hist, Tp: int, Jp: int):
        self._conv_call_rows(cp, x0, h0, x1, h1, out, hist, x0hist, self.B, c.k, Tp, Jp, c.rows)

    def _lstm(self, c, out, Tp: int, Jp: int):
        call("idv_stream_clstm_rows", p(self.G), p(self.lstm_wt), p(self.lstm_b1), p(self.lstm_state), p(self.hout), out, i(self.H),
             i(self.B), i(c.k), i(Tp), i(Jp), c.rows, stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------------
# The I-DCCRN-VAE pair: noisy encoder -> latent draw -> fine-tuned decoder with the noisy skips (pad='sig') -> mean over the
# num_samples waveforms (inference.enhance_vae offline).

LATENTS = ("speech", "noise")


def check_vae(noisy_encoder, decoder, batch, latent="speech", seed=0, eps=None) -> None:
    """The construction guards of StreamingVAE (host only, before any GPU work)."""
    from .model import pvae_module as pm
    if not isinstance(noisy_encoder, (pm.nsvae_pvae_dccrn_encoder_twophase, pm.pvae_dccrn_encoder_skip_prepare)):
        raise ValueError("StreamingVAE takes a model.pvae_module.nsvae_pvae_dccrn_encoder_twophase or pvae_dccrn_encoder_skip_prepare "
                         "as noisy_encoder")
    if isinstance(decoder, pm.pvae_dccrn_decoder_skip_prepare):
        raise ValueError("StreamingVAE: pvae_dccrn_decoder_skip_prepare decodes with pad='zero' (zero skips), which is not streamed; "
                         "pass the fine-tuned nsvae_pvae_dccrn_decoder_twophase (run with pad='sig')")
    if not isinstance(decoder, pm.nsvae_pvae_dccrn_decoder_twophase):
        raise ValueError("StreamingVAE takes a model.pvae_module.nsvae_pvae_dccrn_decoder_twophase as decoder")
    if not isinstance(latent, str) or latent not in LATENTS:
        raise ValueError(f"latent must be one of {LATENTS}, got {latent!r}")
    latent_num = getattr(noisy_encoder, "latent_num", 1)
    if latent == "noise" and latent_num != 2:
        raise ValueError("latent='noise' needs an encoder with latent_num 2: this encoder has no noise latent")
    _check_pair("StreamingVAE", noisy_encoder, decoder)
    _check_batch_seed("StreamingVAE", batch, seed)
    if eps is not None and not callable(eps):
        raise ValueError("eps must be None (the streamer's own draws) or a callable (t0, k) -> (eps_r, eps_i)")
    _check_lstm("StreamingVAE", noisy_encoder)
    _check_chain("StreamingVAE", noisy_encoder, decoder)
    _check_on_gpu("StreamingVAE", (noisy_encoder, decoder))


def _check_pair(name, noisy_encoder, decoder, what="decoder") -> None:
    """An encoder and one decoder agree: causal, n_fft / hop / win, zdim, num_samples, a known recon_type."""
    if not noisy_encoder.causal or not decoder.causal or any(e.conv._cfg[2][1] != 1 for e in noisy_encoder.encoders):
        raise ValueError(f"{name} needs a causal encoder and {what} (encoder time padding 1): with time padding 0 frame t needs "
                         "x[t+1]")
    se, sd = noisy_encoder.stft, decoder.istft
    if (se.n_fft, se.hop_length, se.win_length) != (sd.n_fft, sd.hop_length, sd.win_length):
        raise ValueError(f"{name}: encoder and {what} differ in n_fft / hop / win")
    if noisy_encoder.zdim != decoder.zdim or noisy_encoder.num_samples != decoder.num_samples:
        raise ValueError(f"{name}: encoder and {what} differ in zdim or num_samples")
    if decoder.recon_type not in ("mask", "real_imag"):
        raise ValueError(f"{name}: unknown recon_type {decoder.recon_type!r} (mask or real_imag)")


def _check_batch_seed(name, batch, seed) -> None:
    if isinstance(batch, bool) or not isinstance(batch, int) or batch <= 0:
        raise ValueError(f"{name}: batch must be a positive int")
    check_seed(seed)


def _check_lstm(name, noisy_encoder) -> None:
    latent_num = getattr(noisy_encoder, "latent_num", 1)
    lstms = noisy_encoder.lstms
    if (len(lstms) != 1 or lstms[0].num_layer != 2 or lstms[0].hidden_size != 3 * noisy_encoder.zdim * latent_num
            or L.lib().idv_stream_clstm_wide_supported(i(lstms[0].hidden_size)) != 1):
        raise ValueError(f"{name}: one two-layer ComplexLSTM with hidden size 3 * zdim * latent_num, a multiple of 16 up to 768, "
                         "is supported")


def _check_chain(name, noisy_encoder, decoder, what="decoder") -> None:
    """The decoder's channel chain against the encoder's skips (a zero skip takes the same channels of the weights)."""
    lstms = noisy_encoder.lstms
    enc_c = [e.conv.out_channel for e in noisy_encoder.encoders]
    if len(decoder.decoders) != len(enc_c) or lstms[0].input_size % enc_c[-1]:
        raise ValueError(f"{name}: the {what} does not mirror the encoder")
    top_f = lstms[0].input_size // enc_c[-1]
    if decoder.dense.in_channel != decoder.zdim or decoder.dense.out_channel % top_f:
        raise ValueError(f"{name}: the {what}'s dense layer does not match zdim and the top encoder shape")
    c = decoder.dense.out_channel // top_f
    for di, blk in enumerate(decoder.decoders):
        c1 = enc_c[len(enc_c) - 1 - di] if (decoder.use_sc and di in decoder.skip_to_use) else 0
        if c + c1 != blk.transconv.in_channel:
            raise ValueError(f"{name}: {what} block {di} takes {blk.transconv.in_channel} channels, the chain and the encoder's "
                             f"skip give {c} + {c1}")
        c = blk.transconv.out_channel
    if c != 1:
        raise ValueError(f"{name}: the last {what} must give one channel")


def _check_on_gpu(name, modules) -> None:
    for m in modules:
        if any(not q.is_cuda for q in m.parameters()) or any(not b.is_cuda for b in m.buffers()):
            raise RuntimeError(f"{name} runs on the MI355X only: move the models to the GPU first (there is no CPU path)")


ESTIMATES = ("clean_direct",) + tuple(OUTTYPES)       # outtype: the speech decoder alone, or a mask estimator of inference.py


def check_vae_two_latents(noisy_encoder, speech_decoder, noise_decoder, batch, outtype="phase_mask", phase=2, seed=0,
                          eps=None) -> None:
    """The construction guards of StreamingVAETwoLatents (host only, before any GPU work)."""
    from .model import pvae_module as pm
    name = "StreamingVAETwoLatents"
    if not isinstance(noisy_encoder, (pm.nsvae_pvae_dccrn_encoder_twophase, pm.pvae_dccrn_encoder_skip_prepare)):
        raise ValueError(f"{name} takes a model.pvae_module.nsvae_pvae_dccrn_encoder_twophase as noisy_encoder")
    if getattr(noisy_encoder, "latent_num", 1) != 2:
        raise ValueError(f"{name} needs an encoder with latent_num 2: this encoder has no noise latent")
    if not isinstance(outtype, str) or outtype not in ESTIMATES:
        raise ValueError(f"outtype must be one of {ESTIMATES}, got {outtype!r}")
    if isinstance(phase, bool) or phase not in (1, 2):
        raise ValueError(f"phase must be 1 (zero skips) or 2 (the noisy skips, pad='sig'), got {phase!r}")
    if outtype == "clean_direct":
        noise_decoder = None            # not run
    elif noise_decoder is None:
        raise ValueError(f"outtype {outtype!r} needs a noise_decoder: only 'clean_direct' runs the speech decoder alone")
    decs = [("speech_decoder", speech_decoder)] + ([("noise_decoder", noise_decoder)] if noise_decoder is not None else [])
    for what, dec in decs:
        if isinstance(dec, pm.pvae_dccrn_decoder_skip_prepare):
            if phase == 2:
                raise ValueError(f"{name}: phase=2 decodes with the noisy skips (pad='sig'), which the {what}, a "
                                 "pvae_dccrn_decoder_skip_prepare, does not take; pass phase=1 or the fine-tuned "
                                 "nsvae_pvae_dccrn_decoder_twophase")
            if dec.recon_type != "real_imag":
                raise ValueError(f"{name}: the {what}, a pvae_dccrn_decoder_skip_prepare, implements recon_type 'real_imag' only")
        elif not isinstance(dec, pm.nsvae_pvae_dccrn_decoder_twophase):
            raise ValueError(f"{name} takes a model.pvae_module.nsvae_pvae_dccrn_decoder_twophase or "
                             f"pvae_dccrn_decoder_skip_prepare as {what}")
        _check_pair(name, noisy_encoder, dec, what)
        if outtype != "clean_direct" and getattr(dec, "resynthesis", False):
            raise ValueError(f"{name}: the {what} has resynthesis=True: its predict is a re-analysis of the decoded waveform, which "
                             f"cannot be formed per column, so outtype {outtype!r} is not streamed with it")
    if noise_decoder is not None:
        a, b = speech_decoder, noise_decoder
        if a.recon_type != b.recon_type:
            raise ValueError(f"{name}: speech_decoder and noise_decoder differ in recon_type")
        skips = lambda d: sorted(set(d.skip_to_use)) if d.use_sc else []
        if skips(a) != skips(b):
            raise ValueError(f"{name}: speech_decoder and noise_decoder differ in their skip set (use_sc / skip_to_use)")
    _check_batch_seed(name, batch, seed)
    if eps is not None and not callable(eps):
        raise ValueError("eps must be None (the streamer's own draws) or a callable (t0, k) -> (eps_sr, eps_si, eps_nr, eps_ni)")
    _check_lstm(name, noisy_encoder)
    for what, dec in decs:
        _check_chain(name, noisy_encoder, dec, what)
    _check_on_gpu(name, [noisy_encoder] + [d for _, d in decs])


def check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise ValueError("seed must be an int in [0, 2**63)")
    return seed


class _DecChain:
    """One decoder of a VAE streamer: the packs of its dense layer and blocks (``dense``, ``dec``), the rows of the LSTM output
    its latent takes (``lat_off``), whether its blocks read the repeated noisy skips (``skips``; else they are packed as zero
    skips), and what it owns on the device: the histories ``h_dense`` / ``h_dec`` and the raw last-block output ``raw``."""
    __slots__ = ("dec", "dense", "lat_off", "skips", "h_dense", "h_dec", "raw")


class _VAEStreamer(_StreamBase):
    """What both VAE streamers share: the construction guards, the packed weights of the pair, the activation and state buffers
    (encoder side at batch B, decoder side at batch B * ns, row b * ns + s), the draws of ``eps`` and the network over the frames
    of one launch group.  A subclass supplies the framing, the conv block, the LSTM, the draws and the repeated skips of its kind
    (scalars for lock-step streams, row tables for sessions)."""

    _name = "StreamingVAE"
    _skip_halves = 1               # parity halves of the repeated skip histories (h_skip_n)

    def __init__(self, noisy_encoder, decoder, batch: int, seed: int = 0, latent: str = "speech", average: bool = True, eps=None,
                 frames_per_launch: int = 64, max_columns: int = 4096, conv: str = "valu"):
        self.conv = check_conv(conv)
        check_vae(noisy_encoder, decoder, batch, latent, seed, eps)
        for blk in list(noisy_encoder.encoders) + list(decoder.decoders):
            (blk.conv if hasattr(blk, "conv") else blk.transconv)._check_supported()
        self.encoder, self.decoder, self.B = noisy_encoder, decoder, batch
        self.ns = noisy_encoder.num_samples
        self.Bn = batch * self.ns
        self.zdim = noisy_encoder.zdim
        self.latent, self.average, self._eps_fn = latent, bool(average), eps
        self._seed = seed
        self.device = next(noisy_encoder.parameters()).device
        st = noisy_encoder.stft
        self.n_fft, self.hop, self.win = st.n_fft, st.hop_length, st.win_length
        self.F = self.n_fft // 2 + 1
        self.cap = max(1, min(frames_per_launch, max_columns // self.Bn))
        self.plan = StreamPlan(self.n_fft, self.hop, self.win, self.cap)
        self.skip_to_use = list(decoder.skip_to_use) if decoder.use_sc else []
        self.recon = decoder.recon_type
        with torch.no_grad(), torch.cuda.device(self.device):
            self._pack()
            self._alloc()
        self.reset()

    @property
    def seed(self) -> int:
        return self._seed

    @seed.setter
    def seed(self, v):
        self._seed = check_seed(v)

    # ------------------------------------------------------------------ construction
    def _pack(self):
        self._pack_encoder()
        self.chain = self._pack_chain(self.decoder, LATENTS.index(self.latent), False)
        self.dec, self.dense, self.lat_off = self.chain.dec, self.chain.dense, self.chain.lat_off
        self.conv_engines = [cp.engine for cp in self.enc + self.dec]      # enc0 .. then dec0 ..

    def _pack_encoder(self):
        enc = self.encoder
        self.enc, self.enc_shapes = [], []
        ch, Fin = 1, self.F
        for blk in enc.encoders:
            cp = self._conv(blk.conv, blk, ch, 0, Fin, self.B)
            self.enc.append(cp)
            ch, Fin = cp.Cout, cp.Fout
            self.enc_shapes.append((ch, Fin))
        if ch * Fin != enc.lstms[0].input_size:
            raise ValueError(f"{self._name}: the LSTM input does not match the top encoder shape")
        self._pack_lstm(enc.lstms[0], ch * Fin)
        dft = ops.DftPlan(self.n_fft, self.win, self.hop, 1, self.device)
        self.dft_fwd, self.dft_inv = dft.fwd, dft.inv

    def _pack_chain(self, dec, latent: int, zero_skip: bool) -> "_DecChain":
        """The packs of one decoder on latent number ``latent``: dense and blocks, with the noisy skips of ``self.skip_to_use``
        or, ``zero_skip``, with zero skips (packed away, see ``_conv``)."""
        ch = _DecChain()
        Fin = self.enc_shapes[-1][1]
        dch = dec.dense.out_channel // Fin
        if getattr(self, "dense_out", (dch, Fin)) != (dch, Fin):
            raise ValueError(f"{self._name}: the decoders' dense layers differ in shape")
        self.dense_out = (dch, Fin)
        ch.dec = []
        n = len(self.enc)
        c, f = dch, Fin
        for di, blk in enumerate(dec.decoders):
            c1 = self.enc_shapes[n - 1 - di][0] if di in self.skip_to_use else 0
            if c1 and self.enc_shapes[n - 1 - di][1] != f:
                raise ValueError(f"{self._name}: a skip's bins do not match the decoder block")
            cp = self._conv(blk.transconv, blk, c, 0 if zero_skip else c1, f, self.Bn, zero_skip=bool(zero_skip and c1))
            ch.dec.append(cp)
            c, f = cp.Cout, cp.Fout
        if (c, f) != (1, self.F):
            raise ValueError(f"{self._name}: the last decoder must give one channel of n_fft/2 + 1 bins")
        dn = dec.dense
        ch.dense = [ops.pack_pw(dn.linear_read.weight.detach().float(), dn.linear_read.bias.detach().float()),
                    ops.pack_pw(dn.linear_imag.weight.detach().float(), dn.linear_imag.bias.detach().float())]
        o = 3 * self.zdim * latent
        ch.lat_off = (o, o + self.zdim, o + 2 * self.zdim)
        ch.skips = not zero_skip
        return ch

    def _alloc(self):
        self._alloc_encoder()
        self._alloc_decoder([self.chain], self.Bn)
        self.dec_out.append(self.chain.raw)
        self.h_dense, self.h_dec = self.chain.h_dense, self.chain.h_dec
        self.state = [self.h_in, self.h_dense, self.lstm_state, self.ring, self.carry] + self.h_enc + self.h_dec

    def _alloc_encoder(self):
        """The encoder side, batch B: activations, LSTM scratch and the per-stream state of the encoder and the input ring."""
        B, dev, cap = self.B, self.device, self.cap
        Tp = cap + 1
        mk = lambda C, F, b: Planar.empty(C, F, b, cap, Tp, dev, zero=True)
        self.fr = mk(1, self.win // 2, B)
        self.X = mk(1, self.F, B)
        self.enc_out = [mk(c, f, B) for c, f in self.enc_shapes]
        self.lat = mk(self.H, 1, B)
        self.G = torch.empty(2 * B * cap * 8 * self.H, dtype=torch.float32, device=dev)
        self.hstep = torch.empty(int(L.lib().idv_stream_clstm_wide_hstep_floats(i(self.H), i(B), i(cap))), dtype=torch.float32, device=dev)
        hist = lambda C, F, b: torch.zeros(2, 2 * C * F * b, dtype=torch.float32, device=dev)
        self.h_in = hist(1, self.F, B)
        self.h_enc = [hist(c, f, B) for c, f in self.enc_shapes]
        self.lstm_state = torch.zeros(4 * 4 * B * self.H, dtype=torch.float32, device=dev)
        self.ring = torch.zeros(B * self.plan.ring, dtype=torch.float32, device=dev)

    def _alloc_decoder(self, chains, carry_rows: int):
        """The decoder side, batch Bn = B * ns, row b * ns + s: the activation scratch the chains share (``z``, ``dense_buf``,
        ``dec_out`` of every block but the last, the repeated skips), each chain's own state (``h_dense``, ``h_dec``) and raw
        last-block output, and the overlap-add carry of ``carry_rows`` rows."""
        B, Bn, dev, cap = self.B, self.Bn, self.device, self.cap
        Tp = cap + 1
        mk = lambda C, F, b: Planar.empty(C, F, b, cap, Tp, dev, zero=True)
        hist = lambda C, F, b: torch.zeros(2, 2 * C * F * b, dtype=torch.float32, device=dev)
        self.z = mk(self.zdim, 1, Bn)
        self.dense_buf = mk(*self.dense_out, Bn)
        n = len(self.enc)
        skips = self.skip_to_use if any(ch.skips for ch in chains) else []
        self.skip_n = {di: mk(*self.enc_shapes[n - 1 - di], Bn) for di in skips if di < n}
        # scratch, not state: the history half a chunk reads, repeated (sessions: one half per parity, slot b's in half parity_b)
        self.h_skip_n = {di: torch.zeros(self._skip_halves * 2 * self.enc_shapes[n - 1 - di][0] * self.enc_shapes[n - 1 - di][1] * Bn,
                                         dtype=torch.float32, device=dev) for di in self.skip_n}
        first = chains[0].dec
        self.dec_out = [mk(cp.Cout, cp.Fout, Bn) for cp in first[:-1]]
        for ch in chains:
            if [(cp.Cout, cp.Fout) for cp in ch.dec] != [(cp.Cout, cp.Fout) for cp in first]:
                raise ValueError(f"{self._name}: the decoders differ in their block shapes")
            ch.raw = mk(first[-1].Cout, first[-1].Fout, Bn)
            ch.h_dense = hist(*self.dense_out, Bn)
            ch.h_dec = [hist(cp.Cout, cp.Fout, Bn) for cp in ch.dec[:-1]]
        self.eps_buf = torch.empty(2 * len(chains), Bn * cap * self.zdim, dtype=torch.float32, device=dev)
        self.pred = mk(1, self.F, Bn)
        self.ifr = mk(1, self.win // 2, Bn)
        work = max([cp.nsplit * 2 * cp.Cout * cp.Fout * B * cap for cp in self.enc if cp.nsplit > 1] +
                   [cp.nsplit * 2 * cp.Cout * cp.Fout * Bn * cap for ch in chains for cp in ch.dec if cp.nsplit > 1] + [0])
        self.work = torch.empty(max(work, 1), dtype=torch.float32, device=dev)
        self.carry = torch.zeros(2, carry_rows * self.plan.carry_cap, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ the draws
    def eps(self, t0: int, k: int):
        """The draws frames t0 .. t0+k-1 use with the streamer's own generator and its current seed: (eps_r, eps_i), each
        [B, ns, k, zdim]."""
        if isinstance(t0, bool) or not isinstance(t0, int) or t0 < 0 or isinstance(k, bool) or not isinstance(k, int) or k <= 0:
            raise ValueError("eps(t0, k): t0 >= 0 and k > 0 frames")
        out = torch.empty(2, self.B, self.ns, k, self.zdim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            call("idv_stream_eps", ll(self._seed), ll(t0), i(k), i(self.B), i(self.ns), i(self.zdim), p(out[0]), p(out[1]), stream_ptr())
        return out[0], out[1]

    # ------------------------------------------------------------------ the network over one launch group
    @staticmethod
    def _at(pl, Jp: int, plane: int = 0):
        """Device pointer of plane ``plane`` of a Planar used at row pitch ``Jp``."""
        return L._P(pl.buf.data_ptr() + 4 * (ops.SLACK + plane * pl.F * Jp))

    def _network(self, c, io):
        """Frames -> spectrum -> encoders -> wide LSTM (batch B) -> draws -> reparameterisation -> dense -> decoders with the
        repeated skips -> mask -> windowed inverse-DFT frames (self.ifr), batch B * ns, for the c.k columns per stream of launch
        group c; ``io`` is what the subclass's framing needs."""
        self._encode(c, io)
        self._decode(c, self.chain, self._draws(c), self._skips(c))
        self._tail(c, self.chain)

    def _encode(self, c, io):
        """Frames -> spectrum (self.X) -> encoders (self.enc_out) -> wide LSTM (self.lat), batch B."""
        B, k = self.B, c.k
        Tp = k + 1
        Jp = Planar.jp_for(B, Tp)
        ptr = lambda pl, plane=0: self._at(pl, Jp, plane)
        self._frames(c, io, ptr(self.fr), Tp, Jp)
        ops.pw_gemm(ptr(self.fr), self.win, self.dft_fwd[0], self.dft_fwd[1], 2 * self.F, B, Tp, Jp, k, ptr(self.X))
        src, hsrc = self.X, self.h_in
        for e, cp in enumerate(self.enc):
            out = self.enc_out[e]
            self._block(cp, c, ptr(src), hsrc, None, None, ptr(out), self.h_enc[e], self.h_in if e == 0 else None, Tp, Jp, False)
            src, hsrc = out, self.h_enc[e]
        # LSTM: layer-0 projection of both input parts (idv_pw_gemm as offline), then one launch per layer per step
        H, K = self.H, self.K
        wih, bih = self.lstm_ih
        top = self.enc_out[-1]
        for z in range(2):
            ops.pw_gemm(ptr(top, z * top.C), K, wih, bih, 8 * H, B, Tp, Jp, k,
                        L._P(self.G.data_ptr() + 4 * z * k * B * 8 * H), swap=True, ldo=8 * H)
        self._lstm(c, ptr(self.lat), Tp, Jp)

    def _skips(self, c):
        """The skips and the history half this group reads, repeated to batch B * ns, once for every chain that reads them:
        block number -> (x1, h1) of its ``_block`` call."""
        B, Bn, k = self.B, self.Bn, c.k
        Tp = k + 1
        Jp, Jpn = Planar.jp_for(B, Tp), Planar.jp_for(Bn, Tp)
        n = len(self.enc)
        out = {}
        for di in self.skip_n:
            sk = n - 1 - di
            xn = self._at(self.skip_n[di], Jpn)
            out[di] = (xn, self._repeat(c, di, sk, self._at(self.enc_out[sk], Jp), xn, Tp, Jp, Jpn))
        return out

    def _decode(self, c, ch: "_DecChain", draws, skips):
        """One decoder chain at batch B * ns: reparameterisation of the chain's latent with ``draws`` (eps_r, eps_i) -> dense ->
        decoder blocks (``skips`` from ``_skips``; none for a zero-skip chain) -> the raw last-block output ``ch.raw``."""
        B, Bn, ns, k = self.B, self.Bn, self.ns, c.k
        Tp = k + 1
        Jp, Jpn = Planar.jp_for(B, Tp), Planar.jp_for(Bn, Tp)
        s = stream_ptr()
        ptrn = lambda pl, plane=0: self._at(pl, Jpn, plane)
        er, ei = draws
        zd = self.zdim
        call("idv_reparam", self._at(self.lat, Jp), i(self.H), i(ch.lat_off[0]), i(ch.lat_off[1]), i(ch.lat_off[2]), i(zd), er, ei,
             i(ns), i(B), i(k), i(Tp), i(Jp), ptrn(self.z), i(Jpn), s)
        dc, df = self.dense_out
        for ri, pk in enumerate(ch.dense):
            ops.pw_gemm(ptrn(self.z, ri * zd), zd, pk[0], pk[1], dc * df, Bn, Tp, Jpn, k, ptrn(self.dense_buf, ri * dc))
        src, hsrc = self.dense_buf, ch.h_dense
        last = len(ch.dec) - 1
        for di, cp in enumerate(ch.dec):
            out = ch.raw if di == last else self.dec_out[di]
            x1, h1 = skips[di] if (ch.skips and di in skips) else (None, None)
            hout = ch.h_dec[di] if di < last else None                   # nothing reads the last block's history
            self._block(cp, c, ptrn(src), hsrc, x1, h1, ptrn(out), hout, ch.h_dense if di == 0 else None, Tp, Jpn, True)
            if di < last:
                src, hsrc = out, ch.h_dec[di]

    def _tail(self, c, ch: "_DecChain"):
        """``ch.raw`` -> mask -> windowed inverse-DFT frames (self.ifr), batch B * ns."""
        B, Bn, k = self.B, self.Bn, c.k
        Tp = k + 1
        Jp, Jpn = Planar.jp_for(B, Tp), Planar.jp_for(Bn, Tp)
        ptrn = lambda pl, plane=0: self._at(pl, Jpn, plane)
        pred = ch.raw
        if self.recon == "mask":
            call("idv_mask_apply", ptrn(pred), self._at(self.X, Jp), i(self.ns), i(Jp), ptrn(self.pred), p(None), i(self.F), i(Bn), i(k),
                 i(Tp), i(Jpn), stream_ptr())
            pred = self.pred
        ops.pw_gemm(ptrn(pred), 2 * self.F, self.dft_inv[0], self.dft_inv[1], self.win, Bn, Tp, Jpn, k, ptrn(self.ifr))


class StreamingVAE(_VAEStreamer):
    """Lock-step streaming I-DCCRN-VAE enhancement for ``batch`` signals: the noisy encoder at batch B, one latent draw per
    sample, the fine-tuned decoder with the noisy skips (``pad='sig'``) at batch B * num_samples (row b * ns + s).

        st = StreamingVAE(noisy_encoder, decoder, batch=B, seed=0, latent="speech", average=True, eps=None)
        y = st.push(x)          # x [B, n] on the GPU -> [B, m] (average=False: [B * ns, m], row b * ns + s)
        y = st.flush()
        er, ei = st.eps(t0, k)  # the draws frames t0 .. t0+k-1 use, each [B, ns, k, zdim]

    Frame and sample bookkeeping is :class:`StreamPlan`, as in :class:`StreamingDCCRN`.  All pushes and the flush together
    return what ``inference.enhance_vae(noisy_encoder, decoder, x_full, eps=<the same draws>, latent=latent)`` returns, and the
    same bits however the signal is cut.  The draws come from a counter-based generator (``idv_stream_eps``): a draw is a
    function of (seed, b, s, t, u) alone, the same seed gives the same draws for every signal, and ``seed`` may be set between
    signals.  ``eps`` may instead be a callable ``(t0, k) -> (eps_r, eps_i)`` ([B, ns, k, zdim] each, on the GPU) that supplies
    the chosen latent's draws.  ``conv`` as in :class:`StreamingDCCRN` (``"bf16x3"`` included: the conv blocks of encoder and
    decoder, nothing else).  ``ops.PRECISION`` is never read; weights are packed at construction.
    """

    def reset(self):
        """Zero every per-stream state buffer and the bookkeeping (done by construction and by flush); the seed stays."""
        super().reset()
        self.plan.reset()

    # ------------------------------------------------------------------ the draws
    def _draws(self, c: Chunk):
        """Device pointers of eps_r / eps_i [B][ns][c.k][zdim] of chunk c."""
        if self._eps_fn is None:
            call("idv_stream_eps", ll(self._seed), ll(c.t0), i(c.k), i(self.B), i(self.ns), i(self.zdim), p(self.eps_buf[0]),
                 p(self.eps_buf[1]), stream_ptr())
            return p(self.eps_buf[0]), p(self.eps_buf[1])
        pair = self._eps_fn(c.t0, c.k)
        want = (self.B, self.ns, c.k, self.zdim)
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("eps(t0, k) must return (eps_r, eps_i)")
        out = []
        for t in pair:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
                raise ValueError(f"eps(t0, k) must return two tensors of shape {want}")
            if t.device != self.device:
                raise RuntimeError("eps(t0, k) must return tensors on the streamer's GPU")
            out.append(p(t.float().contiguous()))
        return tuple(out)

    # ------------------------------------------------------------------ push / flush
    def push(self, x: torch.Tensor) -> torch.Tensor:
        check_input(x, self.B, self.device)
        x, ldx, n_new = self._pitched(x, self.B)
        n_prev = self.plan.n
        with torch.no_grad(), torch.cuda.device(self.device):
            chunks = self.plan.push(n_new)
            y = self._run(chunks, x, ldx, n_new, n_prev, None)
            self._lock_ring(x, ldx, n_new, n_prev)
        return y

    def flush(self) -> torch.Tensor:
        L_total = self.plan.n
        self.plan.check_flush(L_total)
        with torch.no_grad(), torch.cuda.device(self.device):
            chunks = self.plan.flush()
            y = self._run(chunks, None, 0, 0, L_total, L_total)
            self.reset()
        return y

    def _run(self, chunks: List[Chunk], x, ldx: int, n_new: int, n_prev: int, L_end: Optional[int]) -> torch.Tensor:
        m = (chunks[-1].e1 - chunks[0].e0) if chunks else 0
        y = torch.empty(self.Bn, m, dtype=torch.float32, device=self.device)
        T_total = self.plan.total_frames(L_end) if L_end is not None else -1
        for c in chunks:
            if c.k > 0:
                self._network(c, (x, ldx, n_new, n_prev, L_end))
            self._lock_ola(c, self.ifr if c.k > 0 else None, self.carry, self.Bn, T_total, y, m, c.e0 - chunks[0].e0)
        if not self.average:
            return y
        out = torch.empty(self.B, m, dtype=torch.float32, device=self.device)
        if m:
            call("idv_mean_over_samples", p(y), i(self.ns), i(self.B), i(m), p(out), stream_ptr())
        return out

    # ------------------------------------------------------------------ the lock-step kernels of the network
    def _frames(self, c: Chunk, io, frames, Tp: int, Jp: int):
        self._lock_frames(c, io, frames, Tp, Jp)

    def _block(self, cp: _ConvPack, c: Chunk, x0, h0, x1, h1, out, hist, x0hist, Tp: int, Jp: int, dec: bool):
        """One conv block of the encoder (batch B) or the decoder (batch B * ns): histories are read from half c.parity of the
        [2][...] buffers and written to the other half; h1 is what ``_repeat`` returned."""
        P = c.parity
        self._conv_call(cp, x0, h0[P], x1, h1, out, hist[1 - P] if hist is not None else None,
                        p(x0hist[1 - P]) if x0hist is not None else p(None), self.Bn if dec else self.B, c.k, Tp, Jp)

    def _lstm(self, c: Chunk, out, Tp: int, Jp: int):
        call("idv_stream_clstm_wide", p(self.G), p(self.lstm_wt), p(self.lstm_b1), p(self.lstm_state), p(self.hstep), out,
             i(self.H), i(self.B), i(c.k), i(Tp), i(Jp), stream_ptr())

    def _repeat(self, c: Chunk, di: int, sk: int, x, xn, Tp: int, Jp: int, Jpn: int):
        sc, sf = self.enc_shapes[sk]
        call("idv_stream_repeat", x, p(self.h_enc[sk][c.parity]), i(sc), i(sf), i(self.B), i(self.ns), i(c.k), i(Tp), i(Jp), xn,
             p(self.h_skip_n[di]), i(Jpn), stream_ptr())
        return self.h_skip_n[di]


class _TwoLatents:
    """What both two-latent streamers share, mixed in in front of their single-decoder base: the construction (guards, the two
    decoder chains on their latents), the buffers, and the network over one launch group.  The base supplies the framing, the
    conv block, the LSTM, the repeated skips and the draws of its kind; ``self._draws(c)`` returns the pointers of the speech
    pair followed, when the noise decoder runs, by those of the noise pair."""

    _name = "StreamingVAETwoLatents"

    def _init_two_latents(self, noisy_encoder, speech_decoder, noise_decoder, batch, outtype, phase, seed, eps, frames_per_launch,
                          max_columns, conv):
        self.conv = check_conv(conv)
        check_vae_two_latents(noisy_encoder, speech_decoder, noise_decoder, batch, outtype, phase, seed, eps)
        if outtype == "clean_direct":
            noise_decoder = None
        decoders = [speech_decoder] + ([noise_decoder] if noise_decoder is not None else [])
        for blk in list(noisy_encoder.encoders) + [b for d in decoders for b in d.decoders]:
            (blk.conv if hasattr(blk, "conv") else blk.transconv)._check_supported()
        self.encoder, self.decoder, self.noise_decoder, self.B = noisy_encoder, speech_decoder, noise_decoder, batch
        self.outtype, self.phase = outtype, phase
        self.ns = noisy_encoder.num_samples
        self.Bn = batch * self.ns
        self.zdim = noisy_encoder.zdim
        self.latent, self.average, self._eps_fn = "speech", True, eps
        self._seed = seed
        self.device = next(noisy_encoder.parameters()).device
        st = noisy_encoder.stft
        self.n_fft, self.hop, self.win = st.n_fft, st.hop_length, st.win_length
        self.F = self.n_fft // 2 + 1
        self.cap = max(1, min(frames_per_launch, max_columns // self.Bn))
        self.plan = StreamPlan(self.n_fft, self.hop, self.win, self.cap)
        self.skip_to_use = list(speech_decoder.skip_to_use) if speech_decoder.use_sc else []
        self.recon = speech_decoder.recon_type
        with torch.no_grad(), torch.cuda.device(self.device):
            self._pack()
            self._alloc()
        self.reset()

    # ------------------------------------------------------------------ construction
    def _pack(self):
        self._pack_encoder()
        zero = self.phase == 1
        self.chain = self.speech = self._pack_chain(self.decoder, 0, zero)
        self.noise = self._pack_chain(self.noise_decoder, 1, zero) if self.noise_decoder is not None else None
        self.chains = [self.speech] + ([self.noise] if self.noise is not None else [])
        self.conv_engines = [cp.engine for cp in self.enc] + [cp.engine for ch in self.chains for cp in ch.dec]

    def _alloc(self):
        B, dev, cap = self.B, self.device, self.cap
        self._alloc_encoder()
        # clean_direct keeps StreamingVAE's tail: one overlap-add row per sample; the estimators leave one row per stream
        self._alloc_decoder(self.chains, self.Bn if self.noise is None else B)
        if self.noise is not None:
            self.spec = Planar.empty(1, self.F, B, cap, cap + 1, dev, zero=True)
            self.ifr_b = Planar.empty(1, self.win // 2, B, cap, cap + 1, dev, zero=True)
        self.state = [self.h_in, self.lstm_state, self.ring, self.carry] + self.h_enc
        for ch in self.chains:
            self.state += [ch.h_dense] + ch.h_dec

    # ------------------------------------------------------------------ the network over one launch group
    def _network(self, c, io):
        """Encoder and LSTM once; both decoder chains on their latents; then either StreamingVAE's tail on the speech chain
        (clean_direct: self.ifr, batch B * ns) or the estimator and the inverse DFT at batch B (self.ifr_b)."""
        self._encode(c, io)
        d = self._draws(c)
        skips = self._skips(c)
        self._decode(c, self.speech, d[:2], skips)
        if self.noise is None:
            self._tail(c, self.speech)
            return
        self._decode(c, self.noise, d[2:], skips)
        B, k = self.B, c.k
        Tp = k + 1
        Jp, Jpn = Planar.jp_for(B, Tp), Planar.jp_for(self.Bn, Tp)
        call("idv_stream_estimate", self._at(self.speech.raw, Jpn), self._at(self.noise.raw, Jpn), self._at(self.X, Jp),
             i(1 if self.recon == "mask" else 0), i(OUTTYPES[self.outtype]), i(self.ns), i(self.F), i(B), i(k), i(Tp), i(Jp), i(Jpn),
             self._at(self.spec, Jp), stream_ptr())
        ops.pw_gemm(self._at(self.spec, Jp), 2 * self.F, self.dft_inv[0], self.dft_inv[1], self.win, B, Tp, Jp, k, self._at(self.ifr_b, Jp))


class StreamingVAETwoLatents(_TwoLatents, StreamingVAE):
    """Lock-step streaming of the two-latent evaluation (``inference.enhance_vae_two_latents``, the reference's
    ``latent_to_use == 2``) for ``batch`` signals: one pass of the noisy encoder at batch B, the speech decoder on the speech
    latent and the noise decoder on the noise latent at batch B * num_samples (row b * ns + s), then the ``outtype`` estimator.

        st = StreamingVAETwoLatents(noisy_encoder, speech_decoder, noise_decoder, batch=B, outtype="phase_mask", phase=2, seed=0)
        y = st.push(x)                   # x [B, n] on the GPU -> [B, m], the samples that became final
        y = st.flush()
        sr, si, nr, ni = st.eps(t0, k)   # the draws frames t0 .. t0+k-1 use, each [B, ns, k, zdim]

    :class:`StreamingVAE`'s contract: :class:`StreamPlan` bookkeeping, the same sample counts per ``push`` / ``flush`` and the
    same bits however the signal is cut; all pushes and the flush together return what ``inference.enhance_vae_two_latents(
    noisy_encoder, speech_decoder, noise_decoder, x_full, outtype, phase, eps=<the same four draws>)`` returns.

    ``phase=2``: both decoders are ``nsvae_pvae_dccrn_decoder_twophase`` and read the noisy skips (``pad='sig'``); the repeated
    skips and their history halves are formed once per launch group for both.  ``phase=1``: zero skips, as ``pad='zero'``
    offline, with either decoder class; a zero skip is packed away (the block keeps the first C0 input channels of its
    weights), so no zeros are read.  ``outtype="clean_direct"`` runs the speech decoder alone (``noise_decoder`` may be None)
    and, at ``phase=2``, returns the bits of ``StreamingVAE(noisy_encoder, speech_decoder, batch=B, seed=seed)``.  The mask
    estimators (``real_imag_mask``, ``complex_mask``, ``phase_mask``) form the two sample means and the estimate per column
    (``idv_stream_estimate``) in front of the inverse DFT, which with the overlap-add then runs at batch B.

    The draws of both latents come from one counter-based block per (seed, b, s, t, u) (``idv_stream_eps_pair``; the speech
    pair is ``StreamingVAE``'s); ``eps`` may instead be a callable ``(t0, k) -> (eps_sr, eps_si, eps_nr, eps_ni)``, each
    [B, ns, k, zdim] on the GPU.  ``conv`` as in :class:`StreamingDCCRN`; ``conv_engines`` lists enc0 .. 5, speech dec0 .. 5,
    then noise dec0 .. 5.  Exact fp32; weights are packed at construction.
    """

    def __init__(self, noisy_encoder, speech_decoder, noise_decoder, batch: int, outtype: str = "phase_mask", phase: int = 2,
                 seed: int = 0, eps=None, frames_per_launch: int = 64, max_columns: int = 4096, conv: str = "valu"):
        self._init_two_latents(noisy_encoder, speech_decoder, noise_decoder, batch, outtype, phase, seed, eps, frames_per_launch,
                               max_columns, conv)

    # ------------------------------------------------------------------ the draws
    def eps(self, t0: int, k: int):
        """The draws frames t0 .. t0+k-1 use with the streamer's own generator and its current seed: (eps_sr, eps_si, eps_nr,
        eps_ni), each [B, ns, k, zdim]; the first two are ``StreamingVAE.eps``'s."""
        if isinstance(t0, bool) or not isinstance(t0, int) or t0 < 0 or isinstance(k, bool) or not isinstance(k, int) or k <= 0:
            raise ValueError("eps(t0, k): t0 >= 0 and k > 0 frames")
        out = torch.empty(4, self.B, self.ns, k, self.zdim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            call("idv_stream_eps_pair", ll(self._seed), ll(t0), i(k), i(self.B), i(self.ns), i(self.zdim), p(out[0]), p(out[1]),
                 p(out[2]), p(out[3]), stream_ptr())
        return out[0], out[1], out[2], out[3]

    def _draws(self, c: Chunk):
        """Device pointers of eps_sr / eps_si / eps_nr / eps_ni [B][ns][c.k][zdim] of chunk c."""
        if self._eps_fn is None:
            if self.noise is None:
                return super()._draws(c) + (p(None), p(None))
            e = self.eps_buf
            call("idv_stream_eps_pair", ll(self._seed), ll(c.t0), i(c.k), i(self.B), i(self.ns), i(self.zdim), p(e[0]), p(e[1]), p(e[2]),
                 p(e[3]), stream_ptr())
            return p(e[0]), p(e[1]), p(e[2]), p(e[3])
        four = self._eps_fn(c.t0, c.k)
        want = (self.B, self.ns, c.k, self.zdim)
        if not isinstance(four, (tuple, list)) or len(four) != 4:
            raise ValueError("eps(t0, k) must return (eps_sr, eps_si, eps_nr, eps_ni)")
        out = []
        for t in four:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
                raise ValueError(f"eps(t0, k) must return four tensors of shape {want}")
            if t.device != self.device:
                raise RuntimeError("eps(t0, k) must return tensors on the streamer's GPU")
            out.append(p(t.float().contiguous()))
        return tuple(out)

    def _run(self, chunks: List[Chunk], x, ldx: int, n_new: int, n_prev: int, L_end: Optional[int]) -> torch.Tensor:
        if self.noise is None:
            return super()._run(chunks, x, ldx, n_new, n_prev, L_end)
        m = (chunks[-1].e1 - chunks[0].e0) if chunks else 0
        y = torch.empty(self.B, m, dtype=torch.float32, device=self.device)
        T_total = self.plan.total_frames(L_end) if L_end is not None else -1
        for c in chunks:
            if c.k > 0:
                self._network(c, (x, ldx, n_new, n_prev, L_end))
            self._lock_ola(c, self.ifr_b if c.k > 0 else None, self.carry, self.B, T_total, y, m, c.e0 - chunks[0].e0)
        return y


def decoder_rows(rows: List[List[int]], ns: int) -> List[List[int]]:
    """The decoder-side table of a launch group of VAE sessions: [B * ns][NF] with row b * ns + s equal to slot b's row."""
    return [r for r in rows for _ in range(ns)]


def vae_session_tables(plan: SessionCall, ns: int, seeds: Sequence[int] = (), draw_slots: Sequence[int] = ()) -> List[int]:
    """The host side of the one copy a VAE sessions call makes: per launch group the slots' table [B][NF] followed by its
    decoder-side table [B * ns][NF], then the slots to zero, then ``seeds`` (one per slot, as they stand when the call is made),
    then ``draw_slots`` (one per slot; empty while every slot draws as itself)."""
    return ([v for g in plan.groups for r in g.rows + decoder_rows(g.rows, ns) for v in r] + list(plan.zero) + list(seeds) +
            list(draw_slots))


class _VAELaunch(NamedTuple):
    """What the network needs of a VAE sessions launch group: k_launch and the device pointers of its two row tables (encoder
    side [B][NF], decoder side [B * ns][NF]) and of the slots' seeds [B]."""
    k: int
    rows: object
    rows_n: object
    seeds: object
    draws: object = None        # the slots' draw slots [B], or None while every slot draws as itself


class StreamingVAESessions(_Slots, _VAEStreamer):
    """Streaming I-DCCRN-VAE enhancement for ``slots`` independent signals in one batch: :class:`StreamingVAE`'s network with the
    ``push`` / ``counts`` / ``end`` / ``drop`` / ``positions`` contract of :class:`StreamingSessions`.

        st = StreamingVAESessions(noisy_encoder, decoder, slots, seed=0, latent="speech", average=True)
        y, m = st.push(x, counts=None, end=())   # x [slots, n] -> y [slots, max(m)] (average=False: [slots * ns, max(m)], row b * ns + s)
        st.drop(slots); st.positions; st.reset()
        st.seed; st.seeds; st.set_seed(slots, seed)
        er, ei = st.eps(t0, k)                   # [slots, ns, k, zdim] each, the generator of StreamingVAE.eps, every slot's own seed
        st.save(slots); st.load(slots, states); st.draw_slots

    Slot b's samples are bit-identical to what ``StreamingVAE(noisy_encoder, decoder, batch=slots, seed=st.seeds[b],
    latent=latent, conv=conv)`` returns for the same signal in slot b, whatever the other slots do and for every signal the slot
    serves one after another: a draw depends on (the slot's seed, b, s, the slot's own frame index, u).  ``seed`` is the default
    every slot draws with; ``set_seed(slots, seed)`` gives the named slots a seed of their own, which they keep over ``end`` and
    ``drop`` until it is set again or ``seed`` is assigned.  A slot's seed can change only while its position is 0, ``seed`` only
    while every position is 0 (a signal's draws must not change midway); a callable ``eps`` is not taken.  Every guard runs on
    the host before any GPU work and before any bookkeeping changes.  Per launch group the kernels take two tables, the slots'
    (:class:`SessionPlan`) for the encoder side and :func:`decoder_rows` of it for the decoder side; both tables of every group,
    the list of slots to zero and the slots' seeds go to the device in one copy (:func:`vae_session_tables`).

    ``save`` / ``load`` (:class:`_Slots`): a state carries the slot's seed and its draw slot, the slot number in the counter
    word of its draws.  ``load`` gives the target slot that seed (it stays afterwards, as a ``set_seed`` value does) and that
    draw slot until the signal ends or is dropped (``draw_slots``), so the moved stream continues with the bits of
    ``StreamingVAE(..., batch=slots, seed=<the original seed>)`` for the signal in the original slot.  A loaded slot is in
    mid-signal: its seed cannot be changed.  Only while some slot draws as another does the object call
    ``idv_stream_eps_pair_rows_as``; otherwise it launches what it always launched.
    """

    _name = "StreamingVAESessions"
    _state_kind = "vae"
    _skip_halves = 2
    _eps_outputs = 2               # tensors ``eps`` returns: one pair, or the speech and the noise pair
    _per_sample = True             # overlap-add at batch B * ns (self.ifr, then the mean over the samples) or at batch B (self.ifr_b)

    def __init__(self, noisy_encoder, decoder, slots: int, seed: int = 0, latent: str = "speech", average: bool = True,
                 frames_per_launch: int = 64, max_columns: int = 4096, conv: str = "valu"):
        super().__init__(noisy_encoder, decoder, slots, seed, latent, average, None, frames_per_launch, max_columns, conv)
        self._init_slots()
        # state buffers as [outer][slots][inner] for idv_stream_zero_rows; a B * ns-batch buffer has inner = ns * (its inner)
        ns = self.ns
        self._zero_views = [(self.ring, 1, self.plan.ring), (self.carry, 2, ns * self.plan.carry_cap), (self.lstm_state, 16, self.H)]
        self._zero_views += [(h, h.numel() // slots, 1) for h in [self.h_in] + self.h_enc]
        self._zero_views += [(h, h.numel() // (slots * ns), ns) for h in [self.h_dense] + self.h_dec]

    def _init_slots(self):
        super()._init_slots()
        self._own_seeds = {}        # slot -> the seed set_seed or load gave it
        self._moved = {}            # slot -> the slot number its loaded stream draws with, until that signal ends or is dropped

    # ------------------------------------------------------------------ seeds
    @property
    def seed(self) -> int:
        return self._seed

    @seed.setter
    def seed(self, v):
        v = check_seed(v)
        if any(self.positions):
            raise ValueError("seed can be set only between signals (every position 0): a signal's draws must not change midway")
        self._seed = v
        self._own_seeds.clear()

    @property
    def seeds(self) -> List[int]:
        """The seed every slot draws with: its own where ``set_seed`` gave it one, else ``seed``."""
        return [self._own_seeds.get(b, self._seed) for b in range(self.B)]

    @property
    def draw_slots(self) -> List[int]:
        """The slot number every slot draws with (counter word ``draw_slot * ns + s``): its own, except for a slot that
        ``load`` gave a stream from elsewhere, which keeps that stream's until its signal ends or is dropped."""
        return [self._moved.get(b, b) for b in range(self.B)]

    def _draw_table(self) -> List[int]:
        """What travels behind the seeds: nothing while every slot draws as itself (idv_stream_eps_pair_rows), else the draw
        slots (idv_stream_eps_pair_rows_as)."""
        return self.draw_slots if any(v != b for b, v in self._moved.items()) else []

    def _ended(self, slots):
        for b in slots:
            self._moved.pop(b, None)

    # ------------------------------------------------------------------ save / load
    def _state_extra(self):
        return (self.ns, self.zdim, self.H, self.latent, self.average)

    def _state_of(self, b: int, data: torch.Tensor) -> SlotState:
        st = super()._state_of(b, data)
        st.seed, st.draw_slot = self.seeds[b], self.draw_slots[b]
        return st

    def _state_check_extra(self, st: SlotState):
        if st.seed is None or st.draw_slot is None:
            raise ValueError("load: a VAE state carries the seed and the draw slot of its stream")
        check_seed(st.seed)
        v = st.draw_slot
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v or (v + 1) * self.ns > 2 ** 31:
            raise ValueError("load: draw_slot must be an int >= 0 with (draw_slot + 1) * num_samples <= 2^31")

    def _state_set_extra(self, b: int, st: SlotState):
        # the slot now serves a signal in mid-stream: its seed is the stream's (and stays, as a set_seed value does), and it
        # draws as the slot the stream began in until the signal ends
        self._own_seeds[b] = st.seed
        self._moved[b] = st.draw_slot

    def set_seed(self, slots, seed):
        """Give these slots a seed of their own; each must be between signals (position 0)."""
        slots = check_slots(slots, self.B)
        seed = check_seed(seed)
        pos = self.positions
        for b in slots:
            if pos[b]:
                raise ValueError(f"set_seed: slot {b} is {pos[b]} samples into its signal; a slot's seed can be set only between "
                                 "signals (position 0): a signal's draws must not change midway")
        for b in slots:
            self._own_seeds[b] = seed

    def eps(self, t0: int, k: int):
        """The draws frames t0 .. t0+k-1 use, every slot's with its own seed (``seeds``): (eps_r, eps_i), each [slots, ns, k,
        zdim]; a two-latent streamer returns (eps_sr, eps_si, eps_nr, eps_ni)."""
        if isinstance(t0, bool) or not isinstance(t0, int) or t0 < 0 or isinstance(k, bool) or not isinstance(k, int) or k <= 0:
            raise ValueError("eps(t0, k): t0 >= 0 and k > 0 frames")
        B = self.B
        row = [0] * NF
        row[ROW_FIELDS.index("t0")], row[ROW_FIELDS.index("k")] = t0, k
        out = torch.empty(self._eps_outputs, B, self.ns, k, self.zdim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            draws = self._draw_table()
            table = self._upload(torch.tensor(row * B + self.seeds + draws, dtype=torch.int64))
            nr, ni = (p(out[2]), p(out[3])) if self._eps_outputs == 4 else (p(None), p(None))
            if draws:
                call("idv_stream_eps_pair_rows_as", L._P(table.data_ptr() + 8 * B * NF), L._P(table.data_ptr() + 8 * B * (NF + 1)),
                     L._P(table.data_ptr()), i(B), i(self.ns), i(self.zdim), i(k), p(out[0]), p(out[1]), nr, ni, stream_ptr())
            else:
                call("idv_stream_eps_pair_rows", L._P(table.data_ptr() + 8 * B * NF), L._P(table.data_ptr()), i(B), i(self.ns),
                     i(self.zdim), i(k), p(out[0]), p(out[1]), nr, ni, stream_ptr())
        return tuple(out)

    # ------------------------------------------------------------------ push
    def push(self, x: torch.Tensor, counts=None, end=()):
        with torch.no_grad():
            return super().push(x, counts, end)

    def _tables(self, plan: SessionCall):
        return vae_session_tables(plan, self.ns, self.seeds, self._draw_table()), (self.B + self.Bn) * NF

    def _launch(self, g: Group, tables: int, behind: int):
        # the seeds lie behind the zero list, and behind them the draw slots of an object that serves a loaded stream
        draws = L._P(behind + 8 * self.B) if self._draw_table() else None
        return _VAELaunch(g.k, L._P(tables), L._P(tables + 8 * self.B * NF), L._P(behind), draws)

    def _ola_site(self):
        # the overlap-add runs on the decoder side's rows (one per sample) or, behind an estimator, on the slots' rows
        return (self.Bn, self.ifr, "rows_n") if self._per_sample else (self.B, self.ifr_b, "rows")

    def _finish(self, y: torch.Tensor, ldy: int) -> torch.Tensor:
        if not (self._per_sample and self.average):
            return y
        out = torch.zeros(self.B, ldy, dtype=torch.float32, device=self.device)
        if ldy:
            call("idv_mean_over_samples", p(y), i(self.ns), i(self.B), i(ldy), p(out), stream_ptr())
        return out

    # ------------------------------------------------------------------ the per-row kernels of the network
    def _block(self, cp: _ConvPack, c, x0, h0, x1, h1, out, hist, x0hist, Tp: int, Jp: int, dec: bool):
        B, rows = (self.Bn, c.rows_n) if dec else (self.B, c.rows)
        self._conv_call_rows(cp, x0, h0, x1, h1, out, hist, x0hist, B, c.k, Tp, Jp, rows)

    def _lstm(self, c, out, Tp: int, Jp: int):
        call("idv_stream_clstm_wide_rows", p(self.G), p(self.lstm_wt), p(self.lstm_b1), p(self.lstm_state), p(self.hstep), out,
             i(self.H), i(self.B), i(c.k), i(Tp), i(Jp), c.rows, stream_ptr())

    def _draws(self, c):
        """Device pointers of the draws of launch group c, every slot's with its own seed: eps_r / eps_i [B][ns][c.k][zdim], and
        the noise pair behind them where ``eps_buf`` holds one (two decoder chains)."""
        e = [p(t) for t in self.eps_buf]
        nr, ni = e[2:] if len(e) == 4 else (p(None), p(None))
        if c.draws is not None:
            call("idv_stream_eps_pair_rows_as", c.seeds, c.draws, c.rows, i(self.B), i(self.ns), i(self.zdim), i(c.k), e[0], e[1], nr,
                 ni, stream_ptr())
        else:
            call("idv_stream_eps_pair_rows", c.seeds, c.rows, i(self.B), i(self.ns), i(self.zdim), i(c.k), e[0], e[1], nr, ni,
                 stream_ptr())
        return tuple(e)

    def _repeat(self, c, di: int, sk: int, x, xn, Tp: int, Jp: int, Jpn: int):
        sc, sf = self.enc_shapes[sk]
        call("idv_stream_repeat_rows", x, p(self.h_enc[sk]), i(sc), i(sf), i(self.B), i(self.ns), i(c.k), i(Tp), i(Jp), c.rows, xn,
             p(self.h_skip_n[di]), i(Jpn), stream_ptr())
        return self.h_skip_n[di]


class StreamingVAETwoLatentsSessions(_TwoLatents, StreamingVAESessions):
    """The two-latent evaluation of :class:`StreamingVAETwoLatents` for ``slots`` independent signals in one batch, with the
    ``push`` / ``counts`` / ``end`` / ``drop`` / ``positions`` / seeds contract of :class:`StreamingVAESessions`.

        st = StreamingVAETwoLatentsSessions(noisy_encoder, speech_decoder, noise_decoder, slots, outtype="phase_mask", phase=2, seed=0)
        y, m = st.push(x, counts=None, end=())   # x [slots, n] -> y [slots, max(m)], m[b] valid samples of slot b, zeros behind
        st.drop(slots); st.positions; st.reset(); st.seed; st.seeds; st.set_seed(slots, seed)
        sr, si, nr, ni = st.eps(t0, k)           # [slots, ns, k, zdim] each, with every slot's own seed

    Slot b's samples are bit-identical to what ``StreamingVAETwoLatents(noisy_encoder, speech_decoder, noise_decoder, batch=slots,
    outtype=outtype, phase=phase, seed=st.seeds[b], conv=conv)`` returns for the same signal in slot b, whatever the other slots
    do and for every signal the slot serves one after another.  A callable ``eps`` is not taken.

    The network is the lock-step class's on the per-slot kernels of :class:`StreamingVAESessions`, with both tables of a launch
    group; the draws of both latents come from ``idv_stream_eps_pair_rows``.  The estimator (``idv_stream_estimate``) takes no
    table: it runs on all k_launch columns of every slot, each output column from its own input column alone, and the
    overlap-add, on the slots' table at batch B, reads the columns tl < k_b only.  ``clean_direct`` keeps
    :class:`StreamingVAESessions`'s tail at batch B * ns and, at ``phase=2``, returns its bits for the same seeds.
    ``conv_engines`` as in :class:`StreamingVAETwoLatents`.
    """

    _name = "StreamingVAETwoLatentsSessions"
    _state_kind = "two_latents"
    _eps_outputs = 4

    def _state_extra(self):
        return (self.ns, self.zdim, self.H, self.outtype, self.phase, self.average)

    def __init__(self, noisy_encoder, speech_decoder, noise_decoder, slots: int, outtype: str = "phase_mask", phase: int = 2,
                 seed: int = 0, frames_per_launch: int = 64, max_columns: int = 4096, conv: str = "valu"):
        self._init_two_latents(noisy_encoder, speech_decoder, noise_decoder, slots, outtype, phase, seed, None, frames_per_launch,
                               max_columns, conv)
        self._init_slots()
        self._per_sample = self.noise is None
        # state buffers as [outer][slots][inner]; the estimators leave one overlap-add row per slot, clean_direct one per sample
        ns = self.ns
        self._zero_views = [(self.ring, 1, self.plan.ring), (self.carry, 2, (ns if self._per_sample else 1) * self.plan.carry_cap),
                            (self.lstm_state, 16, self.H)]
        self._zero_views += [(h, h.numel() // slots, 1) for h in [self.h_in] + self.h_enc]
        self._zero_views += [(h, h.numel() // (slots * ns), ns) for ch in self.chains for h in [ch.h_dense] + ch.h_dec]


# ---------------------------------------------------------------------------------------------------------------------------
# Streaming at any sample rate: a stateful rational resampler under the push / flush contract (csrc/stream_resample.hip, DESIGN
# 3.6.5), its sessions form, and wrappers that put one in front of and one behind a streamer of the 16 kHz network.
class ResampleStep(NamedTuple):
    """What one push or flush of a resampled stream does: outputs n0 .. n1-1 from position P0, reading history half ``parity``."""
    n0: int
    n1: int
    P0: int
    parity: int


class ResampleCall(NamedTuple):
    """What one ``push(counts, end)`` of resampler sessions does: ``rows[b]`` is slot b's row of the int64 table (ops.SR_ROW_FIELDS),
    ``m[b]`` its number of output samples, ``zero`` the slots whose history is zeroed at the end."""
    rows: "np.ndarray"
    m: List[int]
    zero: List[int]


class ResamplePlan:
    """Sample bookkeeping of one resampled stream for a reduced ratio up / down (host side only; no tensors).

    With half = 10 * max(up, down), output n reads inputs ceil((n*down - half)/up) .. floor((n*down + half)/up): after P inputs the
    outputs below ``n_final(P) = max(0, ceil((P*up - half)/down))`` are final, and a signal of L inputs has ``n_out(L) = ceil(L *
    up / down)`` outputs.  No pending output reads further back than ``H = floor(2*half/up) + 1`` inputs."""

    def __init__(self, up: int, down: int):
        import math
        for v in (up, down):
            if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
                raise ValueError("ResamplePlan: up and down must be positive ints")
        if math.gcd(up, down) != 1 or max(up, down) > ops.RESAMPLE_MAX_M:
            raise ValueError(f"ResamplePlan: up / down must be reduced, with max(up, down) <= {ops.RESAMPLE_MAX_M}")
        self.up, self.down = up, down
        self.half = 10 * max(up, down)
        self.H = ops.stream_resample_hist(up, down)
        self.reset()

    def reset(self):
        self.n = 0            # samples received
        self.parity = 0       # history half the next call reads

    def n_final(self, P: int) -> int:
        return ops.stream_resample_final(P, self.up, self.down)

    def n_out(self, L: int) -> int:
        return ops.resample_len(L, self.up, self.down)

    @property
    def emitted(self) -> int:
        """Output samples returned so far."""
        return self.n_final(self.n)

    def snapshot(self):
        return (self.n, self.parity)

    def restore(self, snap):
        self.n, self.parity = snap

    def push(self, n_new: int) -> ResampleStep:
        if isinstance(n_new, bool) or not isinstance(n_new, int) or n_new < 0:
            raise ValueError("push: the sample count must be an int >= 0")
        step = ResampleStep(self.emitted, self.n_final(self.n + n_new), self.n, self.parity)
        self.n += n_new
        if n_new:
            self.parity ^= 1          # the call writes the other history half
        return step

    def flush(self) -> ResampleStep:
        """The rest of a signal of ``n`` samples; the state stays (the caller resets, as with :class:`StreamPlan`)."""
        return ResampleStep(self.emitted, self.n_out(self.n), self.n, self.parity)

    def advance(self, periods: int):
        """Move the stream on by ``periods * down`` inputs and ``periods * up`` outputs.  The taps an output uses depend on
        n*down - j*up alone, so the history serves the new position as it stands."""
        if isinstance(periods, bool) or not isinstance(periods, int) or periods < 0:
            raise ValueError("advance: periods must be an int >= 0")
        if self.n * self.up < self.half:
            raise ValueError("advance: the stream must be past its first half filter length (n * up >= half)")
        self.n += periods * self.down


class ResampleSessionPlan:
    """Host-side bookkeeping of ``slots`` independent resampled streams in one batch: :class:`ResamplePlan`'s arithmetic on int64
    arrays, one entry per slot, so that the cost of planning a call does not grow with a python loop over the slots."""

    def __init__(self, slots: int, up: int, down: int):
        if isinstance(slots, bool) or not isinstance(slots, int) or slots <= 0:
            raise ValueError("ResampleSessionPlan: slots must be a positive int")
        one = ResamplePlan(up, down)                  # the guards on the ratio
        self.slots, self.up, self.down, self.half, self.H = slots, up, down, one.half, one.H
        self._n = np.zeros(slots, dtype=np.int64)     # samples received per slot
        self._parity = np.zeros(slots, dtype=np.int64)

    @property
    def positions(self) -> List[int]:
        return self._n.tolist()

    def snapshot(self):
        return (self._n.copy(), self._parity.copy())

    def restore(self, snap):
        self._n, self._parity = snap[0].copy(), snap[1].copy()

    def slot_state(self, b: int):
        """Slot b's host integers (n, parity)."""
        return (int(self._n[b]), int(self._parity[b]))

    def set_slot_state(self, b: int, v):
        self.check_slot_state(v)
        self._n[b], self._parity[b] = v

    def check_slot_state(self, v):
        """The guard on a slot's host integers that come from outside (``load``): n >= 0 and parity in {0, 1}."""
        if (not isinstance(v, (tuple, list)) or len(v) != 2 or any(isinstance(q, bool) or not isinstance(q, int) for q in v)
                or not 0 <= v[0] < 2 ** 50 or v[1] not in (0, 1)):
            raise ValueError("a resampled slot's plan is two ints (n, parity) with 0 <= n < 2^50 and parity 0 or 1")

    def n_final(self, P):
        return np.maximum(0, -((self.half - P * self.up) // self.down))

    def n_out(self, L):
        return -((-L * self.up) // self.down)

    def check(self, counts, end):
        """Every guard of a push, before anything changes -> the counts as an int64 array."""
        c = np.asarray(counts)
        if c.shape != (self.slots,):
            raise ValueError(f"{len(counts)} counts for {self.slots} slots")
        if c.dtype.kind not in "iu" or (c < 0).any():
            raise ValueError("counts must be ints >= 0")
        if any(isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.slots for b in end):
            raise ValueError(f"slot numbers lie in 0 .. {self.slots - 1}")
        return c.astype(np.int64)

    def push(self, counts, end) -> ResampleCall:
        c = self.check(counts, end)
        P0 = self._n
        P1 = P0 + c
        ends = np.zeros(self.slots, dtype=bool)
        ends[list(end)] = True
        ends &= P1 > 0                                # ending a slot that has received nothing is a no-op
        n0 = self.n_final(P0)
        m = np.where(ends, self.n_out(P1), self.n_final(P1)) - n0
        idle = (c == 0) & ~ends
        rows = np.stack([P0, c, n0, m, self._parity, ends.astype(np.int64), idle.astype(np.int64)], axis=1)
        self._parity = np.where(ends, 0, self._parity ^ (c > 0))      # a call with samples writes the other history half
        self._n = np.where(ends, 0, P1)
        return ResampleCall(rows, m.tolist(), np.flatnonzero(ends).tolist())

    def drop(self, slots):
        slots = list(slots)
        self._n[slots] = 0
        self._parity[slots] = 0


def _check_rates(name: str, fs_in, fs_out):
    up, down = ops.resample_ratio(fs_in, fs_out)
    if up == down:
        raise ValueError(f"{name}: fs_in == fs_out = {fs_in} Hz leaves nothing to resample (AtRate / SessionsAtRate pass such a "
                         "stream straight through)")
    return up, down


def _check_device(name: str, device) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError(f"{name} runs on the MI355X only: there is no CPU path")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"{name} runs on the MI355X only: there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


class StreamingResampler:
    """Lock-step streaming resampler for ``batch`` signals from ``fs_in`` to ``fs_out`` Hz.

        rs = StreamingResampler(48000, 16000, batch=B)
        y = rs.push(x)          # x [B, n >= 0] float32 on the GPU -> [B, m]: the output samples that became final
        y = rs.flush()          # end of all B signals -> the rest; the resampler is then reset ([B, 0] for empty signals)

    All pushes and the flush together are ``inference.resample(x_full, fs_in, fs_out)[0]`` bit for bit, however the signal is
    cut: the same fp32 taps (``scipy.signal.resample_poly``'s default filter, not soxr), the same terms in the same order in one
    double accumulator per output.  Output n is returned by the push that delivers input ``floor((n*down + half)/up)``, half = 10
    max(up, down): a delay of half/up input samples.  State per stream: the last ``plan.H`` input samples and the position; a
    stream may run past 2^31 samples, and the cost of a push does not depend on the position.  ``x`` may be a column slice of a
    longer buffer (any row pitch); anything else is made contiguous.  ``taps_mode`` ("auto", "mem", "lds") forces where the kernel
    reads the taps; every mode gives the same bits.
    """

    def __init__(self, fs_in: int, fs_out: int, batch: int, device=None, taps_mode: str = "auto"):
        up, down = _check_rates("StreamingResampler", fs_in, fs_out)
        if isinstance(batch, bool) or not isinstance(batch, int) or not 0 < batch <= ops.ROWS_MAX_ROWS:
            raise ValueError(f"StreamingResampler: batch must be an int in 1 .. {ops.ROWS_MAX_ROWS}")
        if taps_mode not in ops.SR_TAPS_MODES:
            raise ValueError(f"taps_mode must be one of {tuple(ops.SR_TAPS_MODES)}")
        self.fs_in, self.fs_out, self.B, self.taps_mode = fs_in, fs_out, batch, taps_mode
        self.device = _check_device("StreamingResampler", device)
        self.plan = ResamplePlan(up, down)
        self.hist = torch.zeros(2, batch, self.plan.H, dtype=torch.float32, device=self.device)
        ops.resample_taps(up, down, self.device)

    def reset(self):
        """Zero the history and the bookkeeping (done by flush)."""
        self.hist.zero_()
        self.plan.reset()

    def push(self, x: torch.Tensor) -> torch.Tensor:
        check_input(x, self.B, self.device)
        n_new = int(x.shape[1])
        if n_new > ops.RESAMPLE_MAX_LEN:
            raise ValueError(f"push: {n_new} samples in one call; at most 2^27 are supported")
        pl = self.plan
        with torch.cuda.device(self.device):
            st = pl.push(n_new)
            return ops.stream_resample(self.hist, st.parity, x, n_new, st.P0, False, st.n0, st.n1 - st.n0, pl.up, pl.down,
                                       self.taps_mode)

    def flush(self) -> torch.Tensor:
        pl = self.plan
        with torch.cuda.device(self.device):
            st = pl.flush()
            y = ops.stream_resample(self.hist, st.parity, None, 0, st.P0, True, st.n0, st.n1 - st.n0, pl.up, pl.down, self.taps_mode)
            self.reset()
        return y

    def _advance(self, periods: int):
        """Test hook: ``periods * down`` input samples and ``periods * up`` outputs further on, the history untouched."""
        self.plan.advance(periods)


class StreamingResamplerSessions(_Slots):
    """Streaming resampler for ``slots`` independent signals in one batch, with the contract of :class:`StreamingSessions`.

        rs = StreamingResamplerSessions(44100, 16000, slots)
        y, m = rs.push(x, counts=None, end=())   # x [slots, n] float32 on the GPU -> y [slots, max(m)], m[b] samples of slot b, zeros behind
        rs.drop(slots); rs.positions; rs.reset()

    ``counts[b]`` leading samples of row b are new for slot b (nothing at or past ``x[b, counts[b]]`` is read); ``end`` names
    the slots whose signal ends after this call's samples: the call returns the rest of their outputs, their history is zeroed
    and their next samples begin a new signal.  Ending a slot that has received nothing is a no-op.  Slot b's samples are the
    bits :class:`StreamingResampler` returns for the same signal in the same slot, whatever the other slots do.  Every guard runs
    on the host before any GPU work and before any bookkeeping changes; the table of a call is held to
    ``idv_stream_resample_rows_check`` before it goes to the device.
    """

    _state_kind = "resampler"

    def _state_head(self):
        return (self.up, self.down, self.H)

    def __init__(self, fs_in: int, fs_out: int, slots: int, device=None, taps_mode: str = "auto"):
        up, down = _check_rates("StreamingResamplerSessions", fs_in, fs_out)
        if isinstance(slots, bool) or not isinstance(slots, int) or not 0 < slots <= ops.ROWS_MAX_ROWS:
            raise ValueError(f"StreamingResamplerSessions: slots must be an int in 1 .. {ops.ROWS_MAX_ROWS}")
        if taps_mode not in ops.SR_TAPS_MODES:
            raise ValueError(f"taps_mode must be one of {tuple(ops.SR_TAPS_MODES)}")
        self.fs_in, self.fs_out, self.B, self.taps_mode = fs_in, fs_out, slots, taps_mode
        self.up, self.down = up, down
        self.device = _check_device("StreamingResamplerSessions", device)
        if int(L.lib().idv_stream_resample_row_fields()) != len(ops.SR_ROW_FIELDS):
            raise L.IdvError("libidccrn_hip.so and ops.SR_ROW_FIELDS disagree about the row table")
        self._init_tables(ResampleSessionPlan(slots, up, down))
        self.H = self.sessions.H
        self.hist = torch.zeros(2, slots, self.H, dtype=torch.float32, device=self.device)
        self._zero_views = [(self.hist, 2, self.H)]
        ops.resample_taps(up, down, self.device)

    def reset(self):
        """Zero every slot's history and bookkeeping."""
        self.hist.zero_()
        self.sessions.drop(range(self.B))

    def check(self, x, counts, end):
        """Every guard of a push (host only; nothing changes) -> (counts, end) as lists."""
        check_input(x, self.B, self.device)
        n = int(x.shape[1])
        if n > ops.RESAMPLE_MAX_LEN:
            raise ValueError(f"push: {n} samples in one call; at most 2^27 are supported")
        return check_counts(counts, self.B, n), check_slots(end, self.B)

    def push(self, x: torch.Tensor, counts=None, end=()):
        counts, end = self.check(x, counts, end)
        n = int(x.shape[1])
        snap = self.sessions.snapshot()
        plan = self.sessions.push(counts, end)
        ldy = max(plan.m)
        NR = len(ops.SR_ROW_FIELDS)
        host = torch.from_numpy(np.concatenate([plan.rows.ravel(), np.asarray(plan.zero, dtype=np.int64)]))
        rc = L.lib().idv_stream_resample_rows_check(L._P(host.data_ptr()), self.B, n, self.up, self.down, self.H, ldy)
        if rc != 0:                                  # a bad table never reaches a kernel
            self.sessions.restore(snap)
            raise L.IdvError(f"idv_stream_resample_rows_check refused the table (status {rc})")
        with torch.cuda.device(self.device):
            if not any(counts) and not plan.zero:    # every slot idle
                return torch.zeros(self.B, 0, dtype=torch.float32, device=self.device), plan.m
            table = self._upload(host)
            y = ops.stream_resample_rows(self.hist, x if n else None, n, L._P(table.data_ptr()), ldy, self.up, self.down,
                                         self.taps_mode)
            self._zero(L._P(table.data_ptr() + 8 * self.B * NR), len(plan.zero))
        return y, plan.m


def _check_wrapped(name: str, streamer, kinds, fs, model_fs):
    if not isinstance(streamer, kinds):
        raise ValueError(f"{name} wraps one of {', '.join(k.__name__ for k in kinds)}")
    if not getattr(streamer, "average", True):
        raise ValueError(f"{name}: a streamer with average=False returns num_samples rows per stream; resample those with a "
                         "StreamingResampler of that many rows")
    ops.resample_ratio(fs, model_fs)                 # the guards on the rates


class AtRate:
    """A lock-step streamer of the ``model_fs`` network (:class:`StreamingDCCRN`, :class:`StreamingVAE`,
    :class:`StreamingVAETwoLatents`) for signals at ``fs`` Hz: a :class:`StreamingResampler` in front of it and one behind it.

        st = AtRate(StreamingDCCRN(model, batch=B), 48000)
        y = st.push(x)          # x [B, n] at fs on the GPU -> the enhanced samples at fs that became final
        y = st.flush()          # the three stages flush in order, each stage's flush output being the next one's last push

    Pushes plus flush return, bit for bit and however the signal is cut, ``inference.resample(E(inference.resample(x, fs,
    model_fs)[0]), model_fs, fs)[0]`` with E the wrapped streamer's whole-signal push + flush; equality with the offline model
    follows within the streamer's own tolerance.  ``fs == model_fs`` passes straight through to the wrapped streamer.  Every guard
    runs on the host before any GPU work and before any bookkeeping changes, the wrapped streamer's refusal to end a signal of
    0 < L16 <= n_fft/2 samples (L16 = ceil(L * up / down)) included: a refused call leaves all three stages as they were.  Added
    latency: half/up input samples per resampler, 30 samples (0.625 ms) at 48 kHz down and the same again on the way back.
    """

    def __init__(self, streamer, fs: int, model_fs: int = 16000):
        _check_wrapped("AtRate", streamer, (StreamingDCCRN, StreamingVAE), fs, model_fs)
        self.streamer, self.fs, self.model_fs = streamer, fs, model_fs
        self.B, self.device = streamer.B, streamer.device
        self.down = self.up = None
        if fs != model_fs:
            self.down = StreamingResampler(fs, model_fs, self.B, self.device)
            self.up = StreamingResampler(model_fs, fs, self.B, self.device)

    def reset(self):
        self.streamer.reset()
        if self.down is not None:
            self.down.reset()
            self.up.reset()

    def push(self, x: torch.Tensor) -> torch.Tensor:
        if self.down is None:
            return self.streamer.push(x)
        check_input(x, self.B, self.device)
        if int(x.shape[1]) > ops.RESAMPLE_MAX_LEN:
            raise ValueError(f"push: {int(x.shape[1])} samples in one call; at most 2^27 are supported")
        return self.up.push(self.streamer.push(self.down.push(x)))

    def flush(self) -> torch.Tensor:
        if self.down is None:
            return self.streamer.flush()
        self.streamer.plan.check_flush(self.down.plan.n_out(self.down.plan.n))      # before anything changes
        mid = self.streamer.push(self.down.flush())
        mid = torch.cat([mid, self.streamer.flush()], dim=1)
        return torch.cat([self.up.push(mid), self.up.flush()], dim=1)


class SessionsAtRate:
    """A sessions streamer of the ``model_fs`` network (:class:`StreamingSessions`, :class:`StreamingVAESessions`,
    :class:`StreamingVAETwoLatentsSessions`) for signals at ``fs`` Hz, with the same ``push`` / ``drop`` / ``positions`` contract.

        st = SessionsAtRate(StreamingSessions(model, slots), 44100)
        y, m = st.push(x, counts=None, end=())   # x [slots, n] at fs -> y [slots, max(m)] at fs, m[b] samples of slot b, zeros behind
        st.drop(slots); st.positions; st.set_seed(slots, seed)

    The down-resampler's ``m`` is the streamer's ``counts`` and the streamer's ``m`` the up-resampler's ``counts``: at 44.1 kHz
    slots at different phases get 159, 160 or 161 samples from the same push.  ``end`` passes through all three stages within
    the call.  Slot b returns the bits :class:`AtRate` returns for the same signal in the same slot.  ``positions`` counts samples
    at ``fs``.  Every guard runs on the host before any GPU work and before any bookkeeping changes, as in :class:`AtRate`.
    """

    def __init__(self, sessions, fs: int, model_fs: int = 16000):
        _check_wrapped("SessionsAtRate", sessions, (StreamingSessions, StreamingVAESessions), fs, model_fs)
        self.sessions, self.fs, self.model_fs = sessions, fs, model_fs
        self.B, self.device = sessions.B, sessions.device
        self.down = self.up = None
        if fs != model_fs:
            self.down = StreamingResamplerSessions(fs, model_fs, self.B, self.device)
            self.up = StreamingResamplerSessions(model_fs, fs, self.B, self.device)

    @property
    def positions(self) -> List[int]:
        return self.sessions.positions if self.down is None else self.down.positions

    def reset(self):
        self.sessions.reset()
        if self.down is not None:
            self.down.reset()
            self.up.reset()

    def drop(self, slots):
        slots = check_slots(slots, self.B)
        self.sessions.drop(slots)
        if self.down is not None:
            self.down.drop(slots)
            self.up.drop(slots)

    def save(self, slots) -> List[SlotState]:
        """The streams of these slots through all three stages, one :class:`SlotState` of kind ``"at_rate"`` per slot whose
        ``stages`` are the states of the down-resampler, the network and the up-resampler (``fs == model_fs``: the wrapped
        sessions' own states).  Three gather launches, no host synchronisation; the slots are untouched."""
        if self.down is None:
            return self.sessions.save(slots)
        slots = _slot_list(slots, self.B, "save")
        layout = (self.fs, self.model_fs)
        stages = zip(self.down.save(slots), self.sessions.save(slots), self.up.save(slots))
        return [SlotState("at_rate", layout, (), torch.empty(0, dtype=torch.float32), stages=st) for st in stages]

    def load(self, slots, states, overwrite: bool = False):
        """``load`` of the three stages (see :meth:`_Slots.load`).  Every guard of every stage runs before anything changes:
        if one stage refuses, none is touched.  Beyond the stages' own guards the three plans must belong together: the network
        has received what the down-resampler has returned, and the up-resampler what the network has returned."""
        if self.down is None:
            return self.sessions.load(slots, states, overwrite)
        slots = _slot_list(slots, self.B, "load")
        if isinstance(states, SlotState) or not isinstance(states, Iterable):
            raise ValueError("load: states must be a list of SlotState, one per slot")
        states = list(states)
        if len(states) != len(slots):
            raise ValueError(f"load: {len(states)} states for {len(slots)} slots")
        for st in states:
            if not isinstance(st, SlotState) or st.kind != "at_rate" or st.stages is None or len(st.stages) != 3:
                raise ValueError("load: SessionsAtRate takes states of kind 'at_rate' with three stages")
            if st.layout != (self.fs, self.model_fs):
                raise ValueError(f"load: the state's rates {st.layout} are not this object's {(self.fs, self.model_fs)}")
        parts = [[st.stages[j] for st in states] for j in range(3)]
        objs = (self.down, self.sessions, self.up)
        for obj, part in zip(objs, parts):
            obj._load_check(slots, part, overwrite)
        for d, net, u in zip(*parts):
            if net.plan[0] != int(self.down.sessions.n_final(d.plan[0])) or u.plan[0] != net.plan[2]:
                raise ValueError("load: the three stages of a state do not belong together (the network has received what the "
                                 "down-resampler returned, the up-resampler what the network returned)")
        for obj, part in zip(objs, parts):
            obj._load_apply(slots, part)

    def set_seed(self, slots, seed):
        """Forwarded to the wrapped VAE sessions (a slot's seed can be set only between signals)."""
        if not hasattr(self.sessions, "set_seed"):
            raise ValueError(f"{type(self.sessions).__name__} draws nothing: it has no seeds")
        self.sessions.set_seed(slots, seed)

    def push(self, x: torch.Tensor, counts=None, end=()):
        if self.down is None:
            return self.sessions.push(x, counts, end)
        counts, end = self.down.check(x, counts, end)
        pos = self.down.positions
        for b in end:                                # the wrapped streamer's refusal, before anything changes
            L16 = self.down.sessions.n_out(pos[b] + counts[b])
            if L16 > 0:
                self.sessions.plan.check_flush(L16)
        y, m = self.down.push(x, counts, end)
        y, m = self.sessions.push(y, m, end)
        return self.up.push(y, m, end)
