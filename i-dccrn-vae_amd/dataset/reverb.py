"""Reverberation on the device (csrc/reverb.hip): the step of the DNS-Challenge synthesizer that convolves the clean
utterance with a room impulse response before it is mixed (``add_pyreverb``: ``scipy.signal.fftconvolve(clean, rir)[:len(clean)]``).

  * :func:`reverb`  convolves a padded batch of rows with one impulse response per row (or one for all);
  * :class:`RirPool`  holds impulse responses of any lengths in one device buffer, with the index of every peak;
  * :func:`draw_reverb`  names the impulse response of every row of training batch k on the host, a function of ``(seed, k)`` alone;
  * :func:`reverb_draw`  convolves the rows a :class:`~.mix.Draw` names, read in place from the clean pool WITH the samples in front
    of each segment, so that a segment equals the cut from the convolved recording.

``y[i] = float32(sum_k h[k] x[i - k])``, the sum of exact products in double (tests/reverb_ref.py; parity with the synthesizer package
itself is unpinned).  A sum that is zero comes back as +0, so a -0.0 sample passes through a unit impulse as +0.0; every other sample
keeps its bits.  There is no host fallback: a CPU tensor is refused.
"""
from __future__ import annotations

import math
import random
from typing import Sequence

import numpy as np
import torch

from .. import ops
from .mix import MAX_LEN, Draw, SignalPool

MAX_TAPS = ops.REVERB_MAX_TAPS


def _int(name: str, v, lo: int, who: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{who}: {name} = {v!r}: an integer >= {lo} is expected")
    return v


def _counts(name: str, v, B: int, upper: list, who: str) -> list:
    """One integer per row, 1 <= v[b] <= upper[b] (host only)."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda or v.dim() != 1 or v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"{who}: {name} must be a python sequence or a 1-D CPU integer tensor")
        v = v.tolist()
    elif isinstance(v, np.ndarray):
        v = v.tolist()
    elif isinstance(v, int) and not isinstance(v, bool):
        v = [v] * B
    elif isinstance(v, (str, bytes)) or not isinstance(v, Sequence):
        raise ValueError(f"{who}: {name} must be an integer, a python sequence or a 1-D CPU integer tensor")
    if any(isinstance(t, bool) or not isinstance(t, int) for t in v):
        raise ValueError(f"{who}: {name} must be integers (sample counts)")
    if len(v) != B:
        raise ValueError(f"{who}: {len(v)} values of {name} for {B} rows")
    for b, (t, u) in enumerate(zip(v, upper)):
        if not 1 <= t <= u:
            raise ValueError(f"{who}: {name}[{b}] = {t}: 1 .. {u} is expected")
    return list(v)


def reverb(x: torch.Tensor, rir: torch.Tensor, lengths=None, rir_lengths=None, taps=None) -> torch.Tensor:
    """``x`` [B, L] and ``rir`` [B, K] (or [1, K]: one response for every row) float32 on the GPU -> ``y`` float32 [B, L]: row b, its
    first ``lengths[b]`` samples (default L), convolved with the first ``taps[b]`` samples of its impulse response (default
    ``rir_lengths[b]``, by default K) and cut to its own length; zeros from there on.  ``taps``: an integer or one per row.  Nothing
    at or past a row's length or a response's tap count is read.  The guards run on the host before any device work."""
    for t, name, what in ((x, "x", "[B, L]"), (rir, "rir", "[B, K]")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"reverb: {name} must be a {what} tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"reverb: {name} is {t.dtype}; float32 samples are expected")
    B, L = x.shape
    K = rir.shape[1]
    if B < 1 or B > 65535:
        raise ValueError(f"reverb: a batch of {B} rows; 1 .. 65535 are supported")
    if L < 1 or L > MAX_LEN:
        raise ValueError(f"reverb: rows of {L} samples; 1 .. 2^27 are supported")
    if K < 1 or K > MAX_TAPS:
        raise ValueError(f"reverb: impulse responses of {K} taps; 1 .. {MAX_TAPS} are supported")
    if rir.shape[0] not in (1, B):
        raise ValueError(f"reverb: {rir.shape[0]} impulse responses for {B} rows; one per row or one for all is expected")
    lens = [L] * B if lengths is None else ops.check_lengths(lengths, B, L, None)
    rlens = [K] * B if rir_lengths is None else _counts("rir_lengths", rir_lengths, B, [K] * B, "reverb")
    tp = rlens if taps is None else _counts("taps", taps, B, rlens, "reverb")
    ops.check_dev_f32(x, "x")
    ops.check_dev_f32(rir, "rir", x.device)
    x, rir = ops._ragged_rows(x), ops._ragged_rows(rir)
    table = torch.tensor([lens, tp, [0] * B], dtype=torch.int32).to(x.device)
    h_off = None
    if rir.shape[0] == 1 and B > 1:                        # one response for all rows: every row's taps start at offset 0
        h_off = torch.zeros(B, dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        return ops.reverb_apply(x, None, rir, h_off, table, B, L, K)


def rir_peaks(signals) -> list:
    """The index of max|h| of every impulse response, the first on ties (host only)."""
    out = []
    for s in signals:
        a = np.abs(s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s))
        out.append(int(np.argmax(a)))
    return out


def early_taps(lengths: Sequence[int], peaks: Sequence[int], ms: float = 50.0, fs: int = 16000) -> list:
    """``min(len_k, peaks[k] + 1 + round(ms fs / 1000))``: the taps of the direct sound and of the reflections of the ``ms``
    milliseconds behind it (host only)."""
    if isinstance(ms, bool) or not isinstance(ms, (int, float)) or not math.isfinite(ms) or ms < 0:
        raise ValueError(f"early_taps: ms = {ms!r}: a finite number >= 0 is expected")
    _int("fs", fs, 1, "early_taps")
    extra = int(round(ms * fs / 1000.0))
    return [min(n, pk + 1 + extra) for n, pk in zip(lengths, peaks)]


class RirPool(SignalPool):
    """A :class:`~.mix.SignalPool` of room impulse responses of at most 2^16 samples each.  ``peaks[k]``: the index of max|h| of
    member k (the first on ties), found once on the host from the arrays as given.  Behind the members the buffer keeps one sample
    1.0, the unit impulse that dry rows are convolved with (``unit_offset``)."""

    def __init__(self, signals, device="cuda", fs: int = 16000):
        _int("fs", fs, 1, "RirPool")
        if not isinstance(signals, (torch.Tensor, np.ndarray)) and isinstance(signals, Sequence):
            for k, s in enumerate(signals):
                if isinstance(s, (torch.Tensor, np.ndarray)) and s.ndim == 1 and s.shape[0] > MAX_TAPS:
                    raise ValueError(f"RirPool: impulse response {k} has {s.shape[0]} samples; at most {MAX_TAPS} are supported")
        super().__init__(signals, device)
        self.fs = fs
        self.peaks = rir_peaks(signals)
        self.unit_offset = int(self.data.shape[0])
        self.data = torch.cat([self.data, torch.ones(1, dtype=torch.float32, device=self.device)])

    @classmethod
    def shoebox(cls, room, source, mic, beta, taps, fs: int = 16000, device="cuda", c: float = 343.0, max_order=None,
                max_images: int = 2 ** 28) -> "RirPool":
        """The pool of the image-source responses of B rectangular rooms (dataset/rir.py ``shoebox_rir``, whose arguments and host
        guards these are), member b of ``taps[b]`` samples.  The samples never leave the device: the rows are packed
        there and the peaks come from ``idv_ism_peaks``, one small download.  Every attribute is what ``RirPool([rows .cpu()])`` of
        the same rows holds."""
        from . import rir as R
        _int("fs", fs, 1, "RirPool.shoebox")
        geom, tp, mo = R.check_rooms(room, source, mic, beta, taps, fs, c, max_order, max_images, who="RirPool.shoebox")
        device = R._device(device, "RirPool.shoebox")
        h, dev_taps, _ = R._launch(geom, tp, mo, device)
        with torch.cuda.device(device):
            peaks = ops.ism_peaks(h, dev_taps)
            keep = torch.arange(h.shape[1], device=device)[None, :] < dev_taps[:, None]
            data = torch.cat([h[keep], torch.ones(1, dtype=torch.float32, device=device)])
        self = cls.__new__(cls)
        self.lengths = list(tp)
        self.offsets = [0]
        for n in self.lengths[:-1]:
            self.offsets.append(self.offsets[-1] + n)
        self.data, self.device = data, data.device
        self.fs = fs
        self.peaks = [int(v) for v in peaks.tolist()]
        self.unit_offset = int(data.shape[0]) - 1
        return self

    def early_taps(self, ms: float = 50.0) -> list:
        """One tap count per member: the direct sound plus ``ms`` milliseconds of early reflections."""
        return early_taps(self.lengths, self.peaks, ms, self.fs)


def draw_reverb(k: int, seed: int, n_rirs: int, batch: int, p: float = 0.5) -> list:
    """The impulse response of every row of batch ``k``: an index below ``n_rirs`` with probability ``p``, -1 (dry) otherwise.  Host
    only, a function of ``(seed, k)`` and the arguments alone, from a generator of its own: what :func:`~.mix.draw_batch` returns
    for ``(seed, k)`` does not change."""
    _int("k", k, 0, "draw_reverb")
    _int("seed", seed, 0, "draw_reverb")
    _int("n_rirs", n_rirs, 1, "draw_reverb")
    _int("batch", batch, 1, "draw_reverb")
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError(f"draw_reverb: p = {p!r}: a probability in [0, 1] is expected")
    rng = random.Random(f"rir:{seed}:{k}")
    out = []
    for _ in range(batch):
        wet, idx = rng.random() < p, rng.randrange(n_rirs)           # both are drawn for every row
        out.append(idx if wet else -1)
    return out


def reverb_rows(x: torch.Tensor, rir_pool: RirPool, rir_ids: Sequence[int], taps=None) -> torch.Tensor:
    """``x`` [B, L] float32 on the pool's device, every row whole (an assembled clip: the history in front of it is zero), each
    convolved as by :func:`reverb` with member ``rir_ids[b]`` of ``rir_pool`` read in place (-1: dry, the unit impulse) -> float32
    [B, L].  ``taps``: one tap count per MEMBER, as in :func:`reverb_draw`.  The guards run on the host."""
    if not isinstance(rir_pool, RirPool):
        raise ValueError("reverb_rows: rir_pool must be a RirPool")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("reverb_rows: x must be a float32 [B, L] tensor")
    B, L = x.shape
    if B < 1 or B > 65535 or L < 1 or L > MAX_LEN:
        raise ValueError(f"reverb_rows: a batch of {B} rows of {L} samples; 1 .. 65535 rows of 1 .. 2^27 samples are supported")
    if isinstance(rir_ids, (str, bytes)) or not isinstance(rir_ids, Sequence) or len(rir_ids) != B:
        raise ValueError(f"reverb_rows: rir_ids must name one impulse response (or -1) for each of the {B} rows")
    if any(isinstance(r, bool) or not isinstance(r, int) or not -1 <= r < len(rir_pool) for r in rir_ids):
        raise ValueError(f"reverb_rows: rir_ids must be integers in -1 .. {len(rir_pool) - 1} (-1: dry)")
    member_taps = rir_pool.lengths if taps is None else _counts("taps", taps, len(rir_pool), rir_pool.lengths, "reverb_rows")
    if not x.is_cuda or x.device != rir_pool.device:
        raise ValueError(f"reverb_rows: x is on {x.device}, rir_pool on {rir_pool.device}")
    x = ops._ragged_rows(x)
    tp = [1 if r < 0 else member_taps[r] for r in rir_ids]
    h_off = torch.tensor([rir_pool.unit_offset if r < 0 else rir_pool.offsets[r] for r in rir_ids], dtype=torch.int64).to(x.device)
    table = torch.tensor([[L] * B, tp, [0] * B], dtype=torch.int32).to(x.device)
    with torch.cuda.device(x.device):
        return ops.reverb_apply(x, None, rir_pool.data, h_off, table, B, L, max(tp))


def reverb_draw(clean_pool: SignalPool, rir_pool: RirPool, draw: Draw, rir_ids: Sequence[int], samples: int, taps=None) -> torch.Tensor:
    """The clean rows a :class:`~.mix.Draw` names, each convolved with member ``rir_ids[b]`` of ``rir_pool`` (-1: dry, the unit
    impulse) -> float32 [rows, samples], zeros from a row's length on.  Rows and responses are read in place through device tables of
    offsets; a segment that starts inside its recording also reads the up to ``taps - 1`` samples in front of it, so the result is
    the segment cut from the convolved recording.  ``taps``: one tap count per MEMBER of ``rir_pool`` (default: its length), as
    :meth:`RirPool.early_taps` returns.  The guards run on the host."""
    if not isinstance(clean_pool, SignalPool) or not isinstance(rir_pool, RirPool):
        raise ValueError("reverb_draw: clean_pool must be a SignalPool and rir_pool a RirPool")
    if clean_pool.device != rir_pool.device:
        raise ValueError(f"reverb_draw: the pools are on {clean_pool.device} and {rir_pool.device}")
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1 or samples > MAX_LEN:
        raise ValueError(f"reverb_draw: samples = {samples!r}; 1 .. 2^27 are supported")
    B = len(draw.lens)
    if B < 1 or B > 65535 or len(draw.clean_id) != B or len(draw.clean_start) != B:
        raise ValueError(f"reverb_draw: a draw of {B} rows; 1 .. 65535, every field of the same length, are supported")
    if isinstance(rir_ids, (str, bytes)) or not isinstance(rir_ids, Sequence) or len(rir_ids) != B:
        raise ValueError(f"reverb_draw: rir_ids must name one impulse response (or -1) for each of the {B} rows")
    member_taps = rir_pool.lengths if taps is None else _counts("taps", taps, len(rir_pool), rir_pool.lengths, "reverb_draw")
    x_off, h_off, tp, hist = [], [], [], []
    for b in range(B):
        ci, s0, n, r = draw.clean_id[b], draw.clean_start[b], draw.lens[b], rir_ids[b]
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (ci, s0, n, r)):
            raise ValueError(f"reverb_draw: row {b} does not hold integers")
        if not 0 <= ci < len(clean_pool):
            raise ValueError(f"reverb_draw: row {b} names recording {ci}; the pool holds {len(clean_pool)}")
        if not (1 <= n <= samples and 0 <= s0 and s0 + n <= clean_pool.lengths[ci]):
            raise ValueError(f"reverb_draw: row {b}: samples [{s0}, {s0 + n}) of a recording of {clean_pool.lengths[ci]}, at most {samples}")
        if not -1 <= r < len(rir_pool):
            raise ValueError(f"reverb_draw: row {b} names impulse response {r}; the pool holds {len(rir_pool)} (-1: dry)")
        x_off.append(clean_pool.offsets[ci] + s0)
        h_off.append(rir_pool.unit_offset if r < 0 else rir_pool.offsets[r])
        tp.append(1 if r < 0 else member_taps[r])
        hist.append(min(s0, tp[-1] - 1))
    dev = clean_pool.device
    off = torch.tensor([x_off, h_off], dtype=torch.int64).to(dev)
    table = torch.tensor([draw.lens, tp, hist], dtype=torch.int32).to(dev)
    with torch.cuda.device(dev):
        return ops.reverb_apply(clean_pool.data, off[0], rir_pool.data, off[1], table, B, samples, max(tp))
