"""Mixture synthesis on the device (csrc/mix.hip): the step that turns speech and noise recordings into the
``(noisy, clean, noise)`` triples every recipe reads.

  * :func:`snr_mix`  mixes a padded batch of clean rows with cyclically read noise rows at a given SNR and level, per row;
  * :class:`SignalPool`  holds recordings of any lengths in one device buffer;
  * :func:`mix_draw`  mixes rows read in place from two pools; ``clean=``: a [rows, samples] device tensor stands in for the clean
    rows (the reverberant speech of dataset/reverb.py ``reverb_draw``);
  * :func:`draw_batch`  names the rows and parameters of training batch k on the host, a function of ``(seed, k)`` alone;
  * :class:`DynamicMixtures`  yields ``(noisy, clean, noise)`` like ``dataload.SyntheticMixtures``, mixed afresh from two pools; with
    ``rir_pool=`` a ``RirPool`` the rows that ``draw_reverb`` picks (``p_reverb``) are convolved with a room impulse response before
    they are mixed, and ``target="early"`` yields as ``clean`` the speech under the direct sound and ``early_ms``
    milliseconds of reflections instead of the whole response.

The definition is ``normalize`` / ``snr_mixer`` / ``segmental_snr_mixer`` of the DNS-Challenge synthesizer, restated in float64 in
tests/mix_ref.py (parity with that package is unpinned: it is not installed where this was written), with one deliberate difference: a
window's level is the true dB of its mean square.  There is no host fallback: a CPU tensor is refused.
"""
from __future__ import annotations

import math
import random
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import ops

MAX_LEN = ops.MIX_MAX_LEN


def _finite(name: str, v, who: str = "mix") -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{who}: {name} = {v!r}: a finite number is expected")
    return float(v)


def check_mix_args(target_db, clip, win, thresh_db, segmental) -> tuple:
    """The guards on the mixer's parameters (host only, no device use) -> (target_db, clip, win, thresh_db, segmental)."""
    target_db, clip, thresh_db = _finite("target_db", target_db), _finite("clip", clip), _finite("thresh_db", thresh_db)
    if not 0.0 < clip <= 1.0:
        raise ValueError(f"mix: clip = {clip!r}: a threshold in (0, 1] is expected")
    if isinstance(win, bool) or not isinstance(win, int) or win < 4 or win > MAX_LEN or win % 4:
        raise ValueError(f"mix: win = {win!r}: a multiple of 4 in 4 .. 2^27 is expected")
    if not isinstance(segmental, bool):
        raise ValueError(f"mix: segmental = {segmental!r}: True or False is expected")
    return target_db, clip, win, thresh_db, segmental


def _per_row(name: str, v, B: int) -> list:
    """A scalar or one value per row -> B finite floats."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise ValueError(f"mix: {name} must be a number, a python sequence or a CPU tensor")
        v = v.tolist()
    if isinstance(v, np.ndarray):
        v = v.tolist()
    if isinstance(v, (str, bytes)):
        raise ValueError(f"mix: {name} = {v!r}: a finite number is expected")
    if not isinstance(v, Sequence):
        return [_finite(name, v)] * B
    if len(v) != B:
        raise ValueError(f"mix: {len(v)} values of {name} for a batch of {B} rows")
    return [_finite(f"{name}[{b}]", x) for b, x in enumerate(v)]


def _signals(x, name: str):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"mix: {name} must be a [B, L] tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"mix: {name} is {x.dtype}; float32 samples are expected")
    if x.shape[0] < 1 or x.shape[0] > 65535:
        raise ValueError(f"mix: a batch of {x.shape[0]} rows; 1 .. 65535 are supported")
    if x.shape[1] < 1 or x.shape[1] > MAX_LEN:
        raise ValueError(f"mix: rows of {x.shape[1]} samples; 1 .. 2^27 are supported")


def _mix(rows: ops.MixRows, snr: list, level: list, segmental, target_db, clip, win, thresh_db, stats: bool):
    par = torch.tensor(list(zip(snr, level)), dtype=torch.float64).to(rows.clean.device)
    rec, windows = ops.mix_gains(rows, par, segmental, target_db, clip, win, thresh_db)
    noisy, clean_out, noise_out = ops.mix_write(rows, rec)
    F = ops.MIX_FIELD
    info = {"g_clean": rec[:, F["g_clean"]], "g_noise": rec[:, F["g_noise"]], "level_db": rec[:, F["level_db"]],
            "clipped": rec[:, F["clipped"]].to(torch.int32), "active": rec[:, F["active"]].to(torch.int32)}
    if stats:
        info.update({k: rec[:, F[k]] for k in ("max_c", "sum_c2", "max_v", "sum_v2", "act_c2", "act_v2", "sum_y2", "max_y")})
        info["windows"] = windows.clone()
    return noisy, clean_out, noise_out, info


def snr_mix(clean: torch.Tensor, noise: torch.Tensor, snr_db, level_db=-25.0, lengths=None, noise_lengths=None, noise_offsets=None,
            segmental: bool = False, target_db: float = -25.0, clip: float = 0.99, win: int = 1600, thresh_db: float = -50.0,
            stats: bool = False):
    """``clean`` [B, L] and ``noise`` [B, Ln] float32 on the GPU -> ``(noisy, clean_out, noise_out, info)``, the three signals
    float32 [B, L].  Row b holds ``lengths[b]`` clean samples (default L) and ``noise_lengths[b]`` noise samples (default Ln), read
    cyclically from ``noise_offsets[b]`` (default 0); the noise is scaled to ``snr_db`` against the clean signal (over the whole
    row, or with ``segmental`` over the ``win``-sample windows whose noise level exceeds ``thresh_db``), the mixture to
    ``level_db``, and a row whose peak then exceeds ``clip`` is scaled down to it.  ``snr_db`` / ``level_db``: a number or one per
    row.  Rows are zero from their length on; nothing at or past it is read.

    ``info``: device tensors per row, ``g_clean`` / ``g_noise`` (float64: clean_out = g_clean * clean, noise_out = g_noise * the noise
    as read), the realised ``level_db`` (float64), ``clipped`` and ``active`` (int32: the samples in active windows, the length in
    plain mode).  ``stats``: also the float64 row statistics ``max_c, sum_c2, max_v, sum_v2, act_c2, act_v2, sum_y2, max_y`` and
    ``windows`` [B, ceil(L / win), 6] = max|c|, sum c^2, max|v|, sum v^2, max|y0|, sum y0^2 of every window, y0 the mixture before the
    level step.  Every guard runs on the host before any device work and raises ValueError."""
    _signals(clean, "clean")
    _signals(noise, "noise")
    B, L = clean.shape
    Ln = noise.shape[1]
    if noise.shape[0] != B:
        raise ValueError(f"mix: {noise.shape[0]} noise rows for {B} clean rows")
    target_db, clip, win, thresh_db, segmental = check_mix_args(target_db, clip, win, thresh_db, segmental)
    snr, level = _per_row("snr_db", snr_db, B), _per_row("level_db", level_db, B)
    lens = [L] * B if lengths is None else ops.check_lengths(lengths, B, L, None)
    nlens = [Ln] * B if noise_lengths is None else ops.check_lengths(noise_lengths, B, Ln, None)
    offs = [0] * B if noise_offsets is None else _offsets(noise_offsets, nlens)
    ops.check_dev_f32(clean, "clean")
    ops.check_dev_f32(noise, "noise", clean.device)
    clean, noise = ops._ragged_rows(clean), ops._ragged_rows(noise)
    table = torch.tensor([lens, nlens, offs], dtype=torch.int32).to(clean.device)
    rows = ops.MixRows(clean, None, noise, None, table, B, L, Ln)
    return _mix(rows, snr, level, segmental, target_db, clip, win, thresh_db, stats)


def _offsets(v, nlens: list) -> list:
    """The guards on the cyclic offsets (host only): one integer per row, 0 <= offset < that row's noise length."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda or v.dim() != 1 or v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError("mix: noise_offsets must be a python sequence or a 1-D CPU integer tensor")
        v = v.tolist()
    elif isinstance(v, (str, bytes)) or not isinstance(v, Sequence):
        raise ValueError("mix: noise_offsets must be a python sequence or a 1-D CPU integer tensor")
    if any(isinstance(o, bool) or not isinstance(o, int) for o in v):
        raise ValueError("mix: noise_offsets must be integers (sample counts)")
    if len(v) != len(nlens):
        raise ValueError(f"mix: {len(v)} noise_offsets for a batch of {len(nlens)} rows")
    for b, (o, m) in enumerate(zip(v, nlens)):
        if not 0 <= o < m:
            raise ValueError(f"mix: noise_offsets[{b}] = {o}: 0 <= offset < noise length {m} is expected")
    return list(v)


class SignalPool:
    """Recordings of any lengths, concatenated once into one float32 device buffer: ``data`` (flat), ``offsets`` and ``lengths``
    (python ints: member k is ``data[offsets[k]:offsets[k] + lengths[k]]``).  The mixer reads members, or segments of them, in
    place through a table of offsets; nothing is gathered or padded."""

    def __init__(self, signals, device="cuda"):
        if isinstance(signals, (torch.Tensor, np.ndarray)) or not isinstance(signals, Sequence) or len(signals) == 0:
            raise ValueError("SignalPool: a non-empty list of 1-D float32 signals is expected")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"SignalPool: device {device} is not a GPU; the mixer has no host fallback")
        parts = []
        for k, s in enumerate(signals):
            s = torch.from_numpy(s) if isinstance(s, np.ndarray) else s
            if not isinstance(s, torch.Tensor) or s.dim() != 1 or s.dtype != torch.float32:
                raise ValueError(f"SignalPool: signal {k} must be a 1-D float32 tensor or array")
            if s.shape[0] < 1 or s.shape[0] > MAX_LEN:
                raise ValueError(f"SignalPool: signal {k} has {s.shape[0]} samples; 1 .. 2^27 are supported")
            parts.append(s)
        self.lengths = [int(s.shape[0]) for s in parts]
        self.offsets = [0]
        for n in self.lengths[:-1]:
            self.offsets.append(self.offsets[-1] + n)
        self.data = torch.cat([s.to(device) for s in parts])
        self.device = self.data.device

    def __len__(self):
        return len(self.lengths)

    def member(self, k: int) -> torch.Tensor:
        return self.data[self.offsets[k]:self.offsets[k] + self.lengths[k]]

    def stats(self) -> dict:
        """Per member, device tensors: ``peak`` = max|x|, ``rms`` and ``activity`` (float64), from one pass of the window kernel of
        csrc/assemble.hip over the pool (dataset/assemble.py ``pool_stats``); computed once and kept."""
        if getattr(self, "_stats", None) is None:
            from .assemble import pool_stats
            self._stats = pool_stats(self)
        return self._stats

    def usable(self, clip: float = 0.99) -> list:
        """The python list of the members with ``peak <= clip``: the recordings no sample of which clips.  One synchronisation per
        pool and threshold, not per batch; ValueError where no member is left."""
        clip = _finite("clip", clip, "usable")
        kept = self.__dict__.setdefault("_usable", {})
        if clip not in kept:
            from .assemble import usable_members
            kept[clip] = usable_members(self, clip)
        return list(kept[clip])


class Draw(NamedTuple):
    """Batch k as :func:`draw_batch` names it, one entry per row."""
    clean_id: list          # the clean recording
    clean_start: list       # the first sample of the segment in it
    lens: list              # the segment's length: ``samples``, or the whole of a shorter recording
    noise_id: list          # the noise recording
    noise_offset: list      # the cyclic offset into it
    snr_db: list
    level_db: list


def _range(name, r):
    if isinstance(r, (str, bytes)) or not isinstance(r, Sequence) or len(r) != 2:
        raise ValueError(f"draw_batch: {name} = {r!r}: a (low, high) pair is expected")
    lo, hi = _finite(f"{name}[0]", r[0], "draw_batch"), _finite(f"{name}[1]", r[1], "draw_batch")
    if not lo < hi:
        raise ValueError(f"draw_batch: {name} = {r!r}: low < high is expected")
    return lo, hi


def draw_batch(k: int, seed: int, clean_lengths: Sequence[int], noise_lengths: Sequence[int], batch: int, samples: int,
               snr_db=(-5.0, 20.0), level_db=(-35, -15)) -> Draw:
    """The rows and parameters of batch ``k``: host only, a function of ``(seed, k)`` and the arguments alone (no state, so any
    batch can be drawn without the ones before it).  Per row, in this order: a clean recording; where it is longer than ``samples``
    the start of its ``samples``-long segment (a shorter one gives its whole length); a noise recording; its cyclic offset; an SNR
    uniform in ``snr_db = (low, high)``; an integer level in ``[low, high)`` of ``level_db``."""
    for name, v in (("k", k), ("seed", seed), ("batch", batch), ("samples", samples)):
        if isinstance(v, bool) or not isinstance(v, int) or v < (1 if name in ("batch", "samples") else 0):
            raise ValueError(f"draw_batch: {name} = {v!r}: a {'positive' if name in ('batch', 'samples') else 'non-negative'} integer is expected")
    for name, lens in (("clean_lengths", clean_lengths), ("noise_lengths", noise_lengths)):
        if len(lens) == 0 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in lens):
            raise ValueError(f"draw_batch: {name} must be a non-empty sequence of positive integers")
    snr_lo, snr_hi = _range("snr_db", snr_db)
    lev_lo, lev_hi = _range("level_db", level_db)
    if lev_lo != int(lev_lo) or lev_hi != int(lev_hi):
        raise ValueError(f"draw_batch: level_db = {level_db!r}: integer bounds are expected")
    rng = random.Random(f"mix:{seed}:{k}")
    d = Draw([], [], [], [], [], [], [])
    for _ in range(batch):
        ci = rng.randrange(len(clean_lengths))
        n = clean_lengths[ci]
        d.clean_id.append(ci)
        d.clean_start.append(rng.randrange(n - samples + 1) if n > samples else 0)
        d.lens.append(min(n, samples))
        ni = rng.randrange(len(noise_lengths))
        d.noise_id.append(ni)
        d.noise_offset.append(rng.randrange(noise_lengths[ni]))
        d.snr_db.append(rng.uniform(snr_lo, snr_hi))
        d.level_db.append(float(rng.randrange(int(lev_lo), int(lev_hi))))
    return d


def mix_draw(clean_pool: SignalPool, noise_pool: SignalPool, draw: Draw, samples: int, segmental: bool = False, target_db: float = -25.0,
             clip: float = 0.99, win: int = 1600, thresh_db: float = -50.0, stats: bool = False, clean: Optional[torch.Tensor] = None,
             noise: Optional[torch.Tensor] = None):
    """The rows a :class:`Draw` names, read in place from the two pools through device tables of offsets (no gather copy) and mixed as
    by :func:`snr_mix` -> ``(noisy, clean_out, noise_out, info)``, the signals float32 [rows, samples].  ``clean``: a float32
    [rows, samples] tensor on the pools' device whose row b, its first ``draw.lens[b]`` samples, stands in for the clean segment the
    draw names (the segment after reverberation, say); the noise rows are still read in place.  ``noise``: a float32 [rows, samples]
    tensor whose row b, read from offset 0 with length ``samples``, stands in for the noise recording and offset the draw names (an
    assembled noise clip, say).  The guards run on the host."""
    if not isinstance(clean_pool, SignalPool) or not isinstance(noise_pool, SignalPool):
        raise ValueError("mix: clean_pool and noise_pool must be SignalPool objects")
    if clean_pool.device != noise_pool.device:
        raise ValueError(f"mix: the pools are on {clean_pool.device} and {noise_pool.device}")
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1 or samples > MAX_LEN:
        raise ValueError(f"mix: samples = {samples!r}; 1 .. 2^27 are supported")
    target_db, clip, win, thresh_db, segmental = check_mix_args(target_db, clip, win, thresh_db, segmental)
    B = len(draw.lens)
    if B < 1 or B > 65535 or any(len(f) != B for f in draw):
        raise ValueError(f"mix: a draw of {B} rows; 1 .. 65535, every field of the same length, are supported")
    snr, level = _per_row("snr_db", draw.snr_db, B), _per_row("level_db", draw.level_db, B)
    for b in range(B):
        ci, s0, n, ni, o = draw.clean_id[b], draw.clean_start[b], draw.lens[b], draw.noise_id[b], draw.noise_offset[b]
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (ci, s0, n, ni, o)):
            raise ValueError(f"mix: row {b} of the draw does not hold integers")
        if not (0 <= ci < len(clean_pool) and 0 <= ni < len(noise_pool)):
            raise ValueError(f"mix: row {b} of the draw names recording {ci} / {ni}; the pools hold {len(clean_pool)} / {len(noise_pool)}")
        if not (1 <= n <= samples and 0 <= s0 and s0 + n <= clean_pool.lengths[ci]):
            raise ValueError(f"mix: row {b} of the draw: samples [{s0}, {s0 + n}) of a recording of {clean_pool.lengths[ci]}, at most {samples}")
        if not 0 <= o < noise_pool.lengths[ni]:
            raise ValueError(f"mix: row {b} of the draw: 0 <= offset {o} < noise length {noise_pool.lengths[ni]} is expected")
    dev = clean_pool.device
    if clean is not None:
        _signals(clean, "clean")
        if tuple(clean.shape) != (B, samples):
            raise ValueError(f"mix: clean is {tuple(clean.shape)}; [{B}, {samples}], a row of `samples` for every row of the draw with "
                             "draw.lens[b] samples in it, is expected")
        ops.check_dev_f32(clean, "clean", dev)
    if noise is not None:
        _signals(noise, "noise")
        if tuple(noise.shape) != (B, samples):
            raise ValueError(f"mix: noise is {tuple(noise.shape)}; [{B}, {samples}], a row of `samples` for every row of the draw, is expected")
        ops.check_dev_f32(noise, "noise", dev)
        clean_off = None if clean is not None else torch.tensor([clean_pool.offsets[c] + s for c, s in zip(draw.clean_id, draw.clean_start)],
                                                                dtype=torch.int64).to(dev)
        table = torch.tensor([draw.lens, [samples] * B, [0] * B], dtype=torch.int32).to(dev)
        rows = ops.MixRows(clean_pool.data if clean is None else ops._ragged_rows(clean), clean_off, ops._ragged_rows(noise), None, table, B,
                           samples, samples)
        with torch.cuda.device(dev):
            return _mix(rows, snr, level, segmental, target_db, clip, win, thresh_db, stats)
    off = torch.tensor([[clean_pool.offsets[c] + s for c, s in zip(draw.clean_id, draw.clean_start)],
                        [noise_pool.offsets[j] for j in draw.noise_id]], dtype=torch.int64).to(dev)
    table = torch.tensor([draw.lens, [noise_pool.lengths[j] for j in draw.noise_id], draw.noise_offset], dtype=torch.int32).to(dev)
    if clean is None:
        rows = ops.MixRows(clean_pool.data, off[0], noise_pool.data, off[1], table, B, samples, max(noise_pool.lengths))
    else:
        rows = ops.MixRows(ops._ragged_rows(clean), None, noise_pool.data, off[1], table, B, samples, max(noise_pool.lengths))
    with torch.cuda.device(dev):                            # the kernels are queued on the current device's stream
        return _mix(rows, snr, level, segmental, target_db, clip, win, thresh_db, stats)


class DynamicMixtures:
    """``(noisy, clean, noise)`` float32 [batch, samples] on the device, the order and shapes of ``dataload.SyntheticMixtures`` and of
    the NSVAE loader, with a fresh pairing, segment, SNR and level for every row of every batch: batch k is what :func:`draw_batch`
    names for ``(seed, k)``, read in place from the two pools (no gather copy) and mixed by the kernels of :func:`snr_mix`.  A clean
    recording shorter than ``samples`` comes back zero-padded.  ``length``: the number of batches of one iteration (None: endless).

    ``rir_pool``: a ``dataset.reverb.RirPool``.  Row b of batch k is then convolved with the impulse response that
    ``draw_reverb(k, seed, len(rir_pool), batch, p_reverb)`` names (-1: the row stays dry), with the samples in front of its segment,
    and mixed as the reverberant clean signal, as the DNS-Challenge synthesizer does; ``clean`` is the scaled reverberant speech.
    ``target="early"``: ``clean`` is float32(g_clean x the row convolved with ``rir_pool.early_taps(early_ms)`` taps only), the
    direct sound and early reflections at the gain of the mixture.  Without a pool nothing changes.

    ``clips=True`` (dataset/assemble.py): the clean and the noise row of every mixture are CLIPS, several recordings of
    the pool's usable members (``SignalPool.usable(clip)``: no sample above ``clip``) laid end to end with ``gap`` samples of pause
    until the row is full, as ``draw_clips(k, seed, ..., stream="clean" / "noise")`` names them; of the ``tries`` candidates of a row
    the device takes the first whose share of active 50 ms windows (at ``fs``) exceeds ``clean_activity`` / ``noise_activity``, or
    the most active one.  A short recording then no longer leaves a zero tail and a mixture holds several noise sources in a row.
    With a ``rir_pool`` the rows ``draw_reverb`` names are convolved whole (the history in front of a clip is zero); SNR and level
    are those of ``draw_batch(k)``.  With ``clips=False`` none of this runs."""

    def __init__(self, clean_pool: SignalPool, noise_pool: SignalPool, batch: int, samples: int = 64000, seed: int = 123,
                 length: Optional[int] = None, segmental: bool = False, snr_db=(-5.0, 20.0), level_db=(-35, -15),
                 target_db: float = -25.0, clip: float = 0.99, win: int = 1600, thresh_db: float = -50.0, rir_pool=None,
                 p_reverb: float = 0.5, target: str = "reverberant", early_ms: float = 50.0, clips: bool = False, tries: int = 4,
                 gap: int = 3200, clean_activity: float = 0.6, noise_activity: float = 0.0, fs: int = 16000):
        if isinstance(p_reverb, bool) or not isinstance(p_reverb, (int, float)) or not 0.0 <= p_reverb <= 1.0:
            raise ValueError(f"DynamicMixtures: p_reverb = {p_reverb!r}: a probability in [0, 1] is expected")
        if target not in ("reverberant", "early"):
            raise ValueError(f"DynamicMixtures: target = {target!r}: 'reverberant' or 'early' is expected")
        self.early_ms = _finite("early_ms", early_ms, "DynamicMixtures")
        if self.early_ms < 0:
            raise ValueError(f"DynamicMixtures: early_ms = {early_ms!r}: a finite number >= 0 is expected")
        if rir_pool is not None:
            from .reverb import RirPool
            if not isinstance(rir_pool, RirPool):
                raise ValueError("DynamicMixtures: rir_pool must be a RirPool object (or None)")
        if not isinstance(clean_pool, SignalPool) or not isinstance(noise_pool, SignalPool):
            raise ValueError("DynamicMixtures: clean_pool and noise_pool must be SignalPool objects")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1 or batch > 65535:
            raise ValueError(f"DynamicMixtures: batch = {batch!r}; 1 .. 65535 rows are supported")
        if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1 or samples > MAX_LEN:
            raise ValueError(f"DynamicMixtures: samples = {samples!r}; 1 .. 2^27 are supported")
        self.mix_args = check_mix_args(target_db, clip, win, thresh_db, segmental)
        draw_batch(0, seed, clean_pool.lengths, noise_pool.lengths, 1, samples, snr_db, level_db)      # the guards on the ranges
        self.clean_pool, self.noise_pool, self.batch_size, self.samples = clean_pool, noise_pool, batch, samples
        self.seed, self.length, self.snr_db, self.level_db = seed, length, snr_db, level_db
        if rir_pool is not None and rir_pool.device != clean_pool.device:
            raise ValueError(f"DynamicMixtures: the pools are on {clean_pool.device} and rir_pool on {rir_pool.device}")
        self.rir_pool, self.p_reverb, self.target = rir_pool, float(p_reverb), target
        if not isinstance(clips, bool):
            raise ValueError(f"DynamicMixtures: clips = {clips!r}: True or False is expected")
        self.clips = clips
        if clips:
            from . import assemble as AS
            AS.window_of(fs, "DynamicMixtures")
            self.gate = (_finite("clean_activity", clean_activity, "DynamicMixtures"), _finite("noise_activity", noise_activity, "DynamicMixtures"))
            self.tries, self.gap, self.fs = tries, gap, fs
            AS.draw_clips(0, seed, clean_pool.lengths, 1, samples, tries, gap)              # the guards on tries and gap
            if batch * tries > AS.MAX_ROWS:
                raise ValueError(f"DynamicMixtures: batch x tries = {batch * tries}; at most {AS.MAX_ROWS} candidate rows are supported")
            self.usable = (clean_pool.usable(self.mix_args[1]), noise_pool.usable(self.mix_args[1]))      # one synchronisation per pool

    def draw(self, k: int) -> Draw:
        return draw_batch(k, self.seed, self.clean_pool.lengths, self.noise_pool.lengths, self.batch_size, self.samples, self.snr_db,
                          self.level_db)

    def batch(self, k: int, info: bool = False, stats: bool = False):
        """Batch k -> (noisy, clean, noise), with ``info`` also the dict of :func:`snr_mix` and, with a ``rir_pool``, ``rir_id``: the
        python list of ``draw_reverb``; with ``clips=True`` also ``clean_clips`` / ``noise_clips`` (the :class:`~.assemble.Clips`),
        ``clean_chosen`` / ``noise_chosen`` and ``clean_accepted`` / ``noise_accepted`` (int32 on the device)."""
        target_db, clip, win, thresh_db, segmental = self.mix_args
        if self.clips:
            out = self._clip_batch(k, stats)
            return out if info else out[:3]
        if self.rir_pool is None:
            out = mix_draw(self.clean_pool, self.noise_pool, self.draw(k), self.samples, segmental, target_db, clip, win, thresh_db, stats)
            return out if info else out[:3]
        from . import reverb as RV
        d = self.draw(k)
        ids = RV.draw_reverb(k, self.seed, len(self.rir_pool), self.batch_size, self.p_reverb)
        wet = RV.reverb_draw(self.clean_pool, self.rir_pool, d, ids, self.samples)
        noisy, clean, noise, inf = mix_draw(self.clean_pool, self.noise_pool, d, self.samples, segmental, target_db, clip, win, thresh_db, stats,
                                            clean=wet)
        if self.target == "early":
            early = RV.reverb_draw(self.clean_pool, self.rir_pool, d, ids, self.samples, taps=self.rir_pool.early_taps(self.early_ms))
            clean = (inf["g_clean"][:, None] * early.double()).float()
        inf["rir_id"] = ids
        return (noisy, clean, noise, inf) if info else (noisy, clean, noise)

    def _clip_batch(self, k: int, stats: bool):
        from . import assemble as AS
        target_db, clip, win, thresh_db, segmental = self.mix_args
        d = self.draw(k)                                       # the SNR and the level of every row
        extra, rows = {}, []
        for name, pool, ids, gate in zip(("clean", "noise"), (self.clean_pool, self.noise_pool), self.usable, self.gate):
            c = AS.draw_clips(k, self.seed, pool.lengths, self.batch_size, self.samples, self.tries, self.gap, ids, name)
            r, a = AS.assemble(pool, c, self.samples, gate, self.fs)
            rows.append(r)
            extra.update({f"{name}_clips": c, f"{name}_chosen": a["chosen"], f"{name}_accepted": a["accepted"]})
        speech, early = rows[0], None
        if self.rir_pool is not None:
            from . import reverb as RV
            extra["rir_id"] = RV.draw_reverb(k, self.seed, len(self.rir_pool), self.batch_size, self.p_reverb)
            speech = RV.reverb_rows(rows[0], self.rir_pool, extra["rir_id"])
            if self.target == "early":
                early = RV.reverb_rows(rows[0], self.rir_pool, extra["rir_id"], taps=self.rir_pool.early_taps(self.early_ms))
        noisy, clean, noise, inf = snr_mix(speech, rows[1], d.snr_db, d.level_db, segmental=segmental, target_db=target_db, clip=clip,
                                           win=win, thresh_db=thresh_db, stats=stats)
        if early is not None:
            clean = (inf["g_clean"][:, None] * early.double()).float()
        inf.update(extra)
        return noisy, clean, noise, inf

    def __iter__(self):
        k = 0
        while self.length is None or k < self.length:
            yield self.batch(k)
            k += 1
