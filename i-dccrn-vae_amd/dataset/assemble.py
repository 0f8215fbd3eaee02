"""Clip assembly on the device (csrc/assemble.hip): the step of the DNS-Challenge synthesizer that builds every clean and
noise clip of a mixture from several recordings and gates it on its content.

  * :func:`activity`  the share of active 50 ms windows of every row of a padded batch (``activitydetector``);
  * :func:`pool_stats`  peak, rms and activity of every member of a :class:`~.mix.SignalPool` (``SignalPool.stats()`` / ``usable()``);
  * :func:`draw_clips`  names, on the host, ``tries`` candidate rows for every row of training batch k: recordings laid end to end
    with pauses between them until the row is full (``build_audio``); a function of ``(seed, k, stream)`` alone;
  * :func:`assemble`  measures every candidate on the device, takes for each row the first one that is active enough (the most active
    one if none is) and writes it; nothing returns to the host.

The definition is restated in float64 in tests/assemble_ref.py (parity with the synthesizer package is unpinned: it is not installed
where this was written), with two deliberate differences: a bounded number of candidates, chosen on the device, instead of a host
loop that draws until one passes; clipped recordings excluded once per pool instead of per draw.  There is no host fallback.
"""
from __future__ import annotations

import random
from typing import NamedTuple, Optional, Sequence

import torch

from .. import ops
from .mix import MAX_LEN, SignalPool, _finite

MAX_PIECES = ops.ASM_MAX_PIECES
MAX_TRIES = ops.ASM_MAX_TRIES
MAX_ROWS = ops.ASM_MAX_ROWS


class Clips(NamedTuple):
    """The candidate rows of a batch as :func:`draw_clips` names them, python lists throughout.  Piece i copies ``length[i]`` samples
    from sample ``start[i]`` of pool member ``member[i]`` to position ``dst[i]`` of its row; candidate ``r = b * tries + t`` (candidate
    t of row b) owns the pieces ``first[r] .. first[r] + count[r] - 1``, sorted by ``dst`` and disjoint; what no piece covers is a
    pause."""
    member: list
    start: list
    length: list
    dst: list
    first: list
    count: list
    tries: int

    def pieces(self, b: int, t: int) -> list:
        """Candidate t of row b as (member, start, length, dst) tuples."""
        r = b * self.tries + t
        return [(self.member[i], self.start[i], self.length[i], self.dst[i]) for i in range(self.first[r], self.first[r] + self.count[r])]

    def candidates(self) -> list:
        """[b][t] -> :meth:`pieces`."""
        return [[self.pieces(b, t) for t in range(self.tries)] for b in range(len(self.first) // self.tries)]


def _int(name: str, v, lo: int, hi: Optional[int], who: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{who}: {name} = {v!r}: an integer {'>= ' + str(lo) if hi is None else 'in ' + str(lo) + ' .. ' + str(hi)} is expected")
    return v


def window_of(fs, who: str = "activity") -> int:
    """The 50 ms window of sampling rate ``fs`` in samples.  The kernel reads a row in quads of 4 samples that start at the window's
    first sample, so a window must be a whole number of samples and a multiple of 4: ``fs`` must be a multiple of 80."""
    _int("fs", fs, 1, None, who)
    if fs % 80:
        why = ("50 ms are no whole number of samples" if fs % 20 else
               f"its 50 ms window of {fs // 20} samples is no multiple of 4, and the kernel reads a window in quads of 4 samples that start on its first sample")
        raise ValueError(f"{who}: fs = {fs}: {why}; a multiple of 80 Hz is expected (8000, 16000, 24000, 32000, 48000)")
    win = fs // 20
    if win > MAX_LEN:
        raise ValueError(f"{who}: fs = {fs}: a window of {win} samples; at most 2^27 are supported")
    return win


def _gate_args(fs, energy_thresh, target_db, who: str) -> tuple:
    return window_of(fs, who), _finite("energy_thresh", energy_thresh, who), _finite("target_db", target_db, who)


def draw_clips(k: int, seed: int, lengths: Sequence[int], batch: int, samples: int, tries: int = 4, gap: int = 3200,
               usable: Optional[Sequence[int]] = None, stream: str = "clean") -> Clips:
    """``tries`` candidate rows for each of the ``batch`` rows of batch ``k``: host only, a function of its arguments alone, from a
    generator of its own (what ``draw_batch`` and ``draw_reverb`` return does not change).  Per candidate, recordings are drawn from
    ``usable`` (member indices; default: all) and laid end to end with ``gap`` samples of pause between them until the row holds
    ``samples`` samples; a recording longer than what remains gives a segment of exactly the remaining length, at a drawn start; a
    candidate that is still not full after 64 pieces ends there."""
    who = "draw_clips"
    _int("k", k, 0, None, who), _int("seed", seed, 0, None, who)
    _int("batch", batch, 1, 65535, who), _int("samples", samples, 1, MAX_LEN, who)
    _int("tries", tries, 1, MAX_TRIES, who), _int("gap", gap, 0, None, who)
    if not isinstance(stream, str):
        raise ValueError(f"draw_clips: stream = {stream!r}: a string is expected")
    if isinstance(lengths, (str, bytes)) or not isinstance(lengths, Sequence) or len(lengths) == 0 or any(
            isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in lengths):
        raise ValueError("draw_clips: lengths must be a non-empty sequence of positive integers")
    if usable is None:
        ids = list(range(len(lengths)))
    else:
        if isinstance(usable, (str, bytes)) or not isinstance(usable, Sequence):
            raise ValueError("draw_clips: usable must be a sequence of member indices")
        ids = list(usable)
        if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < len(lengths) for v in ids):
            raise ValueError(f"draw_clips: usable must hold member indices below {len(lengths)}")
        if not ids:
            raise ValueError("draw_clips: the pool has no usable member")
    rng = random.Random(f"clips:{stream}:{seed}:{k}")
    c = Clips([], [], [], [], [], [], tries)
    for _ in range(batch * tries):
        c.first.append(len(c.member))
        pos = cnt = 0
        while pos < samples and cnt < MAX_PIECES:
            m = ids[rng.randrange(len(ids))]
            n, rem = lengths[m], samples - pos
            s0, n = (rng.randrange(n - rem + 1), rem) if n > rem else (0, n)
            c.member.append(m), c.start.append(s0), c.length.append(n), c.dst.append(pos)
            pos += n + gap
            cnt += 1
        c.count.append(cnt)
    return c


def check_clips(clips: Clips, lengths: Sequence[int], samples: int) -> int:
    """The guards on a :class:`Clips` (host only, no device use) against the member ``lengths`` of its pool -> the number of rows B."""
    if not isinstance(clips, Clips):
        raise ValueError("assemble: clips must be a Clips object")
    _int("samples", samples, 1, MAX_LEN, "assemble")
    _int("clips.tries", clips.tries, 1, MAX_TRIES, "assemble")
    for name in ("member", "start", "length", "dst", "first", "count"):
        v = getattr(clips, name)
        if not isinstance(v, list) or any(isinstance(x, bool) or not isinstance(x, int) for x in v):
            raise ValueError(f"assemble: clips.{name} must be a python list of integers")
    P, R = len(clips.member), len(clips.first)
    if not (len(clips.start) == len(clips.length) == len(clips.dst) == P) or len(clips.count) != R:
        raise ValueError(f"assemble: clips holds {P} / {len(clips.start)} / {len(clips.length)} / {len(clips.dst)} piece entries and "
                         f"{R} / {len(clips.count)} candidate entries; equal lengths are expected")
    if P < 1 or R < 1 or R % clips.tries or R > MAX_ROWS:
        raise ValueError(f"assemble: {P} pieces in {R} candidate rows of {clips.tries} tries; at least one piece and 1 .. {MAX_ROWS} "
                         "candidate rows, a multiple of tries, are supported")
    for r in range(R):
        f, c = clips.first[r], clips.count[r]
        if not (0 <= c <= MAX_PIECES and 0 <= f and f + c <= P):
            raise ValueError(f"assemble: candidate {r} names pieces [{f}, {f + c}) of {P}; at most {MAX_PIECES} per candidate")
        end = 0
        for i in range(f, f + c):
            m, s, n, d = clips.member[i], clips.start[i], clips.length[i], clips.dst[i]
            if not 0 <= m < len(lengths):
                raise ValueError(f"assemble: piece {i} names member {m}; the pool holds {len(lengths)}")
            if not (n >= 1 and s >= 0 and s + n <= lengths[m]):
                raise ValueError(f"assemble: piece {i}: samples [{s}, {s + n}) of a member of {lengths[m]}")
            if d < end:
                raise ValueError(f"assemble: piece {i} of candidate {r} starts at {d}, before the end {end} of the piece in front of it: "
                                 "pieces sorted by dst that do not overlap are expected")
            if d + n > samples:
                raise ValueError(f"assemble: piece {i} of candidate {r} covers [{d}, {d + n}) of a row of {samples}")
            end = d + n
    return R // clips.tries


def assemble(pool: SignalPool, clips: Clips, samples: int, min_activity: float = 0.0, fs: int = 16000, energy_thresh: float = 0.13,
             target_db: float = -25.0, stats: bool = False):
    """The rows a :class:`Clips` names, read in place from ``pool`` -> ``(rows, info)``: ``rows`` float32 [B, samples] on the device,
    row b the first of its ``tries`` candidates whose :func:`activity` exceeds ``min_activity`` or, when none does, the one with the
    most active windows (the lowest index on a tie).  ``info`` (device tensors): ``chosen`` int32 [B], ``accepted`` int32 [B] (0 where
    no candidate passed), ``activity`` float64 [B, tries]; ``stats``: also ``active`` / ``windows`` int32 [B, tries], ``peak`` /
    ``sum2`` float64 [B, tries] and ``window_stats`` float64 [B, tries, ceil(samples / win), 2] = max|x|, sum x^2 of every window.  The
    tables go up in one copy, three kernels follow, nothing returns to the host.  The guards run on the host before any device work."""
    if not isinstance(pool, SignalPool):
        raise ValueError("assemble: pool must be a SignalPool object")
    B = check_clips(clips, pool.lengths, samples)
    min_activity = _finite("min_activity", min_activity, "assemble")
    win, energy_thresh, target_db = _gate_args(fs, energy_thresh, target_db, "assemble")
    if not pool.data.is_cuda:
        raise ValueError(f"assemble: the pool is on {pool.data.device}; a GPU is expected, there is no host fallback")
    T = clips.tries
    src = [pool.offsets[m] + s for m, s in zip(clips.member, clips.start)]
    with torch.cuda.device(pool.device):
        tab = ops.asm_tables(pool.data, src, clips.length, clips.dst, clips.first, clips.count, B, T, samples)
        a = ops.asm_activity(tab, None, win, target_db, energy_thresh, min_activity)
        rows = ops.asm_write(tab, a["chosen"])
    info = {"chosen": a["chosen"], "accepted": a["accepted"], "activity": a["activity"].view(B, T)}
    if stats:
        info.update(active=a["active"].view(B, T), windows=a["windows"].view(B, T), peak=a["rowstat"][:, 0].reshape(B, T),
                    sum2=a["rowstat"][:, 1].reshape(B, T), window_stats=a["window_stats"].view(B, T, -1, 2).clone())
    return rows, info


def _row_activity(x: torch.Tensor, offsets: list, lens: list, win: int, energy_thresh: float, target_db: float) -> dict:
    """One single-piece candidate per row (``lens[r]`` samples at ``x.flatten()[offsets[r]]``), at most MAX_ROWS per launch."""
    out = []
    with torch.cuda.device(x.device):
        for r0 in range(0, len(lens), MAX_ROWS):
            n = lens[r0:r0 + MAX_ROWS]
            R = len(n)
            tab = ops.asm_tables(x, offsets[r0:r0 + R], n, [0] * R, list(range(R)), [1] * R, R, 1, max(n))
            rowlen = tab.len                                  # a row is as long as its one piece
            a = ops.asm_activity(tab, rowlen, win, target_db, energy_thresh, 0.0)
            out.append({k: a[k] for k in ("rowstat", "active", "windows", "activity")})
    return out[0] if len(out) == 1 else {k: torch.cat([o[k] for o in out]) for k in out[0]}


def activity(x: torch.Tensor, lengths=None, fs: int = 16000, energy_thresh: float = 0.13, target_db: float = -25.0, stats: bool = False):
    """``x`` [B, L] float32 on the GPU -> float64 [B] on the device: the share of the 50 ms windows of row b, judged over its own
    ``lengths[b]`` samples (default L; the last window may be short), that the synthesizer's ``activitydetector`` calls active.
    Nothing at or past a row's length is read, and a row's value does not depend on the batch around it.  ``stats``: ``(activity,
    active, windows)``, the two counts int32 [B].  The guards run on the host before any device work."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("activity: x must be a [B, L] tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"activity: x is {x.dtype}; float32 samples are expected")
    B, L = x.shape
    if B < 1 or L < 1 or L > MAX_LEN:
        raise ValueError(f"activity: a batch of {B} rows of {L} samples; at least one row of 1 .. 2^27 samples is supported")
    win, energy_thresh, target_db = _gate_args(fs, energy_thresh, target_db, "activity")
    lens = [L] * B if lengths is None else ops.check_lengths(lengths, B, L, None)
    if not x.is_cuda:
        raise ValueError(f"activity: x is on {x.device}; a GPU tensor is expected, there is no host fallback")
    x = ops._ragged_rows(x)
    pitch = x.stride(0)
    flat = torch.as_strided(x, ((B - 1) * pitch + L,), (1,))              # the rows in place, whatever the pitch
    a = _row_activity(flat, [b * pitch for b in range(B)], lens, win, energy_thresh, target_db)
    return (a["activity"], a["active"], a["windows"]) if stats else a["activity"]


def pool_stats(pool: SignalPool, fs: int = 16000, energy_thresh: float = 0.13, target_db: float = -25.0) -> dict:
    """Per member of ``pool``, on the device: ``peak`` = max|x| and ``rms`` (float64), ``activity`` (float64) as :func:`activity`
    judges the whole member."""
    if not isinstance(pool, SignalPool):
        raise ValueError("pool_stats: pool must be a SignalPool object")
    win, energy_thresh, target_db = _gate_args(fs, energy_thresh, target_db, "pool_stats")
    a = _row_activity(pool.data, pool.offsets, pool.lengths, win, energy_thresh, target_db)
    n = torch.tensor(pool.lengths, dtype=torch.float64).to(pool.device)
    return {"peak": a["rowstat"][:, 0].clone(), "rms": torch.sqrt(a["rowstat"][:, 1] / n), "activity": a["activity"]}


def usable_members(pool: SignalPool, clip: float = 0.99) -> list:
    """The members of ``pool`` whose peak does not exceed ``clip`` (one synchronisation per pool); ValueError where there is none."""
    clip = _finite("clip", clip, "usable")
    if not 0.0 < clip <= 1.0:
        raise ValueError(f"usable: clip = {clip!r}: a threshold in (0, 1] is expected")
    ok = [k for k, pk in enumerate(pool.stats()["peak"].tolist()) if pk <= clip]
    if not ok:
        raise ValueError(f"usable: the pool has no usable member: every one of its {len(pool)} recordings peaks above {clip}")
    return ok
