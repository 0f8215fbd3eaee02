"""Room impulse responses of rectangular rooms on the device (csrc/ism.hip): the image-source method of Allen & Berkley
(1979), the producer of the simulated responses that the DNS-Challenge synthesizer convolves its clean speech with.

  * :func:`shoebox_rir`  a batch of rooms -> one impulse response per room, float32 on the GPU;
  * :func:`beta_from_t60`  Sabine's wall coefficient for a wished reverberation time (host);
  * :func:`draw_rooms`  names the rooms of pool k on the host, a function of ``(seed, k)`` alone;
  * :meth:`~.reverb.RirPool.shoebox` (dataset/reverb.py) builds a pool from the device rows.

The definition is tests/ism_ref.py: every image with a delay below ``taps - 1 + 40.5`` samples enters through a Hann-windowed sinc of
81 samples, summed in double; parity with pyroomacoustics, gpuRIR or torchaudio is unpinned.  No high-pass filter and no air absorption
are applied; microphone directivity, frequency-dependent walls and rooms that are not rectangular are out of scope.  There is no host
fallback.
"""
from __future__ import annotations

import math
import random
from typing import NamedTuple, Sequence

import numpy as np
import torch

from .. import ops
from .reverb import MAX_TAPS, _counts, _int

WINDOW = 81                    # samples of the windowed sinc of every image


class Rooms(NamedTuple):
    """What :func:`draw_rooms` names: the arguments of :func:`shoebox_rir`, one row per room, and the ``t60`` drawn for each."""
    room: np.ndarray           # float64 [n, 3]
    source: np.ndarray         # float64 [n, 3]
    mic: np.ndarray            # float64 [n, 3]
    beta: np.ndarray           # float64 [n, 6]: (x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz)
    t60: np.ndarray            # float64 [n]


def _host_rows(name: str, v, cols: int, who: str) -> np.ndarray:
    """A python sequence, numpy array or CPU tensor [B, cols] (or [cols]: one room) of finite numbers -> float64 [B, cols]."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise ValueError(f"{who}: {name} is on {v.device}; the geometry is checked on the host: a python sequence, a numpy array "
                             "or a CPU tensor is expected")
        v = v.detach().numpy()
    try:
        a = np.array(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must hold numbers, [B, {cols}]") from None
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != cols or a.shape[0] < 1:
        raise ValueError(f"{who}: {name} has shape {tuple(a.shape)}; [B, {cols}] is expected")
    if not np.isfinite(a).all():
        raise ValueError(f"{who}: {name} holds a value that is not finite")
    return a


def _positive(name: str, v, who: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
        raise ValueError(f"{who}: {name} = {v!r}: a finite number > 0 is expected")
    return float(v)


def check_rooms(room, source, mic, beta, taps, fs=16000, c=343.0, max_order=None, max_images=2 ** 28, who="shoebox_rir"):
    """Every host guard of :func:`shoebox_rir` -> (geom float64 [B, ops.ISM_FIELDS], taps list, max_order list or None).  Touches
    no device."""
    L = _host_rows("room", room, 3, who)
    B = L.shape[0]
    s, r, bt = _host_rows("source", source, 3, who), _host_rows("mic", mic, 3, who), _host_rows("beta", beta, 6, who)
    for name, a in (("source", s), ("mic", r), ("beta", bt)):
        if a.shape[0] != B:
            raise ValueError(f"{who}: {a.shape[0]} rows of {name} for {B} rooms")
    if B > 65535:
        raise ValueError(f"{who}: a batch of {B} rooms; 1 .. 65535 are supported")
    fs, c = _positive("fs", fs, who), _positive("c", c, who)
    _int("max_images", max_images, 1, who)
    tp = _counts("taps", taps, B, [MAX_TAPS] * B, who)
    mo = None
    if max_order is not None:
        mo = [max_order] * B if isinstance(max_order, int) and not isinstance(max_order, bool) else max_order
        if isinstance(mo, (torch.Tensor, np.ndarray)):
            if isinstance(mo, torch.Tensor) and mo.is_cuda:
                raise ValueError(f"{who}: max_order must be an integer, a python sequence or a CPU tensor")
            mo = mo.tolist()
        if isinstance(mo, (str, bytes)) or not isinstance(mo, Sequence) or len(mo) != B:
            raise ValueError(f"{who}: max_order must be an integer or one per room")
        if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31 for v in mo):
            raise ValueError(f"{who}: max_order must be integers >= 0")
        mo = list(mo)
    if (L <= 0).any():
        raise ValueError(f"{who}: room {int(np.argmax((L <= 0).any(axis=1)))} has a size that is not positive")
    for name, a in (("source", s), ("mic", r)):
        out = ((a <= 0) | (a >= L)).any(axis=1)
        if out.any():
            raise ValueError(f"{who}: the {name} of room {int(np.argmax(out))} is not strictly inside the room")
    if (np.abs(bt) > 1).any():
        raise ValueError(f"{who}: room {int(np.argmax((np.abs(bt) > 1).any(axis=1)))} has a reflection coefficient outside [-1, 1]")
    dist = np.sqrt(((s - r) ** 2).sum(axis=1))
    if (dist < c / fs).any():
        b = int(np.argmax(dist < c / fs))
        raise ValueError(f"{who}: source and microphone of room {b} are {dist[b]:.4g} m apart; at least c / fs = {c / fs:.4g} m (one "
                         "sample) is expected: 1 / (4 pi d) is unbounded below it")
    dmax = (np.array(tp, dtype=np.float64) - 1 + WINDOW / 2) * c / fs
    est = 4.0 / 3.0 * math.pi * dmax ** 3 / L.prod(axis=1)
    if (est > max_images).any():
        b = int(np.argmax(est > max_images))
        raise ValueError(f"{who}: room {b} of {L[b].prod():.4g} m^3 has about {est[b]:.3g} images within {tp[b]} taps; max_images = "
                         f"{max_images}")
    geom = np.empty((B, ops.ISM_FIELDS), dtype=np.float64)
    geom[:, 0:3], geom[:, 3:6], geom[:, 6:9] = L, s, r
    geom[:, ops.ISM_FIELD["beta"]:ops.ISM_FIELD["beta"] + 6] = bt
    geom[:, ops.ISM_FIELD["fs"]], geom[:, ops.ISM_FIELD["c"]] = fs, c
    return geom, tp, mo


def _device(device, who: str) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who}: device {device} is not a GPU; the image-source kernel has no host fallback")
    return device


def _launch(geom: np.ndarray, tp: list, mo, device: torch.device, out=None):
    """The checked rooms on the device -> (rows, the device taps table, the per-tile image counts)."""
    B, Kmax = geom.shape[0], max(tp)
    with torch.cuda.device(device):
        g = torch.from_numpy(geom).to(device)
        table = torch.tensor([tp, mo if mo is not None else [0] * B], dtype=torch.int32).to(device)
        h, counts = ops.ism_rir(g, table[0], table[1] if mo is not None else None, B, Kmax, out)
    return h, table[0], counts


def shoebox_rir(room, source, mic, beta, taps, fs=16000, c=343.0, max_order=None, max_images=2 ** 28, device="cuda") -> torch.Tensor:
    """The impulse responses of B rectangular rooms -> float32 [B, max(taps)] on ``device``: row b its ``taps[b]`` samples, zeros
    behind them.  ``room`` [B, 3]: the sizes in metres; ``source``, ``mic`` [B, 3]: positions strictly inside; ``beta`` [B, 6]: the
    reflection coefficients of the walls at x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz, each in [-1, 1] (python sequences, numpy
    arrays or CPU tensors; one room may be given without the batch axis).  ``taps``: an integer or one per room, 1 .. 65536;
    ``fs`` samples per second, ``c`` metres per second; ``max_order``: None, an integer or one per room, the most reflections an image
    may have had.  Refused on the host before any device work: wrong shapes, values that are not finite, a size that is not positive,
    a position on a wall or outside, |beta| > 1, source and microphone closer than ``c / fs``, rooms whose estimated image count
    ``4/3 pi d_max^3 / V`` exceeds ``max_images``, and a GPU tensor for the geometry."""
    geom, tp, mo = check_rooms(room, source, mic, beta, taps, fs, c, max_order, max_images)
    return _launch(geom, tp, mo, _device(device, "shoebox_rir"))[0]


def beta_from_t60(room, t60) -> np.ndarray:
    """Sabine's design rule (host): ``alpha = 0.161 V / (S t60)``, refused at ``alpha >= 1``, ``beta = sqrt(1 - alpha)`` for all six
    walls -> float64 [B, 6].  The formula is a design rule: the decay that the image-source response realises differs from it, and
    nothing here asserts a realised T60."""
    L = _host_rows("room", room, 3, "beta_from_t60")
    t = np.array(t60, dtype=np.float64).reshape(-1)
    if t.shape[0] == 1 and L.shape[0] > 1:
        t = np.repeat(t, L.shape[0])
    if t.shape[0] != L.shape[0] or not np.isfinite(t).all() or (t <= 0).any() or (L <= 0).any():
        raise ValueError("beta_from_t60: one finite t60 > 0 per room of positive size is expected")
    V = L.prod(axis=1)
    S = 2.0 * (L[:, 0] * L[:, 1] + L[:, 0] * L[:, 2] + L[:, 1] * L[:, 2])
    alpha = 0.161 * V / (S * t)
    if (alpha >= 1).any():
        b = int(np.argmax(alpha >= 1))
        raise ValueError(f"beta_from_t60: room {b}: t60 = {t[b]:.4g} s asks for an absorption of {alpha[b]:.3g} >= 1")
    return np.repeat(np.sqrt(1.0 - alpha)[:, None], 6, axis=1)


def draw_rooms(k: int, seed: int, n: int, size_lo=(3, 3, 2.5), size_hi=(10, 8, 4), t60=(0.2, 0.8), margin: float = 0.5,
               min_dist: float = 0.5, tries: int = 64) -> Rooms:
    """The ``n`` rooms of pool ``k``: sizes uniform in ``size_lo .. size_hi``, a ``t60`` uniform in its range turned into six equal
    wall coefficients by :func:`beta_from_t60`, source and microphone uniform at least ``margin`` from every wall and ``min_dist``
    apart (by rejection, ``tries`` at the most).  Host only, a function of ``(seed, k)`` and the arguments alone, from a generator of
    its own: what :func:`~.mix.draw_batch` and :func:`~.reverb.draw_reverb` return for ``(seed, k)`` does not change."""
    _int("k", k, 0, "draw_rooms")
    _int("seed", seed, 0, "draw_rooms")
    _int("n", n, 1, "draw_rooms")
    _int("tries", tries, 1, "draw_rooms")
    lo, hi = _host_rows("size_lo", size_lo, 3, "draw_rooms")[0], _host_rows("size_hi", size_hi, 3, "draw_rooms")[0]
    tr = _host_rows("t60", t60, 2, "draw_rooms")[0]
    for name, v in (("margin", margin), ("min_dist", min_dist)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"draw_rooms: {name} = {v!r}: a finite number >= 0 is expected")
    if (lo <= 0).any() or (hi < lo).any() or tr[0] <= 0 or tr[1] < tr[0]:
        raise ValueError("draw_rooms: 0 < size_lo <= size_hi and 0 < t60[0] <= t60[1] are expected")
    if (lo <= 2 * margin).any():
        raise ValueError(f"draw_rooms: a room of {tuple(lo)} m leaves no place {margin} m from every wall")
    rng = random.Random(f"room:{seed}:{k}")
    room, src, mic, t60s = [], [], [], []
    for i in range(n):
        L = [rng.uniform(lo[a], hi[a]) for a in range(3)]
        t = rng.uniform(tr[0], tr[1])
        for _ in range(tries):
            s = [rng.uniform(margin, L[a] - margin) for a in range(3)]
            r = [rng.uniform(margin, L[a] - margin) for a in range(3)]
            inside = all(0 < s[a] < L[a] and 0 < r[a] < L[a] for a in range(3))
            if inside and math.dist(s, r) >= min_dist:
                break
        else:
            raise ValueError(f"draw_rooms: room {i}: no source and microphone {min_dist} m apart in {tries} tries")
        room.append(L)
        src.append(s)
        mic.append(r)
        t60s.append(t)
    room = np.array(room, dtype=np.float64)
    t60s = np.array(t60s, dtype=np.float64)
    return Rooms(room, np.array(src, dtype=np.float64), np.array(mic, dtype=np.float64), beta_from_t60(room, t60s), t60s)
