"""Latent-space report on the device, for padded batches of utterances of any lengths (csrc/latent.hip).

What the reference's two evaluation scripts compute on the host, one utterance at a time:

  * :func:`posterior_stats`  pretrained_vaes/test_prevae.py:25-74, 171-197 -- the posterior covariance entries vrr / vri / vii (min,
    max, mean, norm) and the script's KL form, per row;
  * :func:`pair_distance`    nsvae_dccrn/test_nsvae_se.py:27-35, 416-418 -- dis_mean / dis_sigma / dis_delta between two posteriors;
  * :class:`MiuMoments`      test_prevae.py:204-207, 285-333 -- the covariance of miu over every frame of the test set;
  * :func:`sample_rows`, :func:`silhouette`  test_nsvae_se.py:39-50, 309-331, 482-502 -- the simplified silhouette score between
    sampled speech and noise latents.

Latent arguments are ``[B, T, zdim, 2]`` float32 GPU tensors.  The views the encoders return (``_idv`` the planar LSTM output,
``_idv_off`` the channel offset) are read in place; any other tensor is copied into a planar buffer first, and both routes run the
same kernels in the same order and return the same bits.  ``frames``: the valid frames per row (python sequence or CPU integer
tensor, 1 <= frames[b] <= T; None: T each) -- nothing at or past them is read.  Per-row results are float64 tensors ``[B]`` on the
device; a row's value does not depend on the batch around it.  All argument errors are raised before the device is touched.
"""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .ops import Planar

STAT_KEYS = ("kl",) + tuple(f"{v}{s}" for v in ("vrr", "vri", "vii") for s in ("_min", "_max", "_mean", ""))
DIST_KEYS = ("dis_mean", "dis_sigma", "dis_delta")


# ----------------------------------------------------------------------------- host-side checks
def check_zdim(zdim) -> int:
    if isinstance(zdim, bool) or not isinstance(zdim, int) or zdim % 16 or not 16 <= zdim <= 128:
        raise ValueError(f"zdim = {zdim!r}: a multiple of 16 in [16, 128] expected")
    return zdim


def check_frames(frames, B: int, T: int) -> Optional[list]:
    """The guards on the valid frames per row (host only, no device use) -> list of ints, or None for None."""
    if frames is None:
        return None
    if isinstance(frames, torch.Tensor):
        if frames.is_cuda:
            raise ValueError("frames must be a python sequence or a CPU integer tensor: a GPU tensor would have to be fetched with a "
                             "synchronisation")
        if frames.dim() != 1 or frames.is_floating_point() or frames.is_complex() or frames.dtype == torch.bool:
            raise ValueError("frames must be a 1-D integer tensor")
        frames = frames.tolist()
    elif isinstance(frames, (str, bytes)) or not isinstance(frames, Sequence):
        raise ValueError("frames must be a python sequence or a CPU integer tensor")
    if any(isinstance(v, bool) or not isinstance(v, int) for v in frames):
        raise ValueError("frames must be integers (frame counts)")
    if len(frames) != B:
        raise ValueError(f"{len(frames)} frame counts for a batch of {B} rows")
    for b, v in enumerate(frames):
        if not 1 <= v <= T:
            raise ValueError(f"frames[{b}] = {v}: expected 1 <= frames <= T = {T}")
    return list(frames)


def frames(lengths, hop: int) -> List[int]:
    """Sample counts -> valid frames per row, 1 + n // hop (the STFT of the models)."""
    if isinstance(hop, bool) or not isinstance(hop, int) or hop <= 0:
        raise ValueError(f"hop = {hop!r} must be a positive integer")
    if isinstance(lengths, ops.Lengths):
        lengths = lengths.host
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda or lengths.dim() != 1 or lengths.is_floating_point():
            raise ValueError("lengths must be a python sequence or a 1-D CPU integer tensor")
        lengths = lengths.tolist()
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in lengths):
        raise ValueError("lengths must be non-negative integers (sample counts)")
    return [1 + v // hop for v in lengths]


def frames_of(stft_x, hop: Optional[int] = None) -> List[int]:
    """The valid frames per row of the batch an encoder ran on: ``stft_x`` is the spectrum [B, F, T, 2] it returns.  With
    ``lengths=`` the rows have 1 + lengths[b] // hop frames (``hop``: the encoder's, carried by ``stft_x``), else T each."""
    if not isinstance(stft_x, torch.Tensor) or stft_x.dim() != 4:
        raise ValueError("frames_of: the stft_x [B, F, T, 2] an encoder returns expected")
    B, T = stft_x.shape[0], stft_x.shape[2]
    lengths = getattr(getattr(stft_x, "_idv", None), "lengths", None)
    if lengths is None:
        return [T] * B
    hop = getattr(stft_x, "_idv_hop", None) if hop is None else hop
    if hop is None:
        raise ValueError("frames_of: this stft_x does not carry its hop length; pass hop=")
    return frames(lengths, hop)


def _check_latent(t, name: str, shape=None) -> Tuple[int, int, int]:
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[3] != 2:
        raise ValueError(f"{name}: a [B, T, zdim, 2] tensor expected")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: float32 expected, got {t.dtype}")
    B, T, z, _ = t.shape
    if B < 1 or T < 1:
        raise ValueError(f"{name}: an empty batch")
    if B > 65535:
        raise ValueError(f"{name}: a batch of {B} rows; at most 65535 are supported")
    check_zdim(z)
    if shape is not None and (B, T, z) != shape:
        raise ValueError(f"{name}: shape {tuple(t.shape)} does not match the [{shape[0]}, {shape[1]}, {shape[2]}, 2] of the others")
    return B, T, z


def _check_triple(q, name: str, shape=None):
    if not isinstance(q, (tuple, list)) or len(q) != 3:
        raise ValueError(f"{name}: a (miu, log_sigma, delta) triple expected")
    for t, what in zip(q, ("miu", "log_sigma", "delta")):
        shape = _check_latent(t, f"{name} {what}".strip(), shape)
    return shape


def _check_device(tensors, device=None):
    for t in tensors:
        ops.check_dev_f32(t, "latent", device)
        device = t.device
    return device


# ----------------------------------------------------------------------------- planar sources
def _in_place(t: torch.Tensor) -> Optional[Planar]:
    pl = getattr(t, "_idv", None)
    off = getattr(t, "_idv_off", None)
    if isinstance(pl, Planar) and pl.F == 1 and isinstance(off, int) and (pl.B, pl.T) == tuple(t.shape[:2]) and \
            0 <= off and off + t.shape[2] <= pl.C and pl.buf.device == t.device:
        return pl
    return None


def _source(tensors) -> Tuple[Planar, tuple]:
    """(planar buffer, channel offsets) of latents of one shape: the encoder's buffer when all of them are views of it, else one
    fresh buffer that holds copies (as ``reparameterization`` packs foreign tensors)."""
    pls = [_in_place(t) for t in tensors]
    if pls[0] is not None and all(pl is pls[0] for pl in pls):
        return pls[0], tuple(t._idv_off for t in tensors)
    z = tensors[0].shape[2]
    lat = torch.cat(list(tensors), dim=2) if len(tensors) > 1 else tensors[0]
    return Planar.from_tensor5(lat.permute(0, 2, 1, 3).unsqueeze(2).float()), tuple(k * z for k in range(len(tensors)))


def _frames_dev(host: Optional[list], device):
    return None if host is None else torch.tensor(host, dtype=torch.int32, device=device)


# ----------------------------------------------------------------------------- per-row reports
def posterior_stats(miu, log_sigma, delta, frames=None) -> dict:
    """Per row: ``kl`` (the script's form: mean_t [sum_h |miu|^2 + sum_h |sigma - 1 - 0.5 log(sigma^2 - |delta|^2 + 1e-6)|]) and, for
    v in vrr / vri / vii of the guarded posterior covariance, ``v_min``, ``v_max`` over the row's (t, h), ``v_mean`` =
    mean_h mean_t |v| and ``v`` = sqrt(sum_h (mean_t |v|)^2).  Only the real channel of ``log_sigma`` is read.
    -> {key: float64 [B] on the device}."""
    B, T, z = _check_triple((miu, log_sigma, delta), "")
    host = check_frames(frames, B, T)
    dev = _check_device((miu, log_sigma, delta))
    with torch.cuda.device(dev):
        q, off = _source((miu, log_sigma, delta))
        out = ops.latent_row_stats(q, off, z, _frames_dev(host, dev), B, T)
    return {k: out[:, n] for n, k in enumerate(STAT_KEYS)}


def pair_distance(a, b, frames=None) -> dict:
    """``a``, ``b``: (miu, log_sigma, delta) triples of two posteriors of the same [B, T, zdim].  Per row: ``dis_mean`` =
    sqrt(sum_{h,ri} mean_t (miu_a - miu_b)^2), ``dis_delta`` the same on delta, ``dis_sigma`` = sqrt(sum_h mean_t
    (exp(ls_a) - exp(ls_b))^2) on the real channel.  -> {key: float64 [B] on the device}."""
    shape = _check_triple(a, "a")
    _check_triple(b, "b", shape)
    B, T, z = shape
    host = check_frames(frames, B, T)
    dev = _check_device(tuple(a) + tuple(b))
    with torch.cuda.device(dev):
        qa, oa = _source(tuple(a))
        qb, ob = _source(tuple(b))
        out = ops.latent_pair_dist(qa, oa, qb, ob, z, _frames_dev(host, dev), B, T)
    return {k: out[:, n] for n, k in enumerate(DIST_KEYS)}


# ----------------------------------------------------------------------------- covariance of miu over a corpus
class MiuMoments:
    """Running mean and covariance of the real and imaginary parts of miu over all valid frames fed to :meth:`update`
    (test_prevae.py:285-333, which holds every frame of the test set in host memory).  State on the device, double: n, the mean
    of the 2 zdim rows (real, then imaginary) and their co-moment matrix.  Nothing touches the device before the first
    :meth:`update` / :meth:`merge`."""

    def __init__(self, zdim: int, device):
        self.zdim = check_zdim(zdim)
        self.device = torch.device(device)
        self._count = 0
        self._state = None

    @property
    def count(self) -> int:
        """Frames accumulated so far (kept on the host: no synchronisation)."""
        return self._count

    def _ensure(self):
        if self._state is not None:
            return
        dev = self.device
        if dev.type != "cuda":
            raise ops.L.IdvError(f"device {dev}: expected a CUDA (ROCm) device; the HIP hot path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        R = 2 * self.zdim
        self._state = torch.zeros(1 + R + R * R, dtype=torch.float64, device=self.device)

    def update(self, miu, frames=None) -> "MiuMoments":
        """Fold the valid frames of a batch miu [B, T, zdim, 2] in."""
        B, T, z = _check_latent(miu, "miu")
        if z != self.zdim:
            raise ValueError(f"MiuMoments.update: zdim {z}, this accumulator was made for {self.zdim}")
        host = check_frames(frames, B, T)
        ops.check_dev_f32(miu, "miu")
        self._ensure()
        ops.check_dev_f32(miu, "miu", self.device)
        with torch.cuda.device(self.device):
            q, off = _source((miu,))
            ops.miu_moments_update(q, off[0], z, _frames_dev(host, self.device), B, T, self._state)
        self._count += B * T if host is None else sum(host)
        return self

    def merge(self, other: "MiuMoments") -> "MiuMoments":
        """Fold another accumulator's state in (Chan's merge, on this one's device): data-parallel ranks or shards."""
        if not isinstance(other, MiuMoments) or other is self:
            raise ValueError("MiuMoments.merge: another MiuMoments expected")
        if other.zdim != self.zdim:
            raise ValueError("MiuMoments.merge: the two accumulators differ in zdim")
        if other._count == 0:
            return self
        self._ensure()
        with torch.cuda.device(self.device):
            ops.miu_moments_merge(self._state, other._state.to(self.device), self.zdim)
        self._count += other._count
        return self

    def result(self) -> dict:
        """-> float64 numpy arrays: ``n``, ``mean_real`` / ``mean_imag`` [z], ``cov_rr`` / ``cov_ri`` / ``cov_ii`` [z, z] (centred
        cross products / n; cov_ri[h1, h2] pairs real h1 with imaginary h2) and ``mean_dis``.  One copy to the host."""
        if self._count < 1:
            raise ValueError("MiuMoments.result: no frames yet")
        st = self._state.cpu().numpy()
        z, R = self.zdim, 2 * self.zdim
        if int(st[0]) != self._count:
            raise RuntimeError(f"MiuMoments: the device counted {int(st[0])} frames, the host {self._count}")
        mean = st[1:1 + R]
        C = st[1 + R:].reshape(R, R)
        blk = np.arange(R) >> 5                                           # the device writes the 32 x 32 blocks on and above the diagonal
        C = np.where(blk[:, None] > blk[None, :], C.T, C) / st[0]
        return {"n": float(st[0]), "mean_real": mean[:z].copy(), "mean_imag": mean[z:].copy(), "cov_rr": C[:z, :z].copy(),
                "cov_ri": C[:z, z:].copy(), "cov_ii": C[z:, z:].copy(), "mean_dis": float(np.sqrt(np.sum(mean ** 2)))}

    def summary(self) -> dict:
        """The script's log numbers for rr / ri / ii: ``diag_abs_<k>`` (sum |diag| / z), ``diag_min_<k>``, ``diag_max_<k>``,
        ``diag_mean_<k>`` and ``offdiag_abs_<k>`` (sum |offdiag| / (z (z - 1))), plus ``mean_dis``."""
        res = self.result()
        out = cov_summary(res["cov_rr"], res["cov_ri"], res["cov_ii"])
        out["mean_dis"] = res["mean_dis"]
        return out


def cov_summary(cov_rr, cov_ri, cov_ii) -> dict:
    """test_prevae.py:301-333 on three [z, z] matrices (host numpy)."""
    out = {}
    for k, c in (("rr", cov_rr), ("ri", cov_ri), ("ii", cov_ii)):
        c = np.asarray(c)
        z = c.shape[0]
        diag = np.diagonal(c, 0)
        off = c - np.diag(diag)
        out[f"diag_abs_{k}"] = float(np.sum(np.abs(diag)) / z)
        out[f"diag_max_{k}"] = float(np.max(diag))
        out[f"diag_min_{k}"] = float(np.min(diag))
        out[f"diag_mean_{k}"] = float(np.mean(diag))
        out[f"offdiag_abs_{k}"] = float(np.sum(np.abs(off)) / (z * (z - 1)))
    return out


# ----------------------------------------------------------------------------- sampled sets
def sample_indices(frames: Sequence[int], n: int, rng: random.Random) -> Tuple[List[int], List[int]]:
    """min(n, frames[b]) distinct frame indices below frames[b] for every row b, drawn with ``rng`` -> (rows, frame indices)."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"n = {n!r}: a positive number of frames per row expected")
    if not isinstance(rng, random.Random):
        raise ValueError("rng: a random.Random expected")
    rows, cols = [], []
    for b, fb in enumerate(frames):
        pick = rng.sample(range(fb), min(n, fb))
        rows += [b] * len(pick)
        cols += pick
    return rows, cols


def sample_rows(v: torch.Tensor, frames, n: int, rng: random.Random) -> torch.Tensor:
    """min(n, frames[b]) random valid frames of every row of v [B, T, zdim, 2] -> a contiguous [N, zdim, 2] tensor on v's device
    (test_nsvae_se.py:309-331 takes 40 of z and 50 of miu per utterance).  Ordinary torch indexing: not a hot path."""
    if not isinstance(v, torch.Tensor) or v.dim() != 4 or v.shape[3] != 2:
        raise ValueError("sample_rows: a [B, T, zdim, 2] tensor expected")
    B, T = v.shape[:2]
    host = check_frames([T] * B if frames is None else frames, B, T)
    rows, cols = sample_indices(host, n, rng)
    return v[torch.tensor(rows, device=v.device), torch.tensor(cols, device=v.device)].contiguous()


def _check_set(s, name: str) -> Tuple[int, int]:
    if not isinstance(s, torch.Tensor) or s.dim() != 3 or s.shape[2] != 2:
        raise ValueError(f"{name}: a [N, zdim, 2] tensor expected")
    if s.dtype != torch.float32:
        raise ValueError(f"{name}: float32 expected, got {s.dtype}")
    if s.shape[0] < 1:
        raise ValueError(f"{name}: an empty set")
    return s.shape[0], check_zdim(s.shape[1])


def silhouette(set1: torch.Tensor, set2: torch.Tensor) -> dict:
    """The script's simplified silhouette score ('euclidean') between two sets of latent vectors [N1, z, 2] / [N2, z, 2]:
    ``sc`` = the mean over both sets of (inter - intra) / max(intra, inter), intra / inter the distances of a vector to its own /
    the other set's mean; ``mean_dis`` = sum (mean1 - mean2)^2 (no square root); ``var_avg_1`` / ``var_avg_2`` = (real, imag) of the
    population variance over N averaged over h.  Python floats (one copy to the host)."""
    N1, z = _check_set(set1, "set1")
    N2, z2 = _check_set(set2, "set2")
    if z != z2:
        raise ValueError(f"silhouette: zdim {z} and {z2} differ")
    if (N1 + N2) * 2 * z > 2 ** 31 - 1:
        raise ValueError("silhouette: the sets are too large")
    dev = _check_device((set1, set2))
    with torch.cuda.device(dev):
        x1, x2 = set1.contiguous(), set2.contiguous()
        m1, m2 = ops.latent_set_moments(x1), ops.latent_set_moments(x2)
        out = ops.latent_silhouette(x1, x2, m1, m2).cpu().tolist()
    return {"sc": out[0], "mean_dis": out[1], "var_avg_1": (out[2], out[3]), "var_avg_2": (out[4], out[5])}
