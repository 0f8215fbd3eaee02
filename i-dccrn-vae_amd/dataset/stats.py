"""Per-bin STFT mean / std tables of a corpus, computed on the device: the ``mean_file`` / ``std_file`` every reference config names
and ``--data_norm`` reads (reference: dataset/cal_mean_std.py:51-89, which needs librosa and holds every frame of the corpus in
host memory before it takes ``np.mean`` / ``np.std(ddof=1)``).

  * :class:`SpecMoments` keeps a running (n, mean, M2) per real / imaginary STFT row in double on the device (csrc/moments.hip):
    ``update`` frames a padded batch (csrc/ragged.hip, zero padding of the signal ends as ``librosa.stft(center=True)`` of the pinned
    librosa 0.10 pads, or torch.stft's mirror), applies the fp32 DFT GEMM and folds the valid frames in; ``merge`` combines the states
    of data-parallel ranks or loader shards; ``result`` / ``save`` / ``buffers`` give the ``(F, 2)`` tables, the text files and the
    ``(1, F, 1, 2)`` float32 buffers ``DCCRN_`` and the VAE classes take as ``data_mean`` / ``data_std``.
  * :func:`cal_mean_std` runs a list of wav paths or tensors through it, resampling what is not at ``fs`` on the device
    (``inference.resample_list``: scipy's ``resample_poly`` definition -- the reference calls ``librosa.resample``, whose soxr filter
    is another one; parity with librosa itself is unpinned, it is not a dependency).
  * the command line takes the reference script's options::

        python -m i-dccrn-vae_amd.dataset.stats --cfg_file configs/pretrained_cvae.ini --folder DIR \\
            --file_name_out_mean mean.txt --file_name_out_std std.txt [--n_jobs 4]
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import inference, ops
from .._lib import call, i, ll, p, stream_ptr
from .dataload import read_wav


def _resolve(device) -> torch.device:
    """``"cuda"`` -> the current device with its index, so that tensors can be compared against it; a CPU device is an error."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ops.L.IdvError(f"device {device}: expected a CUDA (ROCm) device; the HIP hot path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


class SpecMoments:
    """Running mean and variance of the real and imaginary parts of every STFT bin over all frames fed to :meth:`update`.

    ``n_fft, win, hop``: the STFT of the models (periodic hann(win) centred in n_fft, frames every hop, centred); ``pad_mode``:
    "constant" (zeros before and behind the signal: librosa >= 0.10, what the reference's tables were made with) or "reflect"
    (torch.stft's mirror, what the models' own STFT does; needs more than n_fft/2 samples per signal).  A signal of L samples
    contributes 1 + L // hop frames in both modes.  Nothing touches the device before the first :meth:`update` / :meth:`merge`."""

    def __init__(self, n_fft: int, win: int, hop: int, device, pad_mode: str = "constant"):
        for name, v in (("n_fft", n_fft), ("win", win), ("hop", hop)):
            if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
                raise ValueError(f"SpecMoments: {name} = {v!r} must be a positive integer")
        if n_fft % 2 or win % 2 or win > n_fft:
            raise ValueError(f"SpecMoments: n_fft = {n_fft} and win = {win} must be even, win <= n_fft")
        if pad_mode not in ops.PAD_MODES:
            raise ValueError(f"SpecMoments: pad_mode = {pad_mode!r}: expected one of {sorted(ops.PAD_MODES)}")
        self.n_fft, self.win, self.hop, self.pad_mode = n_fft, win, hop, pad_mode
        self.F = n_fft // 2 + 1
        self.device = torch.device(device)
        self._count = 0
        self._state = None           # double [1 + 4F] on the device: n, mean[2F], M2[2F] (rows: real bins, then imaginary bins)
        self._fwd = None             # the forward DFT matrix packed for idv_pw_gemm, once

    @property
    def count(self) -> int:
        """Frames accumulated so far (kept on the host: no synchronisation)."""
        return self._count

    def _ensure(self):
        if self._state is not None:
            return
        self.device = _resolve(self.device)
        with torch.cuda.device(self.device):
            F = self.F
            w_fwd = torch.empty(2 * F, self.win, dtype=torch.float32, device=self.device)
            w_inv = torch.empty(self.win, 2 * F, dtype=torch.float32, device=self.device)
            env = torch.empty(self.n_fft, dtype=torch.float32, device=self.device)
            call("idv_make_dft", i(self.n_fft), i(self.win), i(self.hop), i(1), p(w_fwd), p(w_inv), p(env), stream_ptr())
            self._fwd = ops.pack_pw(w_fwd, None)
            self._state = torch.zeros(1 + 4 * F, dtype=torch.float64, device=self.device)

    def update(self, x: torch.Tensor, lengths=None) -> "SpecMoments":
        """Fold the frames of a padded batch x [B, L] (or one signal [L]) in.  ``lengths``: samples per row (a python sequence or a
        CPU integer tensor); nothing at or past lengths[b] is read and only the 1 + lengths[b] // hop frames of row b count."""
        if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
            raise ValueError("SpecMoments.update: x must be a tensor [L] or [B, L]")
        if x.dim() == 1:
            x = x.reshape(1, -1)
        B, L = x.shape
        if L < 1:
            raise ValueError("SpecMoments.update: empty signals")
        if B > 65535:
            raise ValueError(f"SpecMoments.update: a batch of {B} rows; at most 65535 are supported")
        host = ops.check_lengths([L] * B if lengths is None else lengths, B, L, self.n_fft if self.pad_mode == "reflect" else None)
        ops.check_dev_f32(x, "x")
        self._ensure()
        ops.check_dev_f32(x, "x", self.device)
        with torch.cuda.device(self.device):
            x = ops._ragged_rows(x)
            lens = ops.Lengths(host, self.device)
            T = 1 + max(host) // self.hop
            Tp, rows = T + 1, 2 * self.F
            fr = ops.stft_frames_pad(x, lens, self.n_fft, self.win, self.hop, T, self.pad_mode)
            spec = ops.Planar.empty(1, self.F, B, T, Tp, self.device)
            ops.pw_gemm(fr.ptr(), self.win, self._fwd[0], self._fwd[1], rows, B, Tp, fr.Jp, T, spec.ptr())
            nbytes = int(ops._ll_fn("idv_spec_moments_work_bytes")(i(rows), i(B), i(Tp)))
            if nbytes < 0:
                raise ValueError(f"SpecMoments.update: a batch of {B} rows of {T} frames is not supported")
            work = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
            call("idv_spec_moments_update", spec.ptr(), p(lens.dev), i(B), i(self.hop), i(T), i(Tp), i(spec.Jp), i(rows), p(self._state),
                 p(work), ll(nbytes), stream_ptr())
        self._count += sum(1 + v // self.hop for v in host)
        return self

    def merge(self, other: "SpecMoments") -> "SpecMoments":
        """Fold another accumulator's state in (Chan's merge, on this one's device): data-parallel ranks or loader shards."""
        if not isinstance(other, SpecMoments) or other is self:
            raise ValueError("SpecMoments.merge: another SpecMoments expected")
        if (other.n_fft, other.win, other.hop, other.pad_mode) != (self.n_fft, self.win, self.hop, self.pad_mode):
            raise ValueError("SpecMoments.merge: the two accumulators differ in n_fft / win / hop / pad_mode")
        if other._count == 0:
            return self
        self._ensure()
        with torch.cuda.device(self.device):
            theirs = other._state.to(self.device)
            call("idv_spec_moments_merge", p(self._state), p(theirs), i(2 * self.F), stream_ptr())
        self._count += other._count
        return self

    def result(self):
        """-> (mean [F, 2], std [F, 2]) float64 numpy arrays, real parts in column 0 and imaginary parts in column 1, std with
        ``ddof=1``: the layout the reference writes.  One copy to the host."""
        if self._count < 2:
            raise ValueError(f"SpecMoments.result: {self._count} frames; the std (ddof=1) needs at least 2")
        st = self._state.cpu().numpy()
        F = self.F
        if int(st[0]) != self._count:
            raise RuntimeError(f"SpecMoments: the device counted {int(st[0])} frames, the host {self._count}")
        mean = st[1:1 + 2 * F].reshape(2, F).T.copy()
        std = np.sqrt(st[1 + 2 * F:].reshape(2, F).T / (st[0] - 1.0))
        return mean, std

    def save(self, mean_path: str, std_path: str):
        """``np.savetxt`` of the two tables: the ``mean_file`` / ``std_file`` of the configs."""
        mean, std = self.result()
        np.savetxt(mean_path, mean)
        np.savetxt(std_path, std)

    def buffers(self, device=None):
        """-> (data_mean, data_std) float32 tensors (1, F, 1, 2), as supervised_dccrn/train.py:394-397 reshapes the loaded tables:
        pass them as ``data_mean`` / ``data_std`` to ``DCCRN_`` and the VAE classes."""
        mean, std = self.result()
        dev = self.device if device is None else device
        return tuple(torch.from_numpy(a.reshape(1, a.shape[0], 1, a.shape[1])).float().to(dev) for a in (mean, std))


def _load(item, fs: int, device):
    """One entry of cal_mean_std's list -> (1-D float32 tensor on the device, its rate)."""
    if isinstance(item, (str, os.PathLike)):
        x, fs_x = read_wav(os.fspath(item))
        return torch.from_numpy(np.ascontiguousarray(x)).to(device), fs_x
    if isinstance(item, torch.Tensor):
        item = (item, fs)
    if not (isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], torch.Tensor)):
        raise ValueError("cal_mean_std: entries must be wav paths, tensors or (tensor, fs) pairs")
    x, fs_x = item
    if x.dim() != 1 or x.shape[0] < 1:
        raise ValueError("cal_mean_std: a signal must be a non-empty 1-D tensor")
    ops.check_dev_f32(x, "signal", device)
    return x.float(), fs_x


def cal_mean_std(files_or_signals: Sequence, n_fft: int, win: int, hop: int, fs: int = 16000, pad_mode: str = "constant",
                 max_batch: int = 64, num_workers: int = 0, device="cuda") -> SpecMoments:
    """The reference's ``Cal_mean_std`` on the device -> the filled :class:`SpecMoments` (``.result()``, ``.save()``, ``.buffers()``).

    ``files_or_signals``: wav paths (read with ``dataset.read_wav``; ``num_workers`` > 0 decodes them on that many threads), 1-D GPU
    tensors at ``fs`` or ``(tensor, rate)`` pairs.  Whatever is not at ``fs`` is resampled on the device first.  The list is taken
    in groups of 16 * ``max_batch`` entries, so no more than that is ever held; each group is cut into padded batches by
    ``inference.plan_ragged_batches`` and fed to one accumulator."""
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise ValueError("cal_mean_std: max_batch must be a positive integer")
    if isinstance(num_workers, bool) or not isinstance(num_workers, int) or num_workers < 0:
        raise ValueError("cal_mean_std: num_workers must be a non-negative integer")
    ops.resample_ratio(fs, fs)                                          # the guard on fs
    acc = SpecMoments(n_fft, win, hop, device, pad_mode)
    items = list(files_or_signals)
    acc._ensure()
    pool = None
    if num_workers > 0 and any(isinstance(v, (str, os.PathLike)) for v in items):
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(num_workers)
    try:
        group = 16 * max_batch
        for g0 in range(0, len(items), group):
            part = items[g0:g0 + group]
            loaded = list(pool.map(lambda v: _load(v, fs, acc.device), part)) if pool else [_load(v, fs, acc.device) for v in part]
            sigs: List[torch.Tensor] = [x for x, _ in loaded]
            rates = [r for _, r in loaded]
            if any(r != fs for r in rates):
                sigs = inference.resample_list(sigs, rates, fs, max_batch=max_batch)
            lens = [int(s.shape[0]) for s in sigs]
            for batch in inference.plan_ragged_batches(lens, hop, max_batch=max_batch):
                blens = [lens[k] for k in batch]
                padded = torch.zeros(len(batch), max(blens), dtype=torch.float32, device=acc.device)
                for row, k in enumerate(batch):
                    padded[row, :lens[k]] = sigs[k]
                acc.update(padded, blens)
    finally:
        if pool:
            pool.shutdown()
    return acc


def find_wavs(folder: str) -> List[str]:
    """Every ``*.wav`` under ``folder`` (any letter case), sorted by path."""
    out = []
    for root, _, names in os.walk(folder):
        out += [os.path.join(root, n) for n in names if n.lower().endswith(".wav")]
    return sorted(out)


def main(argv: Optional[Sequence[str]] = None) -> int:
    import argparse
    from ..utils.read_config import myconf
    ap = argparse.ArgumentParser(description="Per-bin STFT mean / std tables of a folder of wav files (the configs' mean_file / std_file)")
    ap.add_argument("--cfg_file", required=True, help=".ini with [STFT] winlen, nfft, hopfrac (the hop in samples) and fs")
    ap.add_argument("--folder", required=True, help="folder searched recursively for wav files")
    ap.add_argument("--file_name_out_mean", required=True)
    ap.add_argument("--file_name_out_std", required=True)
    ap.add_argument("--n_jobs", type=int, default=4, help="threads decoding wav files")
    ap.add_argument("--pad_mode", default="constant", choices=sorted(ops.PAD_MODES))
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    cfg = myconf()
    if not cfg.read(a.cfg_file):
        raise SystemExit(f"cannot read {a.cfg_file}")
    win, n_fft, hop, fs = (cfg.getint("STFT", k) for k in ("winlen", "nfft", "hopfrac", "fs"))
    files = find_wavs(a.folder)
    if not files:
        raise SystemExit(f"no wav files under {a.folder}")
    acc = cal_mean_std(files, n_fft, win, hop, fs, pad_mode=a.pad_mode, num_workers=max(0, a.n_jobs), device=a.device)
    acc.save(a.file_name_out_mean, a.file_name_out_std)
    print(f"{len(files)} files, {acc.count} frames -> {a.file_name_out_mean}, {a.file_name_out_std}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
