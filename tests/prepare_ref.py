"""Float64 numpy definitions of the corpus-preparation family: the yardstick of tests/test_gpu_prepare.py and of
profiles/tools/measure_prepare.py.  No GPU, no package import.

  resampler   scipy.signal.resample_poly(x, up, down) with its default filter, and the same thing written out:
              m = max(up, down), half = 10 m, h = kaiser(2 half + 1, 5.0) * sinc(t / m) / m normalised to sum 1,
              y[n] = up * sum_j x[j] h[half + n down - j up] over 0 <= j < L with the tap index in [0, 2 half], n < ceil(L up / down)
  spectrum    centred frames every hop of the signal padded by n_fft/2 on both sides (zeros: librosa >= 0.10's stft; or the mirror:
              torch.stft), periodic hann(win) centred in n_fft, one-sided DFT as a matrix product
  moments     per bin and part, mean and std (ddof=1) over the concatenated frames of all signals, two passes
  chan_merge  Chan's merge of two (n, mean, M2) triples
"""
import math

import numpy as np

NFFT, WIN, HOP = 512, 400, 100


def ratio(up, down):
    g = math.gcd(up, down)
    return up // g, down // g


def n_out(L, up, down):
    up, down = ratio(up, down)
    return -((-L * up) // down)


def taps(up, down):
    up, down = ratio(up, down)
    m = max(up, down)
    half = 10 * m
    t = np.arange(-half, half + 1, dtype=np.float64)
    h = np.kaiser(2 * half + 1, 5.0) * np.sinc(t / m) / m
    return h / h.sum()


def resample_written_out(x, up, down):
    up, down = ratio(up, down)
    x = np.asarray(x, dtype=np.float64)
    h = taps(up, down)
    half = (len(h) - 1) // 2
    L = len(x)
    y = np.zeros(n_out(L, up, down))
    for n in range(len(y)):
        jlo = max(0, -((half - n * down) // up))
        jhi = min(L - 1, (n * down + half) // up)
        if jhi >= jlo:
            j = np.arange(jlo, jhi + 1)
            y[n] = up * np.dot(x[j], h[half + n * down - j * up])
    return y


def resample(x, up, down, dtype=np.float64):
    """scipy's resample_poly in ``dtype`` (float32: the taps and the products are float32 too)."""
    from scipy.signal import resample_poly
    up, down = ratio(up, down)
    return resample_poly(np.asarray(x, dtype=dtype), up, down)


def dft_matrix(n_fft=NFFT, win=WIN):
    """[n_fft, 2F]: columns F real parts, then F imaginary parts of the windowed one-sided DFT, X = frame @ W."""
    F = n_fft // 2 + 1
    w = np.zeros(n_fft)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
    q = (np.arange(n_fft)[:, None] * np.arange(F)[None, :]) % n_fft          # exact phase reduction
    c, s = np.cos(2 * np.pi * q / n_fft), np.sin(2 * np.pi * q / n_fft)
    s[q % (n_fft // 2) == 0] = 0.0                                           # sin(0), sin(pi): the imaginary parts of bins 0 and n_fft/2
    if n_fft % 4 == 0:
        c[q % (n_fft // 2) == n_fft // 4] = 0.0
    return np.concatenate([w[:, None] * c, -w[:, None] * s], axis=1)


def frames(x, pad_mode, n_fft=NFFT, hop=HOP):
    """[T = 1 + L // hop, n_fft] centred frames of the padded signal."""
    x = np.asarray(x)
    xp = np.pad(x, n_fft // 2, mode="constant" if pad_mode == "constant" else "reflect")
    T = 1 + len(x) // hop
    return np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)])


def spec(x, pad_mode, n_fft=NFFT, win=WIN, hop=HOP, dtype=np.float64):
    """[T, F, 2] (real, imaginary).  ``dtype`` float32: float32 frames times a float32 matrix, accumulated in float32."""
    F = n_fft // 2 + 1
    X = frames(np.asarray(x, dtype=dtype), pad_mode, n_fft, hop) @ dft_matrix(n_fft, win).astype(dtype)
    return np.stack([X[:, :F], X[:, F:]], axis=2)


def moments(signals, pad_mode, n_fft=NFFT, win=WIN, hop=HOP, dtype=np.float64):
    """-> (mean [F, 2], std [F, 2], number of frames): np.mean / np.std(ddof=1) in float64 over the frames of all signals."""
    feat = np.concatenate([spec(x, pad_mode, n_fft, win, hop, dtype) for x in signals], axis=0).astype(np.float64)
    return feat.mean(axis=0), feat.std(axis=0, ddof=1), feat.shape[0]


def triple(feat):
    """(n, mean, M2) of an array of observations [n, ...], two passes."""
    feat = np.asarray(feat, dtype=np.float64)
    mean = feat.mean(axis=0)
    return feat.shape[0], mean, ((feat - mean) ** 2).sum(axis=0)


def chan_merge(a, b):
    (na, ma, Ma), (nb, mb, Mb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    d = mb - ma
    return n, ma + d * (nb / n), Ma + Mb + d * d * (na * (nb / n))


def dc_signal(n, seed):
    """0.05 N(0, 1) + 0.5 as float32: the DC offset puts the mean of bin 0 near 100 with a std below 1."""
    return (0.05 * np.random.default_rng(seed).standard_normal(n) + 0.5).astype(np.float32)
