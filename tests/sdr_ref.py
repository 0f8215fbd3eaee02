"""Host reference of the BSS-eval SDR (csrc/sdr.hip, inference.compute_sdr) in float64 numpy / scipy, the test signals and the cases
the SDR tests share.  A plain module: it calls nothing of the package under test.

The definition is ``bss_eval_sources`` of Vincent, Gribonval and Fevotte (2006) for ONE source with a distortion filter of ``K`` taps
(``mir_eval.separation.bss_eval_sources(ref[None], est[None])`` with ``flen = K``: there ``s_target`` is ``p``, ``e_interf`` is 0 and
``e_artif`` is ``e``).  For a reference ``s`` and an estimate ``y`` of ``L >= 1`` samples, both zero outside ``[0, L)``:

    r[k] = sum_n s[n] s[n + k]                 k = 0 .. K - 1
    d[k] = sum_n s[n] y[n + k]                 k = 0 .. K - 1
    G c = d,   G[i][j] = r[|i - j|]            (K x K, symmetric Toeplitz)
    p[n] = sum_{k < K} c[k] s[n - k]           n = 0 .. L + K - 2
    e[n] = y[n] - p[n]                         n = 0 .. L + K - 2
    SDR  = 10 log10( sum p^2 / sum e^2 )

``G = A'A`` with ``A`` the ``(L + K - 1) x K`` convolution matrix of ``s``, so ``G`` is positive definite for every reference that is
not silent, and ``L < K`` is a valid input.  The package forms ``r`` and ``d`` by FFT; the direct sums here agree with that form within
5e-16 of ``r[0]``.  Special rows, part of the definition here: a silent reference (``r[0] == 0``) gives NaN, ``sum p^2 == 0`` (a silent
estimate) gives -inf, ``sum e^2 == 0`` gives +inf.  Parity with the package itself is pinned by
tests/test_sdr_host.py::test_sdr_ref_matches_mir_eval where the package is installed.
"""
import numpy as np


def lag_sums(s, y, K):
    """r[k] = sum_n s[n] y[n + k], k < K, as direct float64 dot products."""
    L = len(s)
    out = np.zeros(K)
    for k in range(min(K, L)):
        out[k] = np.dot(s[:L - k], y[k:])
    return out


def toeplitz_matrix(r):
    k = np.arange(len(r))
    return r[np.abs(k[:, None] - k[None, :])]


def sdr(x_ref, x_est, K=512, solver="lu"):
    """-> dict(sdr, filter, target_energy, error_energy, r, d).  x_ref: the clean reference, x_est: the estimate (the package's order).
    ``solver``: "lu" (``np.linalg.solve``, the yardstick) or "levinson" (``scipy.linalg.solve_toeplitz``)."""
    s = np.asarray(x_ref, dtype=np.float64)
    y = np.asarray(x_est, dtype=np.float64)
    if s.ndim != 1 or s.shape != y.shape or len(s) < 1:
        raise ValueError("two 1-D signals of one length >= 1 expected")
    L = len(s)
    r, d = lag_sums(s, s, K), lag_sums(s, y, K)
    nan = float("nan")
    if r[0] == 0:
        return dict(sdr=nan, filter=np.full(K, nan), target_energy=nan, error_energy=nan, r=r, d=d)
    if solver == "lu":
        c = np.linalg.solve(toeplitz_matrix(r), d)
    elif solver == "levinson":
        from scipy.linalg import solve_toeplitz
        c = solve_toeplitz(r, d)
    else:
        raise ValueError(f"solver {solver!r}")
    p = np.convolve(c, s)                                                   # L + K - 1 samples
    e = np.concatenate([y, np.zeros(K - 1)]) - p
    tp, te = float(np.sum(p * p)), float(np.sum(e * e))
    if tp == 0:
        val = -np.inf
    elif te == 0:
        val = np.inf
    else:
        val = 10 * np.log10(tp / te)
    return dict(sdr=float(val), filter=c, target_energy=tp, error_energy=te, r=r, d=d)


def condition(r):
    return float(np.linalg.cond(toeplitz_matrix(r)))


def residual(c, r, d):
    """The normal-equation residual max |G c - d| / r[0] of a filter c in float64."""
    return float(np.max(np.abs(toeplitz_matrix(r) @ np.asarray(c, dtype=np.float64) - d)) / r[0])


def sisdr(x_est, x_ref):
    """utils/eval_metrics.py:49-64 in float64."""
    e, r = np.asarray(x_est, dtype=np.float64), np.asarray(x_ref, dtype=np.float64)
    t = np.sum(e * r) / np.sum(r * r) * r
    return float(10 * np.log10(np.sum(t * t) / np.sum((e - t) ** 2)))


# ----------------------------------------------------------------------------- signals (float32 values: what the device is given)
FLOOR = 1e-3
CHANNEL_DELAY = 3
CHANNEL = np.array([0.0, 0.0, 0.0, 0.8, -0.35, 0.2, 0.1, -0.05, 0.03])     # 9 taps: it fits the shortest filter (16)


def reference(L, kind, seed=0):
    """White ("white") or low-passed ("lowpass": a 9-tap moving average, about 1.8 kHz at 16 kHz) noise of unit scale 0.1, plus a
    white floor of 1e-3, as float32."""
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal(L + 8)
    if kind == "white":
        x = x[8:]
    elif kind == "lowpass":
        x = np.convolve(x, np.ones(9) / 3.0, mode="valid")
    else:
        raise ValueError(f"kind {kind!r}")
    return (0.1 * x + FLOOR * rng.standard_normal(L)).astype(np.float32)


def estimate(ref, snr_db, seed=0):
    """The reference through CHANNEL (three samples of delay), cut to its length, plus white noise ``snr_db`` under the REFERENCE's energy
    (the channel's output is silent for a row shorter than the delay), as float32."""
    s = np.asarray(ref, dtype=np.float64)
    nz = np.random.default_rng(2000 + seed).standard_normal(len(s))
    g = np.sqrt(np.sum(s * s) / (np.sum(nz * nz) * 10 ** (snr_db / 10)))
    return (np.convolve(s, CHANNEL)[:len(s)] + g * nz).astype(np.float32)


SNRS = (60, 20, 0)
_SHAPES = {16: (1, 5, 15, 16, 17, 31, 33), 64: (63, 64, 65, 255, 257, 4001), 512: (300, 511, 512, 513, 1023, 1025, 16385)}
# (L, K, kind): the smallest shapes at which the tiling can go wrong -- one sample, one short of / at / one past the filter length, the
# 16-sample block and the 256-lag tile, more than one 4096-sample tile of either tiled pass
CASES = [(L, K, ("white", "lowpass")[j % 2]) for K in sorted(_SHAPES) for j, L in enumerate(_SHAPES[K])]


def case_snr(index):
    """The SNR of CASES[index]: SNRS walked from the longest row of each K down, so the longest has the 60 dB."""
    L, K, _ = CASES[index]
    return SNRS[(len(_SHAPES[K]) - 1 - _SHAPES[K].index(L)) % 3]


def case_signals(index):
    """(reference, estimate) of CASES[index], float32."""
    L, K, kind = CASES[index]
    ref = reference(L, kind, seed=index)
    return ref, estimate(ref, case_snr(index), seed=index)
