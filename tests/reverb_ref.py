"""Float64 numpy definition of reverberation: the yardstick of tests/test_gpu_reverb.py, tests/test_reverb_host.py and
profiles/tools/measure_reverb.py.  No GPU, no package import.

For a row x of n samples, the ``history`` samples that precede it in its recording, and the first ``taps`` samples of an impulse
response h:

    y[i] = sum_{k < taps} h[k] x[i - k],   0 <= i < n,   x[-1], x[-2], ... the history read backwards and 0 in front of it

which is ``np.convolve`` over the history-prefixed row, sliced: the ``scipy.signal.fftconvolve(clean, rir, "full")[:len(clean)]`` of the
DNS-Challenge synthesizer's ``add_pyreverb`` (tests/test_reverb_host.py pins the two against each other; parity with the package
itself is unpinned), applied to the whole recording and then cut where a segment is taken from a longer one.
"""
import numpy as np

from mix_ref import pcm16, ulp32  # noqa: F401  (ulp32 is used by the tests through this module)

# (n, K): one sample, a tap count one either side of the 16-tap block of the kernel, rows shorter than their response, the largest row
SHAPES = [(1, 1), (5, 16), (63, 17), (64, 15), (257, 33), (1025, 255), (1601, 1024), (3201, 4097), (4097, 257), (8193, 8192),
          (16385, 4097), (100, 4097), (12000, 16384)]
DYADIC_MAX_TAPS = 4097


def reverb(x, h, taps=None, history=()):
    """-> (y, S): y float64 [n] as above and S[i] = sum_k |h[k]| |x[i - k]|, the scale of the rounding error of any summation."""
    x = np.asarray(x, dtype=np.float64)
    hh = np.asarray(h, dtype=np.float64)[:taps]
    hist = np.asarray(history, dtype=np.float64)
    full = np.concatenate([hist, x])
    y = np.convolve(full, hh)[len(hist):len(hist) + len(x)]
    S = np.convolve(np.abs(full), np.abs(hh))[len(hist):len(hist) + len(x)]
    return y, S


def bound(K, S, y_dev, y_ref):
    """ulp32 + 2 K 2^-53 S[i]: one float32 rounding, and the first-order bound of two double sums of K exact terms in any order."""
    return np.maximum(ulp32(y_dev), ulp32(y_ref.astype(np.float32))) + 2.0 * K * 2.0 ** -53 * S


def speech_row(n, k):
    """A PCM16 row: values a 16-bit file holds, no negative zero among them (+ 0.0 turns -0.0 into +0.0)."""
    return pcm16(np.random.default_rng(8000 + k).standard_normal(n) / 4) + np.float32(0.0)


def rir_row(K, k):
    """A float32 impulse response: noise under an exponential decay (60 dB over the K taps), a pre-delay of K // 8 taps (at most 40)
    that holds noise 40 dB down, a unit peak behind it."""
    rng = np.random.default_rng(9000 + k)
    d = min(K // 8, 40)
    h = rng.standard_normal(K) * 0.3 * 10.0 ** (-3.0 * np.arange(K) / max(K, 2))
    h[:d] = 1e-2 * rng.standard_normal(d)
    h[d] = 1.0
    return h.astype(np.float32)


def dyadic_rir(K, k):
    """Taps that are multiples of 1/256 with |h| < 1, under a decaying envelope."""
    rng = np.random.default_rng(9500 + k)
    env = 10.0 ** (-2.0 * np.arange(K) / max(K, 2))
    h = np.round(np.clip(rng.standard_normal(K) * 0.4 * env, -0.99, 0.99) * 256) / 256
    return (h + 0.0).astype(np.float32)


def cases():
    """One (x, h) per entry of SHAPES."""
    return [(speech_row(n, k), rir_row(K, k)) for k, (n, K) in enumerate(SHAPES)]


def dyadic_cases():
    """PCM16 rows and dyadic taps at the shapes with K <= 4097."""
    return [(speech_row(n, 100 + k), dyadic_rir(K, k)) for k, (n, K) in enumerate(SHAPES) if K <= DYADIC_MAX_TAPS]
