"""Float64 numpy definition of the SNR mixer: the yardstick of tests/test_gpu_mix.py, tests/test_mix_host.py and
profiles/tools/measure_mix.py.  No GPU, no package import.

It restates ``normalize`` / ``snr_mixer`` / ``segmental_snr_mixer`` of the DNS-Challenge synthesizer for one row (parity with that
package is unpinned: it is not installed here), with one deliberate difference: a window's level is the true dB of its mean square,
10 log10(mean(v2^2) + EPS).  EPS = 2^-52.  For a clean row c of n samples and a noise row of m samples read cyclically from offset o,
v[i] = noise[(o + i) mod m]:

  1. c1 = c / (max|c| + EPS);  c2 = c1 10^(target_db / 20) / (rms(c1) + EPS);  the same for v1, v2;  rms over the n samples
  2. plain:      rc = rms(c2), rv = rms(v2)
     segmental:  [0, n) in windows of ``win`` samples (the last may be short); a window is active when 10 log10(mean(v2^2) + EPS) >
                 thresh_db over it; rc / rv = the root mean square of c2 / v2 over the samples of the active windows, both EPS if none is
  3. v3 = v2 rc / 10^(snr_db / 20) / (rv + EPS);  y = c2 + v3
  4. s = 10^(level_db / 20) / (rms(y) + EPS);  y, c2, v3 scaled by s
  5. max|y| > clip:  all three divided by max|y| / (clip - EPS), clipped = 1
  6. noisy, clean_out, noise_out as float32; g_clean, g_noise with clean_out = g_clean c, noise_out = g_noise v; the realised level
     20 log10(rms(y) + EPS) of the final y; clipped; the number of samples in active windows (n in plain mode)
"""
import numpy as np

EPS = 2.0 ** -52
TARGET_DB, CLIP, WIN, THRESH_DB = -25.0, 0.99, 1600, -50.0

# quad and wave edges, one sample either side of one and of two windows, the largest row of the GPU tests
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1599, 1600, 1601, 3199, 3200, 3201, 4097, 8193, 12000, 16385]
SNRS = (-5.0, 0.0, 20.0, 40.0)
LEVELS = (-35.0, -25.0, -15.0, -6.0)


def rms(x):
    return float(np.sqrt(np.mean(x * x)))


def cyclic(noise, n, offset):
    """v[i] = noise[(offset + i) mod m] for i < n."""
    noise = np.asarray(noise)
    return noise[(offset + np.arange(n)) % len(noise)]


def window_sums(x, win=WIN):
    """[ceil(n / win), 2] float64: max|x| and the sum of the squares of every window."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([[np.abs(x[s:s + win]).max(), np.sum(x[s:s + win] ** 2)] for s in range(0, len(x), win)])


def mix(clean, noise, offset, snr_db, level_db=-25.0, segmental=False, target_db=TARGET_DB, clip=CLIP, win=WIN, thresh_db=THRESH_DB):
    """One row -> dict: noisy / clean_out / noise_out (float32 and, as *_f64, before the cast), g_clean, g_noise, level_db, clipped,
    active, the raw statistics max_c, sum_c2, max_v, sum_v2, ``peak`` (max|y| after the level step, before the clip rule),
    ``window_db`` (the level of every window of v2), ``v`` (the noise as read) and ``cancel`` = sqrt(sum (|c2| + |v3|)^2 / sum y^2), the
    factor by which a rounding of c2 or v3 is amplified in rms(y): large where the two signals cancel."""
    c = np.asarray(clean, dtype=np.float64)
    n = len(c)
    v = cyclic(np.asarray(noise, dtype=np.float64), n, offset)
    t = 10.0 ** (target_db / 20.0)
    max_c, max_v = float(np.abs(c).max()), float(np.abs(v).max())
    c1 = c / (max_c + EPS)
    v1 = v / (max_v + EPS)
    kc = t / (rms(c1) + EPS)
    kv = t / (rms(v1) + EPS)
    c2 = c1 * kc
    v2 = v1 * kv
    g_c, g_v = kc / (max_c + EPS), kv / (max_v + EPS)
    window_db = np.array([10.0 * np.log10(np.mean(v2[s:s + win] ** 2) + EPS) for s in range(0, n, win)])
    if segmental:
        on = np.repeat(window_db > thresh_db, win)[:n]
        active = int(on.sum())
        rc, rv = (rms(c2[on]), rms(v2[on])) if active else (EPS, EPS)
    else:
        active = n
        rc, rv = rms(c2), rms(v2)
    k3 = rc / 10.0 ** (snr_db / 20.0) / (rv + EPS)
    v3 = v2 * k3
    g_v *= k3
    y = c2 + v3
    cancel = float(np.sqrt(np.sum((np.abs(c2) + np.abs(v3)) ** 2) / max(np.sum(y * y), 1e-300))) if y.any() else 1.0
    s = 10.0 ** (level_db / 20.0) / (rms(y) + EPS)
    y, c2, v3 = y * s, c2 * s, v3 * s
    g_c, g_v = g_c * s, g_v * s
    peak = float(np.abs(y).max())
    clipped = int(peak > clip)
    if clipped:
        div = peak / (clip - EPS)
        y, c2, v3 = y / div, c2 / div, v3 / div
        g_c, g_v = g_c / div, g_v / div
    return dict(noisy=y.astype(np.float32), clean_out=c2.astype(np.float32), noise_out=v3.astype(np.float32), noisy_f64=y, clean_f64=c2,
                noise_f64=v3, g_clean=g_c, g_noise=g_v, level_db=20.0 * np.log10(rms(y) + EPS), clipped=clipped, active=active,
                max_c=max_c, sum_c2=float(np.sum(c * c)), max_v=max_v, sum_v2=float(np.sum(v * v)), peak=peak, window_db=window_db,
                v=v, cancel=cancel)


def pcm16(x):
    """round(0.8 * 32767 * clip(x, -1, 1)) / 32768 as float32: values a 16-bit file holds."""
    return (np.round(0.8 * 32767 * np.clip(x, -1.0, 1.0)) / 32768).astype(np.float32)


def clean_row(n, k):
    return pcm16(np.random.default_rng(4000 + k).standard_normal(n) / 4)


def noise_len(n, k):
    return [n, max(1, n // 3), n + 7, 1][k % 4]


def noise_offset(m, k):
    return [0, m // 2, m - 1, 0][k % 4]


def noise_row(m, k, win=WIN):
    """PCM16 noise under an envelope of 1, 1e-2 and 0 that repeats every three windows of the noise row's own samples."""
    env = np.array([1.0, 1e-2, 0.0])[(np.arange(m) // win) % 3]
    return pcm16(np.random.default_rng(5002 + k).standard_normal(m) / 4 * env)


def cases():
    """One (clean, noise, offset) per entry of LENGTHS."""
    out = []
    for k, n in enumerate(LENGTHS):
        m = noise_len(n, k)
        out.append((clean_row(n, k), noise_row(m, k), noise_offset(m, k)))
    return out


def float_cases():
    """0.1 N(0, 1) float32 clean and noise rows at the same lengths and offsets."""
    out = []
    for k, n in enumerate(LENGTHS):
        m = noise_len(n, k)
        out.append(((0.1 * np.random.default_rng(6000 + k).standard_normal(n)).astype(np.float32),
                    (0.1 * np.random.default_rng(7000 + k).standard_normal(m)).astype(np.float32), noise_offset(m, k)))
    return out


def grid():
    """Every (snr_db, level_db, segmental) of the tests."""
    return [(snr, lev, seg) for seg in (False, True) for snr in SNRS for lev in LEVELS]


def clip_margin(r, clip=CLIP):
    """The distance of max|y| from the clip threshold: the decision can only differ below it."""
    return abs(r["peak"] - clip)


def window_margin_db(r, thresh_db=THRESH_DB):
    """The distance in dB of the window nearest to the activity threshold."""
    return float(np.abs(r["window_db"] - thresh_db).min())


def ulp32(x):
    """The float32 spacing at |x| (of the binade that holds it; the smallest subnormal at 0)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
