"""Host reference of STOI / ESTOI (csrc/stoi.hip, inference.compute_stoi) in numpy / scipy, the test signals and the cases the
STOI tests share.  A plain module: it calls nothing of the package under test.

The definition is the published algorithms (Taal et al. 2011 for STOI, Jensen & Taal 2016 for ESTOI) with the constants and the
framing of the ``pystoi`` package: 10 kHz, 256-sample hanning(258)[1:-1] frames at hop 128 over the EXCLUSIVE range
``range(0, len - 256, 128)``, 40 dB silent-frame removal on the clean signal, 512-point DFT, 15 third-octave bands from 150 Hz,
30-frame segments, -15 dB clipping.  ``stoi(x_ref, x_est, fs, extended, dtype)``: ``dtype=np.float64`` is the yardstick;
``dtype=np.float32`` runs every stage in float32 with the DFT as a float32 matrix product, i.e. the yardstick's own rounding floor.
Parity with the package itself is pinned by tests/test_stoi_host.py::test_stoi_ref_matches_pystoi where the package is installed.
"""
import numpy as np

EPS = 2.220446049250313e-16          # float64's machine epsilon, in every dtype
FS = 10000
N_FRAME, HOP, NFFT = 256, 128, 512
NUMBAND, MINFREQ, N_SEG = 15, 150, 30
BETA, DYN_RANGE = -15.0, 40.0
BAND_LO = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
BAND_HI = [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]


# ----------------------------------------------------------------------------- tables
def fir_taps():
    """The 581 taps of the 16 kHz -> 10 kHz anti-aliasing filter (p = 5, q = 8), summing to 1."""
    fc = 1.0 / 16
    half = int(np.ceil((60 - 8) / (28.714 * fc / 10)))
    assert half == 290
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60 - 8.7)) * (2 * 5 * fc * np.sinc(2 * fc * t))
    return h / np.sum(h)


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def band_edges():
    """(lo, hi) bins of the 15 third-octave bands: the bins of the 512-point DFT at 10 kHz nearest to the band edges."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND, dtype=float)
    freq_low = MINFREQ * np.power(2.0, (2 * k - 1) / 6)
    freq_high = MINFREQ * np.power(2.0, (2 * k + 1) / 6)
    lo = [int(np.argmin(np.square(f - v))) for v in freq_low]
    hi = [int(np.argmin(np.square(f - v))) for v in freq_high]
    return lo, hi


def resample_written_out(x):
    """out[n] = 5 * sum_j x[j] * h[290 + 8 n - 5 j]: what the device kernel evaluates (float64 here)."""
    x = np.asarray(x, dtype=np.float64)
    h = fir_taps()
    n_out = -(-5 * len(x) // 8)
    out = np.zeros(n_out)
    for n in range(n_out):
        j0 = max(0, -(-(8 * n - 290) // 5))
        j1 = min(len(x) - 1, (8 * n + 290) // 5)
        j = np.arange(j0, j1 + 1)
        out[n] = 5.0 * np.sum(x[j] * h[290 + 8 * n - 5 * j])
    return out


def resample(x, dtype=np.float64):
    from scipy.signal import resample_poly
    return resample_poly(np.asarray(x, dtype=dtype), 5, 8, window=fir_taps().astype(dtype)).astype(dtype)


# ----------------------------------------------------------------------------- the pipeline
def _frames(x, w):
    starts = range(0, len(x) - N_FRAME, HOP)
    if len(starts) == 0:
        return np.zeros((0, N_FRAME), dtype=x.dtype)
    return np.stack([w * x[i:i + N_FRAME] for i in starts])


def _ola(frames):
    out = np.zeros((len(frames) - 1) * HOP + N_FRAME, dtype=frames.dtype)
    for k in range(len(frames)):
        out[k * HOP:k * HOP + N_FRAME] += frames[k]
    return out


def stoi(x_ref, x_est, fs=16000, extended=False, dtype=np.float64):
    """-> (score, (frames, kept frames, segments), mask margin in dB).  x_ref: clean, x_est: processed (the package's order).
    The margin is min_i |max(e) - 40 - e_i| over the clean signal's frame energies e (inf when there is no frame)."""
    if fs not in (10000, 16000):
        raise ValueError(f"fs = {fs}: 10000 or 16000 expected")
    dt = np.dtype(dtype).type
    x = np.asarray(x_ref, dtype=dtype)
    y = np.asarray(x_est, dtype=dtype)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("two 1-D signals of one length expected")
    if fs == 16000:
        x, y = resample(x, dtype), resample(y, dtype)
    w = window().astype(dtype)
    xf, yf = _frames(x, w), _frames(y, w)
    n_frames = len(xf)
    if n_frames == 0:
        return 1e-5, (0, 0, 0), float("inf")
    e = (dt(20) * np.log10(np.sqrt(np.sum(xf * xf, axis=1, dtype=dtype)) + dt(EPS))).astype(dtype)
    thr = e.max() - dt(DYN_RANGE)
    keep = (thr - e) < 0
    margin = float(np.min(np.abs((thr - e).astype(np.float64))))
    kept = int(keep.sum())
    xs, ys = _ola(xf[keep]), _ola(yf[keep])
    x2, y2 = _frames(xs, w), _frames(ys, w)
    assert len(x2) == kept - 1
    if kept - 1 < N_SEG:
        return 1e-5, (n_frames, kept, 0), margin
    if dt is np.float64:
        X = np.fft.rfft(x2, NFFT, axis=1)
        Y = np.fft.rfft(y2, NFFT, axis=1)
        px, py = np.abs(X) ** 2, np.abs(Y) ** 2
    else:                                                   # the DFT as a matrix product in the working precision
        ang = 2 * np.pi * ((np.arange(N_FRAME)[:, None] * np.arange(NFFT // 2 + 1)[None, :]) % NFFT) / NFFT
        c, s = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
        xr, xi, yr, yi = x2 @ c, x2 @ s, y2 @ c, y2 @ s
        px, py = xr * xr + xi * xi, yr * yr + yi * yi
    tx = np.stack([np.sqrt(np.sum(px[:, lo:hi], axis=1, dtype=dtype)) for lo, hi in zip(BAND_LO, BAND_HI)]).astype(dtype)
    ty = np.stack([np.sqrt(np.sum(py[:, lo:hi], axis=1, dtype=dtype)) for lo, hi in zip(BAND_LO, BAND_HI)]).astype(dtype)
    n2 = tx.shape[1]
    segs = list(range(N_SEG, n2 + 1))
    xseg = np.stack([tx[:, m - N_SEG:m] for m in segs])     # [M, 15, 30]
    yseg = np.stack([ty[:, m - N_SEG:m] for m in segs])
    M = len(segs)
    eps = dt(EPS)
    if extended:
        def rc(a):
            a = a - np.mean(a, axis=2, keepdims=True, dtype=dtype)
            a = a / (np.sqrt(np.sum(a * a, axis=2, keepdims=True, dtype=dtype)) + eps)
            a = a - np.mean(a, axis=1, keepdims=True, dtype=dtype)
            return a / (np.sqrt(np.sum(a * a, axis=1, keepdims=True, dtype=dtype)) + eps)
        score = np.sum(rc(xseg) * rc(yseg), dtype=dtype) / dt(N_SEG) / dt(M)
    else:
        nrm = lambda a: np.sqrt(np.sum(a * a, axis=2, keepdims=True, dtype=dtype))
        c = nrm(xseg) / (nrm(yseg) + eps)
        yp = np.minimum(yseg * c, xseg * dt(1 + 10 ** (-BETA / 20)))
        yp = yp - np.mean(yp, axis=2, keepdims=True, dtype=dtype)
        xm = xseg - np.mean(xseg, axis=2, keepdims=True, dtype=dtype)
        yp = yp / (nrm(yp) + eps)
        xm = xm / (nrm(xm) + eps)
        score = np.sum(yp * xm, dtype=dtype) / dt(NUMBAND * M)
    return float(score), (n_frames, kept, M), margin


def rmse(x_est, x_ref):
    """utils/eval_metrics.py:33-41 in float64."""
    e, r = np.asarray(x_est, dtype=np.float64), np.asarray(x_ref, dtype=np.float64)
    alpha = np.sum(e * r) / np.sum(e ** 2)
    return float(np.sqrt(np.square(alpha * e - r).mean()))


# ----------------------------------------------------------------------------- test signals (16 kHz)
def _carrier(n):
    t = np.arange(n) / 16000.0
    f0 = 120 + 30 * np.sin(2 * np.pi * 1.3 * t)
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    return t, sum(np.sin(k * ph) / k for k in range(1, 25))


def speech(n, seed=0):
    """24 harmonics of f0 = 120 + 30 sin(2 pi 1.3 t), amplitudes 1/k, a syllable envelope with pauses, a 1e-3 white floor."""
    t, c = _carrier(n)
    env = np.clip(np.sin(2 * np.pi * 3.1 * t), 0, None) ** 2 * (1 + 0.5 * np.sin(2 * np.pi * 0.7 * t))
    return c * env + 1e-3 * np.random.default_rng(seed).standard_normal(n)


def steady(n, seed=0):
    """The same carrier without pauses."""
    t, c = _carrier(n)
    return c * (1 + 0.5 * np.sin(2 * np.pi * 2.3 * t))


def noisy(x, snr_db, seed=1):
    nz = np.random.default_rng(seed).standard_normal(len(x))
    g = np.sqrt(np.sum(x ** 2) / (np.sum(nz ** 2) * 10 ** (snr_db / 10)))
    return x + g * nz


# (name, generator, samples): the smallest shapes at which each stage can still go wrong; "one_segment" keeps exactly 31 frames;
# "many_blocks" has 282 frames (more than one 256-frame chunk of the device's prefix sum, frames kept in the second chunk), 134
# second-stage frames (5 spectrum workgroups) and 105 segments (4 segment workgroups, whose partials are folded per row)
CASES = [("compaction", speech, 16000), ("near_30", speech, 12345), ("too_few", speech, 11000), ("range_edge", steady, 8601),
         ("range_next", steady, 8602), ("longer", speech, 24000), ("one_segment", speech, 12064), ("many_blocks", speech, 58029)]
SNRS = (20, 0, -5)
