"""The image-source room impulse response of DESIGN.md 3.20 in float64 numpy: the yardstick of csrc/ism.hip and dataset/rir.py
(Allen & Berkley 1979 for a rectangular room; parity with pyroomacoustics, gpuRIR or torchaudio is unpinned).

A room: size L[3], source s[3] and microphone r[3] inside it, beta[a][0] the reflection coefficient of the wall at coordinate 0 of axis
a and beta[a][1] that of the wall at L[a].  Image (m, q) of axis a lies at p = 2 m L + (1 - 2 q) s - r, was reflected e0 = |m - q|
times at the wall at 0 and e1 = |m| times at the far wall and carries g = beta0^e0 beta1^e1 (x^0 = 1).  With d = |p|, A = gx gy gz /
(4 pi d), tau = d fs / c, n_i = rint(tau), f = tau - n_i, u = n - tau:

    h[n] = float32( sum_i A sinc(u) (1 + cos(2 pi u / W)) / 2 ),  |u| < W / 2,  W = 81,  0 <= n < K
    sinc(0) = 1,  sinc(u) = (-1)^(n - n_i + 1) sin(pi f) / (pi u)

over the images with tau < K - 1 + W / 2 (and e0 + e1 summed over the axes <= max_order where one is given); A = 0 adds nothing.

The ORDER of the operations that decide tau is part of the definition, so that the device reproduces tau, u and f bit for bit:
p = ((2 m) L + (+-s)) - r,  d = sqrt((px px + py py) + pz pz),  tau = (d fs) / c, every step one IEEE double operation."""
import math

import numpy as np

W = 81
HALF = W / 2.0
REACH = 41                     # |n - n_i| <= 41 wherever |u| < 40.5


def axis_images(L, s, r, b0, b1, dmax):
    """(p, e0 + e1, g) of every image of one axis with |m| <= floor(dmax / 2L) + 1, q = 0 then 1 for each m."""
    M = int(math.floor(dmax / (2.0 * L))) + 1
    m = np.repeat(np.arange(-M, M + 1), 2)
    q = np.tile(np.array([0, 1]), 2 * M + 1)
    sgn_s = np.where(q == 0, s, -s)
    p = ((2.0 * m) * L + sgn_s) - r
    e0, e1 = np.abs(m - q), np.abs(m)
    with np.errstate(all="ignore"):
        g = np.power(float(b0), e0.astype(np.float64)) * np.power(float(b1), e1.astype(np.float64))
    return p, e0 + e1, g


def images(L, s, r, beta, K, fs=16000.0, c=343.0, max_order=None):
    """(tau, A) of the image set, float64 arrays."""
    L, s, r = (np.asarray(v, dtype=np.float64).reshape(3) for v in (L, s, r))
    beta = np.asarray(beta, dtype=np.float64).reshape(3, 2)
    fs, c = float(fs), float(c)
    tmax = K - 1 + HALF
    dmax = tmax * c / fs
    ax = [axis_images(L[a], s[a], r[a], beta[a, 0], beta[a, 1], dmax) for a in range(3)]
    (px, ox, gx), (py, oy, gy), (pz, oz, gz) = ax
    taus, amps = [], []
    yy = (py * py)[:, None]
    zz = (pz * pz)[None, :]
    for i in range(px.shape[0]):
        if abs(px[i]) >= dmax:
            continue
        d = np.sqrt((px[i] * px[i] + yy) + zz)
        tau = d * fs / c
        keep = tau < tmax
        if max_order is not None:
            keep &= (ox[i] + oy[:, None] + oz[None, :]) <= max_order
        with np.errstate(all="ignore"):
            A = ((gx[i] * gy)[:, None] * gz[None, :]) / ((4.0 * np.pi) * d)
        keep &= A != 0.0
        taus.append(tau[keep])
        amps.append(A[keep])
    if not taus:
        return np.zeros(0), np.zeros(0)
    return np.concatenate(taus), np.concatenate(amps)


def window(u):
    return 0.5 * (1.0 + np.cos(2.0 * np.pi * u / W))


def rir(L, s, r, beta, K, fs=16000.0, c=343.0, max_order=None, detail=False):
    """h float32 [K]; with ``detail`` also (the double sums, N_n = the images touching sample n, S_n = sum |A| w(n), the image count)."""
    tau_all, A_all = images(L, s, r, beta, K, fs, c, max_order)
    j = np.arange(-REACH, REACH + 1)
    sign = np.where((j + 1) % 2 == 0, 1.0, -1.0)[None, :]
    h64, N, S = np.zeros(K), np.zeros(K, dtype=np.int64), np.zeros(K)
    for lo in range(0, tau_all.shape[0], 1 << 16):                  # blocks of images: the memory stays small
        tau, A = tau_all[lo:lo + (1 << 16)], A_all[lo:lo + (1 << 16)]
        ni = np.rint(tau)
        f = tau - ni
        n = ni[:, None].astype(np.int64) + j[None, :]
        u = n - tau[:, None]
        ok = (np.abs(u) < HALF) & (n >= 0) & (n < K)
        with np.errstate(all="ignore"):
            sinc = np.where(u == 0.0, 1.0, sign * np.sin(np.pi * f)[:, None] / (np.pi * u))
        w = window(u)
        term = A[:, None] * sinc * w
        idx = n[ok]
        h64 += np.bincount(idx, weights=term[ok], minlength=K)[:K]
        if detail:
            N += np.bincount(idx, minlength=K)[:K]
            S += np.bincount(idx, weights=(np.abs(A)[:, None] * w)[ok], minlength=K)[:K]
    h = h64.astype(np.float32)
    if not detail:
        return h
    return h, h64, N, S, int(tau_all.shape[0])


def ulp32(x):
    """The spacing of float32 at |x| (that of the smallest normal below it)."""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)
