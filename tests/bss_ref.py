"""Host reference of the BSS-eval SDR / SIR / SAR with two sources (csrc/bss.hip, inference.compute_bss) in float64 numpy, the test
signals and the cases the BSS tests share.  A plain module: it calls nothing of the package under test.

The definition is ``bss_eval_sources`` of Vincent, Gribonval and Fevotte (2006) for a target and ONE interferer with distortion filters
of ``K`` taps, read for the target (``mir_eval.separation.bss_eval_sources(np.stack([s, v]), ..., compute_permutation=False)``, source 0).
For the target reference ``s``, the interferer reference ``v`` and the estimate ``y`` of ``L >= 1`` samples, all zero outside ``[0, L)``:

    x_ab[k] = sum_n a[n] b[n + k]                  k = -(K - 1) .. K - 1,  a, b in {s, v}
    d_a[k]  = sum_n a[n] y[n + k]                  k = 0 .. K - 1
    G = [[G_ss G_sv], [G_vs G_vv]],  G_ab[i][j] = x_ab[i - j]          (2K x 2K, symmetric)
    G_ss c = d_s                                   (K x K: the system of sdr_ref.sdr)
    G [C_s; C_v] = [d_s; d_v]
    p1   = c * s,   pall = C_s * s + C_v * v       over n = 0 .. L + K - 2
    SDR = 10 log10( sum p1^2 / sum (y - p1)^2 )    (= sdr_ref.sdr: the target part uses s alone)
    SIR = 10 log10( sum p1^2 / sum (pall - p1)^2 )
    SAR = 10 log10( sum pall^2 / sum (y - pall)^2 )

Each ratio: a zero numerator gives -inf, otherwise a zero denominator gives +inf.  Special rows, part of the definition here: a silent
reference gives three NaN; a silent interferer (``x_vv[0] == 0``), ``L <= K`` (``G`` has ``2K`` unknowns and ``L + K - 1`` equations,
so it is singular whatever the signals) and a pivot of the block Levinson recursion that is not positive definite (a numerically
singular ``G``, e.g. ``v = 2 s``) give the SDR of sdr_ref.sdr and NaN for SIR and SAR.  Rows shorter than about ``2K`` are overfitted
(a SAR of 293 dB at ``L = K + 1``, ``K = 16``): the cases stay off them except for the NaN rule.  Parity with the package itself is
pinned by tests/test_bss_host.py::test_bss_ref_matches_mir_eval where the package is installed.
"""
import numpy as np

import sdr_ref as S
from sdr_ref import CHANNEL, lag_sums, reference  # noqa: F401


def lags(s, v, y, K):
    """-> dict of the six lag sets for k = 0 .. K - 1 (x_ab[-k] = x_ba[k])."""
    return dict(ss=lag_sums(s, s, K), sv=lag_sums(s, v, K), vs=lag_sums(v, s, K), vv=lag_sums(v, v, K), ds=lag_sums(s, y, K),
                dv=lag_sums(v, y, K))


def _toeplitz(pos, neg):
    """T[i][j] = pos[i - j] for i >= j, neg[j - i] for i < j."""
    k = np.arange(len(pos))
    d = k[:, None] - k[None, :]
    return np.where(d >= 0, pos[np.abs(d)], neg[np.abs(d)])


def joint_matrix(lg):
    """The 2K x 2K matrix G of the definition."""
    return np.block([[_toeplitz(lg["ss"], lg["ss"]), _toeplitz(lg["sv"], lg["vs"])],
                     [_toeplitz(lg["vs"], lg["sv"]), _toeplitz(lg["vv"], lg["vv"])]])


def _posdef(E):
    return bool(E[0, 0] > 0 and E[1, 1] > 0 and E[0, 0] * E[1, 1] - E[0, 1] * E[1, 0] > 0)


def _inv2(E):
    q = 1.0 / (E[0, 0] * E[1, 1] - E[0, 1] * E[1, 0])
    return np.array([[E[1, 1] * q, -E[0, 1] * q], [-E[1, 0] * q, E[0, 0] * q]])


def block_levinson(lg):
    """The block Levinson recursion (Whittle 1963; Wiggins and Robinson 1965) on G reordered by interleaving the two sources: a
    symmetric block-Toeplitz matrix of the 2 x 2 blocks R_k = [[x_ss[k], x_sv[k]], [x_vs[k], x_vv[k]]], R_-k = R_k'.  F: the forward
    predictor, B: the backward predictor stored reversed, X: the solution.  -> (C_s, C_v), or None when an error matrix is not positive
    definite."""
    K = len(lg["ss"])
    R = np.stack([np.stack([lg["ss"], lg["sv"]], -1), np.stack([lg["vs"], lg["vv"]], -1)], -2)        # [K, 2, 2]
    D = np.stack([lg["ds"], lg["dv"]], -1)                                                               # [K, 2]
    if not _posdef(R[0]):
        return None
    F = np.zeros((K, 2, 2))
    B = np.zeros((K, 2, 2))
    X = np.zeros((K, 2))
    F[0] = B[0] = np.eye(2)
    Ef, Eb = R[0].copy(), R[0].copy()
    X[0] = _inv2(R[0]) @ D[0]
    for n in range(1, K):
        Rm = R[n:0:-1]                                                      # R_{n - j}, j = 0 .. n - 1
        Dl = np.einsum("jab,jbc->ac", Rm, F[:n])
        dx = np.einsum("jab,jb->a", Rm, X[:n])
        Kf, Kb = _inv2(Eb) @ Dl, _inv2(Ef) @ Dl.T
        Fo, Bo = F[:n + 1].copy(), B[:n + 1].copy()
        F[1:n + 1] -= Bo[n - 1::-1][:n] @ Kf                                # F_t -= B_{n - t} Kf, t = 1 .. n
        B[1:n + 1] -= Fo[n - 1::-1][:n] @ Kb
        Ef, Eb = Ef - Dl.T @ Kf, Eb - Dl @ Kb
        if not (_posdef(Ef) and _posdef(Eb)):
            return None
        mu = _inv2(Eb) @ (D[n] - dx)
        X[:n + 1] += B[n::-1] @ mu                                          # X_t += B_{n - t} mu, t = 0 .. n
    return X[:, 0].copy(), X[:, 1].copy()


def _db(num, den):
    if num == 0:
        return -np.inf
    if den == 0:
        return np.inf
    return float(10 * np.log10(num / den))


def bss(x_ref, x_interf, x_est, K=512, solver="lu"):
    """-> dict(sdr, sir, sar, filters [2, K], target_energy, error_energy, interf_energy, projection_energy, artif_energy, lags).
    ``solver``: "lu" (``np.linalg.solve`` on the 2K x 2K matrix, the yardstick) or "levinson" (:func:`block_levinson`)."""
    s, v, y = (np.asarray(a, dtype=np.float64) for a in (x_ref, x_interf, x_est))
    if s.ndim != 1 or s.shape != y.shape or s.shape != v.shape or len(s) < 1:
        raise ValueError("three 1-D signals of one length >= 1 expected")
    if solver not in ("lu", "levinson"):
        raise ValueError(f"solver {solver!r}")
    L = len(s)
    one = S.sdr(s, y, K)
    lg = lags(s, v, y, K)
    nan = float("nan")
    out = dict(sdr=one["sdr"], sir=nan, sar=nan, filters=np.full((2, K), nan), target_energy=one["target_energy"],
               error_energy=one["error_energy"], interf_energy=nan, projection_energy=nan, artif_energy=nan, lags=lg, filter=one["filter"])
    if lg["ss"][0] == 0 or lg["vv"][0] == 0 or L <= K:
        return out
    lev = block_levinson(lg)
    if lev is None:
        return out
    if solver == "lu":
        sol = np.linalg.solve(joint_matrix(lg), np.concatenate([lg["ds"], lg["dv"]]))
        cs, cv = sol[:K], sol[K:]
    else:
        cs, cv = lev
    p1 = np.convolve(one["filter"], s)
    pall = np.convolve(cs, s) + np.convolve(cv, v)
    ypad = np.concatenate([y, np.zeros(K - 1)])
    ei, ea = pall - p1, ypad - pall
    ti, tp, ta = float(np.sum(ei * ei)), float(np.sum(pall * pall)), float(np.sum(ea * ea))
    out.update(sir=_db(one["target_energy"], ti), sar=_db(tp, ta), filters=np.stack([cs, cv]), interf_energy=ti, projection_energy=tp,
               artif_energy=ta)
    return out


def condition(lg):
    return float(np.linalg.cond(joint_matrix(lg)))


def residual(filters, lg):
    """The joint normal-equation residual max |G C - D| / x_ss[0] of the filters [2, K] in float64."""
    c = np.asarray(filters, dtype=np.float64).reshape(-1)
    return float(np.max(np.abs(joint_matrix(lg) @ c - np.concatenate([lg["ds"], lg["dv"]]))) / lg["ss"][0])


# ----------------------------------------------------------------------------- signals (float32 values: what the device is given)
PATH = np.array([0.0, 0.7, 0.3, 0.0, 0.0, -0.2])                            # the interferer's way into the estimate
SNRS = (60, 20, 0)                                                          # white artifacts under the target's energy, dB
# the interferer's gain into the estimate, paired with the artifacts so that no SIR rests on rounding: -20 dB beside the 60 dB
# artifacts, 0 dB beside the 20 dB ones, none beside the 0 dB ones (there the artifacts' own projection on v is the interference)
GAINS = {60: 0.1, 20: 1.0, 0: 0.0}
_SHAPES = {16: (24, 31, 32, 33, 257), 64: (96, 127, 128, 129, 257, 4001), 512: (768, 1023, 1024, 1025, 4082, 16385)}
# (L, K, kind): one short of, at and one past 2 K, at the 16-sample block and the 256-lag tile, the 4081 / 4082 edge of the lag tiles,
# more than one 4096-sample tile of either tiled pass
CASES = [(L, K, ("white", "lowpass")[j % 2]) for K in sorted(_SHAPES) for j, L in enumerate(_SHAPES[K])]


def case_snr(index):
    """The artifacts' level of CASES[index]: SNRS walked from the longest row of each K down, so the longest has the 60 dB."""
    L, K, _ = CASES[index]
    return SNRS[(len(_SHAPES[K]) - 1 - _SHAPES[K].index(L)) % 3]


def mixture(ref, interf, snr_db, gain, seed=0):
    """The target through CHANNEL plus ``gain`` times the interferer through PATH, both cut to the length, plus white artifacts
    ``snr_db`` under the TARGET's energy, as float32."""
    s, v = np.asarray(ref, dtype=np.float64), np.asarray(interf, dtype=np.float64)
    nz = np.random.default_rng(3000 + seed).standard_normal(len(s))
    g = np.sqrt(np.sum(s * s) / (np.sum(nz * nz) * 10 ** (snr_db / 10)))
    return (np.convolve(s, CHANNEL)[:len(s)] + gain * np.convolve(v, PATH)[:len(s)] + g * nz).astype(np.float32)


def case_signals(index):
    """(target reference, interferer reference, estimate) of CASES[index], float32."""
    L, K, kind = CASES[index]
    other = "lowpass" if kind == "white" else "white"
    s = reference(L, kind, seed=index)
    v = (0.5 * reference(L, other, seed=100 + index).astype(np.float64)).astype(np.float32)
    snr = case_snr(index)
    return s, v, mixture(s, v, snr, GAINS[snr], seed=index)
