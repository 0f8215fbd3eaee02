"""Host definition of the latent-space report (i-dccrn-vae_amd/latent.py): the project's own numpy restatement of what the reference's
pretrained_vaes/test_prevae.py and nsvae_dccrn/test_nsvae_se.py compute per utterance and over the test set.  Every function takes a
``dtype``: float64 is the yardstick of the GPU tests, float32 repeats the reference's arithmetic and gives its rounding floor.
tests/golden/latent_report.npz holds what the reference's own functions returned for a small fixture (test_latent_host.py)."""
import numpy as np

STAT_KEYS = ("kl",) + tuple(f"{v}{s}" for v in ("vrr", "vri", "vii") for s in ("_min", "_max", "_mean", ""))
DIST_KEYS = ("dis_mean", "dis_sigma", "dis_delta")
COV_KEYS = ("cov_rr", "cov_ri", "cov_ii")


def make_inputs(shape, seed):
    """(miu, log_sigma, delta) float32 [*shape, 2]: miu ~ N(0, 1) + 0.5 (a mean exists to cancel); log_sigma real ~ U(-1.5, 1), its
    imaginary channel NaN (nobody may read it); delta = rho sigma e^{i phi} with rho ~ U(0, 0.9) for half of the elements and
    U(1.05, 2) for the other half, so both branches of the guard |delta| >= sigma - 1e-3 are taken and none is near its threshold."""
    rng = np.random.default_rng(seed)
    shape = tuple(shape)
    miu = (rng.standard_normal(shape + (2,)) + 0.5).astype(np.float32)
    ls = np.full(shape + (2,), np.nan, dtype=np.float32)
    ls[..., 0] = rng.uniform(-1.5, 1.0, shape)
    sigma = np.exp(ls[..., 0].astype(np.float64))
    big = rng.permutation(int(np.prod(shape))).reshape(shape) % 2 == 1
    rho = np.where(big, rng.uniform(1.05, 2.0, shape), rng.uniform(0.0, 0.9, shape))
    phi = rng.uniform(0.0, 2 * np.pi, shape)
    dl = np.stack([rho * sigma * np.cos(phi), rho * sigma * np.sin(phi)], axis=-1).astype(np.float32)
    return miu, ls, dl


def nan_past(x, frames):
    """A copy of x [B, T, ...] with NaN at and past frames[b] of every row."""
    x = x.copy()
    for b, n in enumerate(frames):
        x[b, n:] = np.nan
    return x


def guard_facts(ls, dl):
    """-> (share of elements that take the guard, the smallest distance of |delta|' to the threshold sigma - 1e-3), in float64."""
    sigma = np.exp(ls[..., 0].astype(np.float64))
    a = np.sqrt(dl[..., 0].astype(np.float64) ** 2 + dl[..., 1].astype(np.float64) ** 2 + 1e-6)
    return float(np.mean(a >= sigma - 1e-3)), float(np.min(np.abs(a - (sigma - 1e-3))))


def var_matrices(ls, dl, dtype=np.float64):
    """-> sigma, guarded delta_real, delta_imag, vrr, vri, vii for log_sigma / delta [..., 2]."""
    c = np.dtype(dtype).type
    sigma = np.exp(ls[..., 0].astype(dtype))
    dr, di = dl[..., 0].astype(dtype), dl[..., 1].astype(dtype)
    a = np.sqrt(dr * dr + di * di + c(1e-6))
    temp = sigma * c(0.99) / (a + c(1e-6))
    take = a >= sigma - c(1e-3)
    dr = np.where(take, dr * temp, dr)
    di = np.where(take, di * temp, di)
    return sigma, dr, di, c(0.5) * (sigma + dr), c(0.5) * di, c(0.5) * (sigma - dr)


def posterior_stats(miu, ls, dl, dtype=np.float64):
    """One utterance [T, z, 2] -> {key: value}: the thirteen numbers of latent.posterior_stats."""
    c = np.dtype(dtype).type
    sigma, dr, di, vrr, vri, vii = var_matrices(ls, dl, dtype)
    mr, mi = miu[..., 0].astype(dtype), miu[..., 1].astype(dtype)
    miu_h_miu = np.sum(mr * mr + mi * mi, axis=1, dtype=dtype)
    lg = np.log(sigma * sigma - (dr * dr + di * di) + c(1e-6))
    per_frame = miu_h_miu + np.sum(np.abs(sigma - c(1) - c(0.5) * lg), axis=1, dtype=dtype)
    out = {"kl": np.mean(per_frame, dtype=dtype)}
    for k, v in (("vrr", vrr), ("vri", vri), ("vii", vii)):
        m = np.mean(np.abs(v), axis=0, dtype=dtype)
        out[k + "_min"], out[k + "_max"] = np.min(v), np.max(v)
        out[k + "_mean"] = np.mean(m, dtype=dtype)
        out[k] = np.sqrt(np.sum(m * m, dtype=dtype))
    return {k: float(v) for k, v in out.items()}


def pair_distance(a, b, dtype=np.float64):
    """a, b: (miu, log_sigma, delta) of one utterance [T, z, 2] -> dis_mean, dis_sigma, dis_delta."""
    def dist(v1, v2):
        res = np.mean((v1 - v2) ** 2, axis=0, dtype=dtype)
        return float(np.sqrt(np.sum(res, dtype=dtype)))
    return {"dis_mean": dist(a[0].astype(dtype), b[0].astype(dtype)),
            "dis_sigma": dist(np.exp(a[1][..., 0].astype(dtype)), np.exp(b[1][..., 0].astype(dtype))),
            "dis_delta": dist(a[2].astype(dtype), b[2].astype(dtype))}


def miu_cov(mius, dtype=np.float64):
    """mius: list of [T_k, z, 2] arrays (the valid frames of every utterance) -> the dictionary of MiuMoments.result()."""
    real = np.vstack([m[..., 0] for m in mius]).astype(dtype)
    imag = np.vstack([m[..., 1] for m in mius]).astype(dtype)
    n = np.dtype(dtype).type(real.shape[0])
    mean_r = np.mean(real, axis=0, keepdims=True, dtype=dtype)
    mean_i = np.mean(imag, axis=0, keepdims=True, dtype=dtype)
    cr, ci = real - mean_r, imag - mean_i
    return {"n": float(n), "mean_real": mean_r[0], "mean_imag": mean_i[0], "cov_rr": np.matmul(cr.T, cr) / n,
            "cov_ri": np.matmul(cr.T, ci) / n, "cov_ii": np.matmul(ci.T, ci) / n,
            "mean_dis": float(np.sqrt(np.sum(mean_r ** 2 + mean_i ** 2, dtype=dtype)))}


def cov_scale(mius):
    """(sum_n |x_i| |x_j|) / n for the three blocks, float64: what the covariance bounds of the GPU tests are relative to."""
    real = np.abs(np.vstack([m[..., 0] for m in mius]).astype(np.float64))
    imag = np.abs(np.vstack([m[..., 1] for m in mius]).astype(np.float64))
    n = real.shape[0]
    return {"cov_rr": real.T @ real / n, "cov_ri": real.T @ imag / n, "cov_ii": imag.T @ imag / n,
            "mean_real": real.mean(axis=0), "mean_imag": imag.mean(axis=0)}


def cov_summary(cov_rr, cov_ri, cov_ii):
    """The log numbers of test_prevae.py for three [z, z] matrices (the keys of latent.cov_summary)."""
    out = {}
    for k, c in (("rr", cov_rr), ("ri", cov_ri), ("ii", cov_ii)):
        z = c.shape[0]
        diag = np.diagonal(c, 0)
        off = c - np.diag(diag)
        out[f"diag_abs_{k}"] = float(np.sum(np.abs(diag)) / z)
        out[f"diag_max_{k}"] = float(np.max(diag))
        out[f"diag_min_{k}"] = float(np.min(diag))
        out[f"diag_mean_{k}"] = float(np.mean(diag))
        out[f"offdiag_abs_{k}"] = float(np.sum(np.abs(off)) / (z * (z - 1)))
    return out


def silhouette(set1, set2, dtype=np.float64):
    """set1 [N1, z, 2], set2 [N2, z, 2] -> sc, mean_dis, var_avg_1, var_avg_2 as latent.silhouette returns them."""
    s1, s2 = set1.astype(dtype), set2.astype(dtype)
    m1 = np.mean(s1, axis=0, keepdims=True, dtype=dtype)
    m2 = np.mean(s2, axis=0, keepdims=True, dtype=dtype)

    def score(s, own, other):
        intra = np.sqrt(np.sum((s - own) ** 2, axis=(1, 2), dtype=dtype))
        inter = np.sqrt(np.sum((s - other) ** 2, axis=(1, 2), dtype=dtype))
        return (inter - intra) / np.maximum(intra, inter)
    sc = np.concatenate((score(s1, m1, m2), score(s2, m2, m1)))
    v1 = np.mean(np.var(s1, axis=0, dtype=dtype), axis=0, dtype=dtype)
    v2 = np.mean(np.var(s2, axis=0, dtype=dtype), axis=0, dtype=dtype)
    return {"sc": float(np.mean(sc, dtype=dtype)), "mean_dis": float(np.sum((m1 - m2) ** 2, dtype=dtype)),
            "var_avg_1": (float(v1[0]), float(v1[1])), "var_avg_2": (float(v2[0]), float(v2[1]))}
