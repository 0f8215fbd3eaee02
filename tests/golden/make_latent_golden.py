"""Writes tests/golden/latent_report.npz: what the reference's own evaluation functions return for a small seeded fixture.

    python tests/golden/make_latent_golden.py --reference /path/to/i_dccrn_vae

Needs a checkout of the reference; it is run once, by hand, where one exists.  pretrained_vaes/test_prevae.py and
nsvae_dccrn/test_nsvae_se.py import librosa, soundfile and sklearn at the top and cannot be imported without them, so the
definitions of ``cal_var_matrices``, ``complex_kl``, ``distance`` and ``simple_silhouette_score`` are read out of the two files with
``ast`` and executed here; the per-utterance summaries and the covariance block, which the scripts compute inline in ``run``, are
their torch / numpy expressions applied to the fixture.  Nothing of the reference's text goes into the file: the inputs (seeded
by tests/latent_ref.make_inputs) and the recorded float32 results only.

The seeds: a covariance entry is a cancelling sum of 12 float32 products, so the relative rounding error of the reference's float32
matmul is not bounded for an entry that happens to come out near zero; about every second seed has such an entry with more than the
1e-5 the host test allows per value.  13 is the first seed from 11 on whose float32 covariance stays within 1e-5 of the float64
one in every entry (8.2e-6 at the worst), so the comparison measures the formulas and not that cancellation.

Fixture: the scripts' batch of 1, three utterances of T = 7, 4 and 1 frames, zdim = 16, two posteriors ("a": the clean encoder's /
the speech latent, "b": the noisy encoder's / the noise latent)."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import latent_ref as R  # noqa: E402

FRAMES, ZDIM = (7, 4, 1), 16
STAT_KEYS, DIST_KEYS = R.STAT_KEYS, R.DIST_KEYS


def reference_functions(path, names):
    """The named top-level functions of a reference script, executed in a namespace that holds torch and numpy only."""
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in keep) == sorted(names), (path, [n.name for n in keep])
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (the folder that holds pretrained_vaes/ and nsvae_dccrn/)")
    ap.add_argument("--out", default=os.path.join(HERE, "latent_report.npz"))
    a = ap.parse_args()
    cal_var_matrices, complex_kl = reference_functions(os.path.join(a.reference, "pretrained_vaes", "test_prevae.py"),
                                                       ["cal_var_matrices", "complex_kl"])
    distance, simple_silhouette_score = reference_functions(os.path.join(a.reference, "nsvae_dccrn", "test_nsvae_se.py"),
                                                            ["distance", "simple_silhouette_score"])
    T = max(FRAMES)
    save = {"frames": np.asarray(FRAMES, dtype=np.int64)}
    post = {}
    for tag, seed in (("a", 13), ("b", 14)):
        post[tag] = R.make_inputs((len(FRAMES), T, ZDIM), seed)
        for name, arr in zip(("miu", "log_sigma", "delta"), post[tag]):
            save[f"{name}_{tag}"] = R.nan_past(arr, FRAMES)

    stats = np.zeros((len(FRAMES), len(STAT_KEYS)), dtype=np.float32)
    dists = np.zeros((len(FRAMES), len(DIST_KEYS)), dtype=np.float32)
    miu_real, miu_imag = [], []
    for k, n in enumerate(FRAMES):
        ta, tb = ([torch.from_numpy(x[k:k + 1, :n].copy()) for x in post[t]] for t in ("a", "b"))
        miu, log_sigma, delta = ta
        # test_prevae.py:171-197
        got = {}
        vrr, vri, _, vii = cal_var_matrices(log_sigma, delta)
        for key, v in (("vrr", vrr), ("vri", vri), ("vii", vii)):
            got[key + "_min"], got[key + "_max"] = torch.min(v), torch.max(v)
            m = torch.mean(torch.mean(torch.abs(v), dim=0), dim=0)
            got[key + "_mean"] = torch.mean(m)
            got[key] = torch.sqrt(torch.sum(m.pow(2)))
        got["kl"] = complex_kl(miu, log_sigma, delta)
        stats[k] = [float(got[key]) for key in STAT_KEYS]
        # test_nsvae_se.py:416-418
        dists[k] = [float(distance(ta[0], tb[0], False)), float(distance(ta[1], tb[1], True)), float(distance(ta[2], tb[2], False))]
        # test_prevae.py:204-207
        m = miu.view(miu.shape[0] * miu.shape[1], miu.shape[2], miu.shape[3]).numpy()
        miu_real.append(m[..., 0])
        miu_imag.append(m[..., 1])
    save["stats"], save["dists"] = stats, dists

    # test_prevae.py:285-323
    miu_real_array, miu_imag_array = np.vstack(miu_real), np.vstack(miu_imag)
    numvecs = miu_real_array.shape[0]
    miu_real_mean = np.mean(miu_real_array, axis=0, keepdims=True)
    miu_imag_mean = np.mean(miu_imag_array, axis=0, keepdims=True)
    save["mean_dis"] = np.float32(np.sqrt(np.sum(miu_real_mean ** 2 + miu_imag_mean ** 2)))
    center_miu_real, center_miu_imag = miu_real_array - miu_real_mean, miu_imag_array - miu_imag_mean
    save["cov_rr"] = np.matmul(center_miu_real.T, center_miu_real) / numvecs
    save["cov_ri"] = np.matmul(center_miu_real.T, center_miu_imag) / numvecs
    save["cov_ii"] = np.matmul(center_miu_imag.T, center_miu_imag) / numvecs
    save["mean_real"], save["mean_imag"] = miu_real_mean[0], miu_imag_mean[0]

    # test_nsvae_se.py:482-502 on the valid frames of the two miu as the two sets
    set1 = np.concatenate([post["a"][0][k, :n] for k, n in enumerate(FRAMES)])
    set2 = np.concatenate([post["b"][0][k, :n] for k, n in enumerate(FRAMES)])
    mean1, mean2 = np.mean(set1, axis=0, keepdims=True), np.mean(set2, axis=0, keepdims=True)
    save["sil_sc"] = np.float32(simple_silhouette_score(set1, set2, mean1, mean2, "euclidean"))
    save["sil_var_avg_1"] = np.mean(np.var(set1, axis=0), axis=0)
    save["sil_var_avg_2"] = np.mean(np.var(set2, axis=0), axis=0)
    save["sil_mean_dis"] = np.float32(np.sum((mean1 - mean2) ** 2, axis=(1, 2))[0])
    for k, v in save.items():
        assert np.asarray(v).dtype in (np.float32, np.int64), (k, np.asarray(v).dtype)
    np.savez_compressed(a.out, **save)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
