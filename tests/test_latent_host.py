"""CPU: the host side of the latent-space report (i-dccrn-vae_amd/latent.py).

(a) tests/latent_ref.py in float64 against tests/golden/latent_report.npz, what the reference's own functions returned for the
    fixture in float32 (tests/golden/make_latent_golden.py): at most 1e-5 relative per value;
(b) the checks on frames, zdim and shapes raise before any device use (there is no device here);
(c) the index logic of sample_rows with a seeded random.Random, and the frames_of / frames arithmetic."""
import importlib
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import latent_ref as R  # noqa: E402

REL = 1e-5            # the fixture is float32 arithmetic


@pytest.fixture(scope="module")
def lat():
    return importlib.import_module("i-dccrn-vae_amd.latent")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "latent_report.npz")))


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(want != 0)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _utt(fx, tag, k):
    n = int(fx["frames"][k])
    return tuple(fx[f"{name}_{tag}"][k, :n] for name in ("miu", "log_sigma", "delta"))


def test_fixture_is_what_the_issue_describes(fx):
    assert fx["frames"].tolist() == [7, 4, 1] and fx["miu_a"].shape == (3, 7, 16, 2)
    assert sum(os.path.getsize(os.path.join(HERE, "golden", f)) for f in ("latent_report.npz",)) < 200 * 1024
    for tag in "ab":
        for k, n in enumerate(fx["frames"]):
            miu, ls, dl = (fx[f"{name}_{tag}"][k] for name in ("miu", "log_sigma", "delta"))
            assert np.isnan(miu[n:]).all() and np.isnan(dl[n:]).all() and np.isnan(ls[..., 1]).all()
            assert np.isfinite(miu[:n]).all() and np.isfinite(dl[:n]).all() and np.isfinite(ls[:n, :, 0]).all()


def test_inputs_take_both_guard_branches_with_a_margin(fx):
    """At least 25 % of the elements on either side of the guard's threshold and none within 1e-3 of it: a last-bit difference
    in exp cannot flip a branch.  For the fixture and for the shapes of the GPU tests."""
    cases = [(fx["log_sigma_a"][k, :n], fx["delta_a"][k, :n]) for k, n in enumerate(fx["frames"]) if n > 1]
    for z in (16, 128):
        _, ls, dl = R.make_inputs((6, 130, z), 100 + z)
        cases.append((ls, dl))
    for ls, dl in cases:
        share, margin = R.guard_facts(ls, dl)
        assert 0.25 <= share <= 0.75 and margin >= 1e-3, (share, margin)


def test_row_statistics_and_distances_match_the_reference_functions(fx):
    worst = 0.0
    for k in range(3):
        a, b = _utt(fx, "a", k), _utt(fx, "b", k)
        s = R.posterior_stats(*a)
        worst = max(worst, _rel([s[key] for key in R.STAT_KEYS], fx["stats"][k]))
        d = R.pair_distance(a, b)
        worst = max(worst, _rel([d[key] for key in R.DIST_KEYS], fx["dists"][k]))
    print("worst relative difference", worst)
    assert worst <= REL


def test_miu_covariance_matches_the_reference_expressions(fx, lat):
    c = R.miu_cov([_utt(fx, "a", k)[0] for k in range(3)])
    assert c["n"] == 12
    worst = max(_rel(c[key], fx[key]) for key in R.COV_KEYS + ("mean_real", "mean_imag"))
    worst = max(worst, _rel(c["mean_dis"], fx["mean_dis"]))
    print("worst relative difference", worst)
    assert worst <= REL
    assert np.abs(c["cov_ri"] - c["cov_ri"].T).max() > 0.1                 # real x imaginary is no symmetric block
    # the package's summary of three matrices is the host definition's
    assert lat.cov_summary(c["cov_rr"], c["cov_ri"], c["cov_ii"]) == R.cov_summary(c["cov_rr"], c["cov_ri"], c["cov_ii"])


def test_silhouette_matches_the_reference_function(fx):
    s1 = np.concatenate([_utt(fx, "a", k)[0] for k in range(3)])
    s2 = np.concatenate([_utt(fx, "b", k)[0] for k in range(3)])
    s = R.silhouette(s1, s2)
    worst = max(_rel(s["sc"], fx["sil_sc"]), _rel(s["mean_dis"], fx["sil_mean_dis"]), _rel(s["var_avg_1"], fx["sil_var_avg_1"]),
                _rel(s["var_avg_2"], fx["sil_var_avg_2"]))
    print("worst relative difference", worst)
    assert worst <= REL


def test_float32_mode_is_the_reference_arithmetic(fx):
    """dtype=float32 stays float32 throughout: it lands on the fixture within a few ulp where float64 lands within 1e-5."""
    for k in range(3):
        s = R.posterior_stats(*_utt(fx, "a", k), dtype=np.float32)
        for j, key in enumerate(R.STAT_KEYS):
            assert abs(s[key] - fx["stats"][k, j]) <= 1e-6 * max(1.0, abs(fx["stats"][k, j])), (k, key)


# ----------------------------------------------------------------------------- argument checks, before any device use
def _lat(B=2, T=5, z=16, dtype=torch.float32):
    return torch.zeros(B, T, z, 2, dtype=dtype)


@pytest.mark.parametrize("frames,msg", [([5], "frame counts for a batch"), ([5, 0], "frames\\[1\\] = 0"), ([6, 1], "frames\\[0\\] = 6"),
                                        ([5, 2.0], "integers"), ([5, True], "integers"), ("55", "sequence"), (5, "sequence"),
                                        (torch.tensor([5.0, 1.0]), "1-D integer"), (torch.tensor([[5, 1]]), "1-D integer")])
def test_bad_frames_raise_on_the_host(lat, frames, msg):
    x = _lat()
    with pytest.raises(ValueError, match=msg):
        lat.posterior_stats(x, x, x, frames=frames)
    with pytest.raises(ValueError, match=msg):
        lat.pair_distance((x, x, x), (x, x, x), frames=frames)
    with pytest.raises(ValueError, match=msg):
        lat.MiuMoments(16, "cuda").update(x, frames)
    with pytest.raises(ValueError, match=msg):
        lat.sample_rows(x, frames, 3, random.Random(0))


def test_good_frames_pass_the_host_checks(lat):
    assert lat.check_frames(None, 2, 5) is None
    assert lat.check_frames([1, 5], 2, 5) == [1, 5] == lat.check_frames(torch.tensor([1, 5]), 2, 5)
    assert lat.check_frames(torch.tensor([1, 5], dtype=torch.int32), 2, 5) == [1, 5]


@pytest.mark.parametrize("z", [0, 8, 24, 144, 256])
def test_bad_zdim_raises_on_the_host(lat, z):
    x = torch.zeros(2, 5, z, 2)
    with pytest.raises(ValueError, match="zdim"):
        lat.posterior_stats(x, x, x)
    with pytest.raises(ValueError, match="zdim"):
        lat.silhouette(torch.zeros(4, z, 2), torch.zeros(4, z, 2))
    with pytest.raises(ValueError, match="zdim"):
        lat.MiuMoments(z, "cuda")
    for bad in (16.0, True, "16"):
        with pytest.raises(ValueError, match="zdim"):
            lat.MiuMoments(bad, "cuda")


def test_bad_shapes_and_types_raise_on_the_host(lat):
    x = _lat()
    for bad in (torch.zeros(2, 5, 16), torch.zeros(2, 5, 16, 3), _lat(dtype=torch.float64), np.zeros((2, 5, 16, 2), np.float32), None):
        with pytest.raises(ValueError):
            lat.posterior_stats(x, bad, x)
        with pytest.raises(ValueError):
            lat.pair_distance((x, x, x), (x, x, bad))
        with pytest.raises(ValueError):
            lat.MiuMoments(16, "cuda").update(bad)
    with pytest.raises(ValueError, match="does not match"):
        lat.posterior_stats(x, _lat(T=6), x)
    with pytest.raises(ValueError, match="does not match"):
        lat.pair_distance((x, x, x), (_lat(B=3),) * 3)
    with pytest.raises(ValueError, match="triple"):
        lat.pair_distance((x, x), (x, x, x))
    with pytest.raises(ValueError, match="zdim 16"):
        lat.MiuMoments(32, "cuda").update(x)
    with pytest.raises(ValueError):
        lat.silhouette(torch.zeros(4, 16, 2), torch.zeros(4, 32, 2))
    with pytest.raises(ValueError):
        lat.silhouette(torch.zeros(0, 16, 2), torch.zeros(4, 16, 2))
    with pytest.raises(ValueError):
        lat.silhouette(torch.zeros(4, 16), torch.zeros(4, 16, 2))
    acc = lat.MiuMoments(16, "cuda")
    with pytest.raises(ValueError):
        acc.merge(acc)
    with pytest.raises(ValueError):
        acc.merge(lat.MiuMoments(32, "cuda"))
    with pytest.raises(ValueError, match="no frames"):
        acc.result()
    assert acc.count == 0 and acc.merge(lat.MiuMoments(16, "cuda")) is acc          # an empty one: nothing to do, no device


def test_cpu_tensors_are_refused_after_the_host_checks(lat):
    """Valid arguments on the CPU reach the device check, which refuses them: there is no CPU fallback."""
    IdvError = importlib.import_module("i-dccrn-vae_amd._lib").IdvError
    x = _lat()
    with pytest.raises(IdvError):
        lat.posterior_stats(x, x, x, frames=[5, 1])
    with pytest.raises(IdvError):
        lat.pair_distance((x, x, x), (x, x, x))
    with pytest.raises(IdvError):
        lat.MiuMoments(16, "cuda").update(x)
    with pytest.raises(IdvError):
        lat.MiuMoments(16, "cpu").update(x)
    with pytest.raises(IdvError):
        lat.silhouette(torch.zeros(4, 16, 2), torch.zeros(3, 16, 2))


def test_new_entries_refuse_bad_arguments_before_any_launch(lat):
    """The C entries return IDV_EINVAL (-1) for refused arguments without touching a device; the size queries are host code."""
    lib = importlib.import_module("i-dccrn-vae_amd._lib").lib()
    c = lib.idv_miu_moments_chunk()
    assert c == lat.ops.miu_moments_chunk() and c >= 64 and c % 64 == 0
    wb = lib.idv_miu_moments_work_bytes
    assert wb(16, 1, 1) == 8 * (1 + 32 + 32 * 32) and wb(128, 5, c) == 5 * 8 * (1 + 256 + 256 * 256)
    assert wb(128, 1, c + 1) == 2 * wb(128, 1, c)
    for bad in ((8, 1, 1), (24, 1, 1), (144, 1, 1), (16, 0, 1), (16, 1, 0), (16, 65536, 1), (16, 65535, 65535)):
        assert wb(*bad) == -1, bad
    assert lib.idv_latent_row_stats(None, 48, 8, 3, 0, 16, 32, 16, None, 1, 2, None, None, None) == -1
    assert lib.idv_latent_set_moments(None, 1, 32, None, None) == -1
    assert lib.idv_miu_moments_merge(None, None, 16, None) == -1


# ----------------------------------------------------------------------------- sampling and frame arithmetic
def test_sample_indices_with_a_seeded_rng(lat):
    fr = [1, 2, 39, 40, 41, 500]
    rows, cols = lat.sample_indices(fr, 40, random.Random(7))
    assert len(rows) == len(cols) == sum(min(40, f) for f in fr)
    for b, f in enumerate(fr):
        mine = [c for r, c in zip(rows, cols) if r == b]
        assert len(mine) == min(40, f) == len(set(mine)) and all(0 <= c < f for c in mine)
    assert rows == sorted(rows)
    assert (rows, cols) == lat.sample_indices(fr, 40, random.Random(7))            # the caller's generator decides the draw
    assert cols != lat.sample_indices(fr, 40, random.Random(8))[1]
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            lat.sample_indices(fr, bad, random.Random(0))
    with pytest.raises(ValueError):
        lat.sample_indices(fr, 3, np.random.default_rng(0))


def test_sample_rows_gathers_valid_frames_only(lat):
    B, T, z = 4, 9, 16
    fr = [1, 4, 9, 2]
    v = torch.arange(B * T, dtype=torch.float32).reshape(B, T, 1, 1).expand(B, T, z, 2).clone()
    for b, f in enumerate(fr):
        v[b, f:] = float("nan")
    got = lat.sample_rows(v, fr, 3, random.Random(1))
    assert got.shape == (1 + 3 + 3 + 2, z, 2) and got.is_contiguous() and torch.isfinite(got).all()
    rows, cols = lat.sample_indices(fr, 3, random.Random(1))
    assert got[:, 0, 0].tolist() == [float(r * T + c) for r, c in zip(rows, cols)]
    assert lat.sample_rows(v[:, :1], None, 5, random.Random(0)).shape == (B, z, 2)


def test_frames_arithmetic(lat):
    assert lat.frames([1600, 900, 1234, 99, 100, 0], 100) == [17, 10, 13, 1, 2, 1]
    assert lat.frames(torch.tensor([1600, 900]), 100) == [17, 10]
    for bad in (0, -1, 100.0, True):
        with pytest.raises(ValueError):
            lat.frames([1600], bad)
    with pytest.raises(ValueError):
        lat.frames([1600, -1], 100)
    with pytest.raises(ValueError):
        lat.frames([1600.0], 100)

    class _X:                                      # what an encoder hangs on stft_x: a planar spectrum that may carry lengths
        lengths = None
    stft_x = torch.zeros(3, 257, 17, 2)
    assert lat.frames_of(stft_x) == [17, 17, 17]
    stft_x._idv = _X()
    assert lat.frames_of(stft_x) == [17, 17, 17]
    stft_x._idv.lengths = lat.ops.Lengths([1600, 900, 1234], None, dev=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="hop"):
        lat.frames_of(stft_x)
    assert lat.frames_of(stft_x, hop=100) == [17, 10, 13]
    stft_x._idv_hop = 100
    assert lat.frames_of(stft_x) == [17, 10, 13]
    with pytest.raises(ValueError):
        lat.frames_of(torch.zeros(3, 17, 2))
