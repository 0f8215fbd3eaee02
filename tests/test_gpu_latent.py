"""The latent-space report on the MI355X (i-dccrn-vae_amd/latent.py, csrc/latent.hip) against the float64 host definition of
tests/latent_ref.py: row statistics and posterior distances of a NaN-padded ragged batch, the covariance of miu on and around the
chunk edges of its accumulator, the silhouette score, and the in-place reading of real encoder outputs.  The references are computed
once per module."""
import importlib
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import latent_ref as R  # noqa: E402
from oracle import idccrn_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
FRAMES, T = [1, 2, 63, 64, 65, 130], 130
ZDIMS = (16, 128)
# both sides sum the same float32 values in double: N < 4000 terms reorder within N 2^-53 = 4.4e-13 of sum |x_i||x_j|
COV_REL = 1e-12


def _lat():
    return importlib.import_module("i-dccrn-vae_amd.latent")


def _dev(arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _views(q, order, pad, Tp):
    """The three latents (device tensors) as encoder-style views of ONE planar buffer that holds them in ``order`` behind ``pad``
    channels of NaN, with ``Tp`` columns per row: what an encoder returns, at another width, pitch and channel order."""
    ops = _lat().ops
    z = q[0].shape[2]
    parts = [torch.full_like(q[0][:, :, :pad], float("nan"))] + [q[i] for i in order]
    pl = ops.Planar.from_tensor5(torch.cat(parts, dim=2).permute(0, 2, 1, 3).unsqueeze(2), Tp)
    out = [None, None, None]
    for pos, i in enumerate(order):
        v = pl.channel_slice(pad + pos * z, pad + (pos + 1) * z)
        v._idv, v._idv_off = pl, pad + pos * z
        out[i] = v
    return tuple(out)


# ----------------------------------------------------------------------------- 1, 2: row statistics and pair distances
@pytest.fixture(scope="module")
def rows_ref():
    """Per zdim: two NaN-padded posteriors of the six rows, and the host definition of every row in float64 and float32."""
    table = {}
    for z in ZDIMS:
        a = tuple(R.nan_past(x, FRAMES) for x in R.make_inputs((len(FRAMES), T, z), 100 + z))
        b = tuple(R.nan_past(x, FRAMES) for x in R.make_inputs((len(FRAMES), T, z), 200 + z))
        ref = {}
        for name, dt in (("f64", np.float64), ("f32", np.float32)):
            cut = lambda q, k: tuple(x[k, :FRAMES[k]] for x in q)
            ref["stats_" + name] = [R.posterior_stats(*cut(a, k), dtype=dt) for k in range(len(FRAMES))]
            ref["dist_" + name] = [R.pair_distance(cut(a, k), cut(b, k), dtype=dt) for k in range(len(FRAMES))]
        table[z] = (a, b, ref)
    return table


def _floors_hold(tag, keys, got, f64, f32):
    """|device - float64| <= 4 x the largest |float32 host - float64 host| of the case, per key; prints both."""
    bad = []
    for key in keys:
        want = np.array([r[key] for r in f64])
        floor = float(np.max(np.abs(np.array([r[key] for r in f32]) - want)))
        worst = float(np.max(np.abs(got[key] - want)))
        print(f"{tag} {key}: float32 floor {floor:.3e} bound {4 * floor:.3e} device worst {worst:.3e}")
        assert np.isfinite(got[key]).all() and got[key].dtype == np.float64 and got[key].shape == want.shape
        if not worst <= 4 * floor:
            bad.append((key, floor, worst))
    assert not bad, bad


@pytest.mark.parametrize("z", ZDIMS)
def test_row_statistics_within_four_float32_floors(rows_ref, z):
    """One batch of rows of 1, 2, 63, 64, 65 and 130 frames (T = 130), NaN at and past every row's frames and in the imaginary channel
    of log_sigma, against tests/latent_ref.py in float64: per key |device - float64| <= 4 x the largest |float32 host - float64
    host| of the case (the rule of tests/test_gpu_prepare.py: the factor covers another summation order and the device's exp / log).

    Measured on the MI355X (DESIGN.md 3.11 has every key), float32 floor / device worst at zdim 16 and 128: kl 9.2e-6 / 8.3e-6 and
    5.0e-5 / 7.0e-5 (values near 50 and 400), vrr_min 1.1e-7 / 1.1e-7 and 6.2e-9 / 1.2e-8, vrr_mean 4.5e-8 / 8.1e-9 and 2.2e-8 /
    2.8e-9, vii 3.2e-7 / 4.5e-8 and 3.4e-7 / 1.2e-7: the double sums gain on the means and norms; minima, maxima and the KL carry the
    rounding of single fp32 elements, where the device's expf / logf and numpy's differ in the last bit."""
    L = _lat()
    a, b, ref = rows_ref[z]
    got = _host(L.posterior_stats(*_dev(a), frames=FRAMES))
    assert tuple(got) == R.STAT_KEYS
    _floors_hold(f"zdim {z}", R.STAT_KEYS, got, ref["stats_f64"], ref["stats_f32"])


@pytest.mark.parametrize("z", ZDIMS)
def test_pair_distances_within_four_float32_floors(rows_ref, z):
    """dis_mean / dis_sigma / dis_delta of the same batch between two posteriors, same rule.  The second posterior is a copy in a
    planar buffer of another width and pitch (delta, log_sigma, miu behind 16 unused channels), read in place, so the kernel reads
    two sources with different H, Jp, Tp and offsets; the copy route gives the same bits.

    Measured on the MI355X, float32 floor / device worst at zdim 16 and 128: dis_mean 5.7e-7 / 8.6e-8 and 6.3e-7 / 6.3e-8, dis_sigma
    3.1e-7 / 7.1e-8 and 3.6e-7 / 1.0e-7, dis_delta 4.2e-7 / 3.6e-8 and 1.0e-6 / 2.6e-8."""
    L = _lat()
    a, b, ref = rows_ref[z]
    da, db = _dev(a), _dev(b)
    vb = _views(db, (2, 1, 0), 16, T + 3)
    assert L._in_place(vb[0]) is vb[0]._idv and L._in_place(da[0]) is None
    dev = L.pair_distance(da, vb, frames=torch.tensor(FRAMES))
    copied = L.pair_distance(da, db, frames=FRAMES)
    assert all(_same_bits(dev[key], copied[key]) for key in R.DIST_KEYS)
    got = _host(dev)
    assert tuple(got) == R.DIST_KEYS
    _floors_hold(f"zdim {z}", R.DIST_KEYS, got, ref["dist_f64"], ref["dist_f32"])


@pytest.mark.parametrize("z", ZDIMS)
def test_rows_do_not_depend_on_the_batch(rows_ref, z):
    """Every row evaluated alone (B = 1, T = its own frames) gives the bits it has inside the NaN-padded batch, for every key."""
    L = _lat()
    a, b, _ = rows_ref[z]
    da, db = _dev(a), _dev(b)
    stats, dist = L.posterior_stats(*da, frames=FRAMES), L.pair_distance(da, db, frames=FRAMES)
    for k, n in enumerate(FRAMES):
        one_a = tuple(x[k:k + 1, :n].contiguous() for x in da)
        one_b = tuple(x[k:k + 1, :n].contiguous() for x in db)
        s1, d1 = L.posterior_stats(*one_a), L.pair_distance(one_a, one_b, frames=[n])
        for key in R.STAT_KEYS:
            assert _same_bits(s1[key], stats[key][k:k + 1].contiguous()), (k, key)
        for key in R.DIST_KEYS:
            assert _same_bits(d1[key], dist[key][k:k + 1].contiguous()), (k, key)


# ----------------------------------------------------------------------------- 3, 4: covariance of miu
@pytest.fixture(scope="module")
def cov_ref():
    """Per zdim: five rows of 1, 2, c - 1, c + 1 and T frames (c the accumulator's chunk length, the frames being numbered b T + t):
    rows end on both sides of a chunk edge, the first chunk holds a single valid frame, six chunks in all."""
    c = _lat().ops.miu_moments_chunk()
    Tc = c + 40
    frames = [1, 2, c - 1, c + 1, Tc]
    assert 5 * Tc >= 3 * c and sum(frames) < 4000
    table = {}
    for z in ZDIMS:
        miu = R.nan_past(R.make_inputs((5, Tc, z), 300 + z)[0], frames)
        valid = [miu[k, :n] for k, n in enumerate(frames)]
        table[z] = (miu, frames, R.miu_cov(valid), R.cov_scale(valid))
    return table


def _cov_close(got, want, scale, tag):
    for key in R.COV_KEYS + ("mean_real", "mean_imag"):
        err = np.abs(got[key] - want[key])
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape and np.isfinite(got[key]).all()
        ratio = float(np.max(err / scale[key]))
        print(f"{tag} {key}: worst |device - float64| / scale {ratio:.3e} (bound {COV_REL:.0e})")
        assert ratio <= COV_REL, (tag, key, ratio)
    assert abs(got["mean_dis"] - want["mean_dis"]) <= COV_REL * want["mean_dis"]


@pytest.mark.parametrize("z", ZDIMS)
def test_miu_covariance_on_the_chunk_edges(cov_ref, z):
    """Every entry of cov_rr / cov_ri / cov_ii within 1e-12 x (sum_n |x_i||x_j|) / n of the float64 host definition, the means within
    1e-12 x mean|x|.  cov_ri is far from symmetric (asserted on the reference), so a transposed tile write can not pass.

    Measured on the MI355X: entries within 1.2e-15 of their scale, means within 1.3e-16, at both zdim and for every cutting."""
    L = _lat()
    miu, frames, want, scale = cov_ref[z]
    asym = np.abs(want["cov_ri"] - want["cov_ri"].T).max()
    assert asym >= 1000 * COV_REL * scale["cov_ri"].max()
    acc = L.MiuMoments(z, "cuda").update(_dev((miu,))[0], frames)
    assert acc.count == sum(frames)
    got = acc.result()
    assert got["n"] == sum(frames)
    _cov_close(got, want, scale, f"zdim {z}")


@pytest.mark.parametrize("z", ZDIMS)
def test_miu_covariance_does_not_depend_on_the_cutting(cov_ref, z):
    """One batch, five batches of one, and two accumulators merged agree within the bound; the same calls twice give the same bits;
    summary() is the host definition's summary of the reference matrices within the bound scaled by the sums it takes."""
    L = _lat()
    miu, frames, want, scale = cov_ref[z]
    x = _dev((miu,))[0]

    def whole():
        return L.MiuMoments(z, "cuda").update(x, frames)

    def singles():
        acc = L.MiuMoments(z, "cuda")
        for k, n in enumerate(frames):
            acc.update(x[k:k + 1, :n].contiguous())
        return acc

    def merged():
        first, second = L.MiuMoments(z, "cuda").update(x[:3], frames[:3]), L.MiuMoments(z, "cuda").update(x[3:], frames[3:])
        return first.merge(second)

    accs = {"whole": whole(), "singles": singles(), "merged": merged()}
    res = {k: a.result() for k, a in accs.items()}
    for k, r in res.items():
        assert accs[k].count == sum(frames)
        _cov_close(r, want, scale, f"zdim {z} {k}")
    for k in ("singles", "merged"):
        for key in R.COV_KEYS + ("mean_real", "mean_imag"):
            assert np.max(np.abs(res[k][key] - res["whole"][key]) / scale[key]) <= COV_REL, (k, key)
    for make, k in ((whole, "whole"), (singles, "singles"), (merged, "merged")):
        assert _same_bits(make()._state, accs[k]._state), k
    bound = {k: COV_REL * scale["cov_" + k] for k in ("rr", "ri", "ii")}
    got, ref = accs["whole"].summary(), R.cov_summary(want["cov_rr"], want["cov_ri"], want["cov_ii"])
    for k, bm in bound.items():
        diag = np.diagonal(bm)
        tol = {"diag_abs": diag.sum() / z, "diag_mean": diag.sum() / z, "diag_min": diag.max(), "diag_max": diag.max(),
               "offdiag_abs": (bm.sum() - diag.sum()) / (z * (z - 1))}
        for name, t in tol.items():
            assert abs(got[f"{name}_{k}"] - ref[f"{name}_{k}"]) <= t, (name, k)
    assert abs(got["mean_dis"] - want["mean_dis"]) <= COV_REL * want["mean_dis"]


# ----------------------------------------------------------------------------- 5: silhouette
@pytest.fixture(scope="module")
def sil_ref():
    table = {}
    for z in ZDIMS:
        for n1 in (1, 40, 257):
            rng = np.random.default_rng(1000 * z + n1)
            s1 = (rng.standard_normal((n1, z, 2)) + 0.5).astype(np.float32)
            s2 = (0.7 * rng.standard_normal((50, z, 2)) - 0.3).astype(np.float32)
            table[(z, n1)] = (s1, s2, R.silhouette(s1, s2), R.silhouette(s1, s2, np.float32))
    return table


@pytest.mark.parametrize("n1", (1, 40, 257))
@pytest.mark.parametrize("z", ZDIMS)
def test_silhouette_within_four_float32_floors(sil_ref, z, n1):
    """sc, mean_dis and var_avg of sets of N1 = 1, 40, 257 and N2 = 50 vectors: |device - float64| <= 4 x |float32 host - float64 host|.

    Measured on the MI355X: sc within 1.2e-16 (floors 2e-9 ... 4e-8), mean_dis within 4.6e-13 (floors 2e-7 ... 7e-6), var_avg within
    2.3e-16 (floors 5e-9 ... 3e-7; exactly 0 on both sides for the set of one vector)."""
    L = _lat()
    s1, s2, f64, f32 = sil_ref[(z, n1)]
    got = L.silhouette(*_dev((s1, s2)))
    assert set(got) == {"sc", "mean_dis", "var_avg_1", "var_avg_2"}
    flat = lambda d: np.array([d["sc"], d["mean_dis"], *d["var_avg_1"], *d["var_avg_2"]], dtype=np.float64)
    assert all(isinstance(v, float) for v in flat(got).tolist()) and np.isfinite(flat(got)).all()
    floor, err = np.abs(flat(f32) - flat(f64)), np.abs(flat(got) - flat(f64))
    print(f"zdim {z} N1 {n1}: float32 floor {floor} device {err}")
    assert (err <= 4 * floor).all()


# ----------------------------------------------------------------------------- 6: real encoders, read in place
def _load(module, seed):
    module.load_state_dict(O.synth_state_dict({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed))
    return module.cuda()


def test_encoder_outputs_are_read_in_place():
    """The views the full-width causal encoders return for lengths = [1600, 900, 1234] (17, 10 and 13 frames), fed as they are (the
    planar LSTM output is read in place: the speech latent at channel offset 0, the noise latent at 384) and as .contiguous() copies
    (packed into a fresh planar buffer): identical bits from posterior_stats, pair_distance and MiuMoments."""
    L = _lat()
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    zdim, lens = 128, [1600, 900, 1234]
    np_ = O.net_params(True, 32)
    noisy_enc = _load(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, 1, 2), 51)
    clean_enc = _load(pm.pvae_dccrn_encoder_skip_prepare(np_, True, "cuda", zdim, NFFT, HOP, WIN, 1), 52)
    g = torch.Generator().manual_seed(5)
    x = torch.full((3, max(lens)), float("nan"))
    for b, n in enumerate(lens):
        x[b, :n] = 0.1 * torch.randn(n, generator=g)
    with torch.no_grad():
        out_n = noisy_enc(x.cuda(), train=False, lengths=lens)
        out_c = clean_enc(x.cuda(), train=False, lengths=lens)
    speech, noise, clean = out_n[1:4], out_n[5:8], out_c[1:4]
    fr = L.frames_of(out_n[-1])
    assert fr == [17, 10, 13] == L.frames_of(out_c[-1]) == L.frames(lens, HOP)
    assert [t._idv_off for t in speech] == [0, 128, 256] and [t._idv_off for t in noise] == [384, 512, 640]
    assert all(tuple(t.shape) == (3, 17, zdim, 2) and not t.is_contiguous() for t in speech + noise + clean)
    copy = lambda q: tuple(t.contiguous() for t in q)
    for name, q in (("speech", speech), ("noise", noise)):
        here, there = L.posterior_stats(*q, frames=fr), L.posterior_stats(*copy(q), frames=fr)
        for key in R.STAT_KEYS:
            assert _same_bits(here[key], there[key]), (name, key)
            assert torch.isfinite(here[key]).all(), (name, key)
    here, there = L.pair_distance(clean, speech, frames=fr), L.pair_distance(copy(clean), copy(speech), frames=fr)
    mixed = L.pair_distance(clean, copy(speech), frames=fr)
    for key in R.DIST_KEYS:
        assert _same_bits(here[key], there[key]) and _same_bits(here[key], mixed[key]), key
        assert torch.isfinite(here[key]).all() and (here[key] > 0).all(), key
    for miu in (speech[0], noise[0]):
        a, b = L.MiuMoments(zdim, "cuda").update(miu, fr), L.MiuMoments(zdim, "cuda").update(miu.contiguous(), fr)
        assert a.count == b.count == sum(fr) and _same_bits(a._state, b._state)
        assert np.isfinite(a.result()["cov_ri"]).all()
    # the values are those of the host definition on the encoder's own numbers (row 1: 10 frames)
    row = tuple(t[1, :10].cpu().numpy() for t in noise)
    want, floor = R.posterior_stats(*row), R.posterior_stats(*row, dtype=np.float32)
    got = L.posterior_stats(*noise, frames=fr)
    for key in R.STAT_KEYS:
        # one row's float32 floor can be zero (a minimum that both precisions compute exactly): a few fp32 ulps are added
        assert abs(float(got[key][1]) - want[key]) <= 4 * abs(floor[key] - want[key]) + 1e-6 * abs(want[key]), key
    sets = [L.sample_rows(t, fr, 8, random.Random(3)) for t in (speech[0], noise[0])]
    assert all(s.shape == (8 * 3, zdim, 2) for s in sets)
    assert np.isfinite(L.silhouette(*sets)["sc"])
