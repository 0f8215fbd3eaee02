"""Mixture synthesis on the MI355X (csrc/mix.hip through dataset.mix.snr_mix / mix_draw / DynamicMixtures) against the float64 host
definition of tests/mix_ref.py.  Rows of at most 16385 samples; the references are computed once per module.  The conditions under
which decisions are compared as integers (margins to the clip threshold and to thresh_db, no cancelling row) are asserted from the
reference alone in tests/test_mix_host.py."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mix_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NMAX = max(R.LENGTHS)
GAIN_TOL = 4 * NMAX * 2.0 ** -53          # any order of four sums of at most NMAX non-negative terms in double: 7.3e-12
SIGNALS = ("noisy", "clean_out", "noise_out")


def _mix():
    return importlib.import_module("i-dccrn-vae_amd.dataset.mix")


def _padded(rows, fill=float("nan"), extra=0):
    """The rows in one batch, ``fill`` at and past every row's end; ``extra``: that many more columns in the allocation (the row
    pitch), sliced away again."""
    width = max(len(r) for r in rows)
    x = torch.full((len(rows), width + extra), fill)
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(np.asarray(r, dtype=np.float32))
    return x.cuda()[:, :width]


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _run(cases, snr, lev, seg, extra=0, stats=False):
    """One snr_mix call on all rows of ``cases`` in NaN-padded batches -> (noisy, clean_out, noise_out, info) on the host."""
    M = _mix()
    out = M.snr_mix(_padded([c for c, _, _ in cases], extra=extra), _padded([v for _, v, _ in cases], extra=extra), snr, lev,
                    lengths=[len(c) for c, _, _ in cases], noise_lengths=[len(v) for _, v, _ in cases],
                    noise_offsets=[o for _, _, o in cases], segmental=seg, stats=stats)
    return out


def _check_against(cases, want, got, tag):
    """3. and 4. of the issue for one call: gains within GAIN_TOL, each output within 1 float32 ulp of the float64 reference cast to
    float32, exact zeros behind a row, finite, and noisy against clean_out + noise_out within 1.5 ulp."""
    noisy, clean_out, noise_out, info = got
    sig = dict(zip(SIGNALS, (noisy.cpu().numpy(), clean_out.cpu().numpy(), noise_out.cpu().numpy())))
    g = {k: info[k].cpu().numpy() for k in ("g_clean", "g_noise", "level_db")}
    worst_g = worst_u = worst_s = 0.0
    for b, ((c, _, _), r) in enumerate(zip(cases, want)):
        n = len(c)
        for k in ("g_clean", "g_noise"):
            assert np.isfinite(g[k][b]) and abs(g[k][b] - r[k]) <= GAIN_TOL * abs(r[k]), (tag, n, k, g[k][b], r[k])
            worst_g = max(worst_g, abs(g[k][b] - r[k]) / abs(r[k]) if r[k] else 0.0)
        assert abs(g["level_db"][b] - r["level_db"]) <= 1e-9, (tag, n, g["level_db"][b], r["level_db"])
        for k in SIGNALS:
            y = sig[k][b]
            assert y.dtype == np.float32 and np.isfinite(y).all() and not y[n:].any(), (tag, n, k)
            err = np.abs(y[:n].astype(np.float64) - r[k].astype(np.float64))
            ulp = np.maximum(R.ulp32(y[:n]), R.ulp32(r[k]))
            assert (err <= ulp).all(), (tag, n, k, float((err / ulp).max()))
            worst_u = max(worst_u, float((err / ulp).max()))
        big = np.maximum(np.abs(sig["noisy"][b, :n]), np.maximum(np.abs(sig["clean_out"][b, :n]), np.abs(sig["noise_out"][b, :n])))
        diff = np.abs(sig["noisy"][b, :n].astype(np.float64) - (sig["clean_out"][b, :n].astype(np.float64) + sig["noise_out"][b, :n]))
        assert (diff <= 1.5 * R.ulp32(big)).all(), (tag, n)
        worst_s = max(worst_s, float((diff / R.ulp32(big)).max()))
    return worst_g, worst_u, worst_s


@pytest.fixture(scope="module")
def ref():
    """The PCM16 cases of mix_ref.cases() and the reference's result for every (snr, level, mode)."""
    cases = R.cases()
    return cases, {key: [R.mix(c, v, o, *key) for c, v, o in cases] for key in R.grid()}


@pytest.fixture(scope="module")
def float_ref():
    cases = R.float_cases()
    return cases, {seg: [R.mix(c, v, o, 5.0, -25.0, seg) for c, v, o in cases] for seg in (False, True)}


def test_statistics_are_bit_exact(ref):
    """Samples k / 32768: every sum of squares is an integer below 2^53 times 2^-30, so no order of summation changes it.  max|c|,
    sum c^2, max|v|, sum v^2 of every row and of every window equal the reference bit for bit; all lengths in one NaN-padded batch
    with the cyclic offsets of the cases."""
    cases, table = ref
    *_, info = _run(cases, 0.0, -25.0, False, stats=True)
    W = info["windows"].cpu().numpy()
    nwin = -(-NMAX // R.WIN)
    assert info["windows"].dtype == torch.float64 and W.shape == (len(cases), nwin, 6)
    for b, ((c, _, _), r) in enumerate(zip(cases, table[(0.0, -25.0, False)])):
        for k in ("max_c", "sum_c2", "max_v", "sum_v2"):
            got = info[k][b].cpu().numpy()
            assert got.dtype == np.float64 and got.view(np.int64) == np.float64(r[k]).view(np.int64), (len(c), k, float(got), r[k])
        wc, wv = R.window_sums(c), R.window_sums(r["v"])
        nw = len(wc)
        assert np.array_equal(W[b, :nw, 0:2].view(np.int64), wc.view(np.int64)), len(c)
        assert np.array_equal(W[b, :nw, 2:4].view(np.int64), wv.view(np.int64)), len(c)
        assert not W[b, nw:].any() and np.isfinite(W[b]).all()


def test_decisions_gains_and_outputs(ref):
    """Every (SNR, level, mode): clipped and the active-sample count equal the reference as integers (valid under the host-asserted
    margins); the gains within 4 n_max 2^-53 = 7.3e-12 relative; the outputs as _check_against states.

    Measured on the MI355X: worst relative gain error 6.5e-16, every output sample equal to the reference's float32, noisy against
    clean_out + noise_out at most 1.0 ulp; 150 of the 768 cases clip, 64 are partly active."""
    cases, table = ref
    worst = (0.0, 0.0, 0.0)
    n_clip = n_part = 0
    for key, want in table.items():
        got = _run(cases, *key)
        info = got[3]
        assert info["clipped"].dtype == info["active"].dtype == torch.int32
        assert info["clipped"].tolist() == [r["clipped"] for r in want], key
        assert info["active"].tolist() == [r["active"] for r in want], key
        n_clip += sum(info["clipped"].tolist())
        n_part += sum(1 for a, (c, _, _) in zip(info["active"].tolist(), cases) if key[2] and 0 < a < len(c))
        worst = tuple(max(a, b) for a, b in zip(worst, _check_against(cases, want, got, key)))
    print(f"mix, PCM16 rows: worst relative gain error {worst[0]:.3e} (bound {GAIN_TOL:.3e}), worst output error {worst[1]:.2f} ulp, "
          f"worst noisy - (clean + noise) {worst[2]:.2f} ulp; {n_clip} cases clip, {n_part} partly active")
    assert (n_clip, n_part) == (150, 64)


def test_rows_are_independent(ref, float_ref):
    """Bit equality of all outputs and info for a row alone (B = 1, 16-byte aligned) against the same row inside the NaN-padded batch
    at row pitches NMAX (odd), + 2, + 3 and + 77, and read in place from SignalPools whose members start 0, 1, 2 and 3 floats past a
    16-byte boundary.  The float32 rows make this a statement about the order of the sums, which the exact PCM16 sums cannot see."""
    M = _mix()
    for cases, key in ((ref[0], (0.0, -15.0, True)), (float_ref[0], (5.0, -25.0, False)), (float_ref[0], (5.0, -25.0, True))):
        snr, lev, seg = key
        alone = []
        for c, v, o in cases:
            y = M.snr_mix(torch.from_numpy(c)[None].cuda(), torch.from_numpy(v)[None].cuda(), snr, lev, noise_offsets=[o], segmental=seg,
                          stats=True)
            alone.append(y)
        keys = sorted(alone[0][3])

        def same(got, tag):
            for b, (c, _, _) in enumerate(cases):
                n, one = len(c), alone[b]
                for s in range(3):
                    assert torch.equal(_bits(got[s][b, :n]), _bits(one[s][0])), (tag, n, SIGNALS[s])
                    assert not got[s][b, n:].any()
                for k in keys:
                    if k == "windows":
                        nw = one[3][k].shape[1]
                        assert torch.equal(_bits(got[3][k][b, :nw]), _bits(one[3][k][0])), (tag, n, k)
                    else:
                        assert torch.equal(_bits(got[3][k][b]), _bits(one[3][k][0])), (tag, n, k)

        for extra in (0, 2, 3, 77):
            same(_run(cases, snr, lev, seg, extra=extra, stats=True), ("pitch", extra))
        cp = M.SignalPool([c for c, _, _ in cases], "cuda")
        npool = M.SignalPool([v for _, v, _ in cases], "cuda")
        assert {o % 4 for o in cp.offsets} == {0, 1, 2, 3} == {o % 4 for o in npool.offsets} and cp.data.data_ptr() % 16 == 0
        B = len(cases)
        draw = M.Draw(list(range(B)), [0] * B, [len(c) for c, _, _ in cases], list(range(B)), [o for _, _, o in cases], [snr] * B, [lev] * B)
        same(M.mix_draw(cp, npool, draw, NMAX, segmental=seg, stats=True), "pool")


def test_float_rows(float_ref):
    """0.1 N(0, 1) float32 clean and noise at the same lengths: the four statistics within n 2^-53 relative of the reference (the
    squares are exact in double on both sides; a sum of n non-negative terms errs by at most (n - 1) u in any order, so two orders
    differ by at most 2 (n - 1) u; the reference's pairwise sum itself stays far inside, so n u is demanded), and gains and outputs
    as for the PCM16 rows.

    Measured on the MI355X: worst relative error of a sum 3.3e-16, of a gain 1.1e-15, every output sample equal."""
    cases, table = float_ref
    for seg, want in table.items():
        got = _run(cases, 5.0, -25.0, seg, stats=True)
        info = got[3]
        worst = 0.0
        for b, ((c, _, _), r) in enumerate(zip(cases, want)):
            for k in ("sum_c2", "sum_v2"):
                e = abs(float(info[k][b]) - r[k]) / r[k]
                worst = max(worst, e)
                assert e <= len(c) * 2.0 ** -53, (len(c), k, e)
            assert float(info["max_c"][b]) == r["max_c"] and float(info["max_v"][b]) == r["max_v"]
        assert info["clipped"].tolist() == [r["clipped"] for r in want] and info["active"].tolist() == [r["active"] for r in want]
        w = _check_against(cases, want, got, ("float", seg))
        print(f"mix, float32 rows, segmental={seg}: worst relative error of a sum {worst:.3e}, of a gain {w[0]:.3e}, outputs {w[1]:.2f} ulp")


def test_degenerate_rows():
    """All-zero clean, all-zero noise, both, n = 1 and m = 1: finite and equal to the reference under the same bounds, in both modes."""
    one, z = R.clean_row(3000, 1), np.zeros(3000, dtype=np.float32)
    other = R.noise_row(3000, 2)
    cases = [(z, other, 5), (one, z, 0), (z, z, 0), (one[:1], other, 7), (one, other[:1], 0), (one[:1], one[:1], 0), (one[:2], z[:1], 0)]
    for seg in (False, True):
        want = [R.mix(c, v, o, 5.0, -20.0, seg) for c, v, o in cases]
        assert all(R.clip_margin(r) >= 1e-6 and R.window_margin_db(r) >= 1e-6 and r["cancel"] <= 1000 for r in want)
        got = _run(cases, 5.0, -20.0, seg)
        assert got[3]["clipped"].tolist() == [r["clipped"] for r in want] and got[3]["active"].tolist() == [r["active"] for r in want]
        assert all(torch.isfinite(got[3][k]).all() for k in ("g_clean", "g_noise", "level_db"))
        _check_against(cases, want, got, ("degenerate", seg))
        assert not got[0][0].any() and not got[0][2].any() and torch.equal(got[0][1], got[1][1])


def test_realised_snr(ref):
    """Plain mode, rows where neither signal is zero: 10 log10(sum clean_out^2 / sum noise_out^2) in float64 from the device outputs
    equals snr_db within 1e-5 dB, ten times the 1e-6 dB one float32 rounding per sample can move it.  Measured on the MI355X: 5.4e-7 dB."""
    cases, _ = ref
    worst = 0.0
    for snr in R.SNRS:
        _, clean_out, noise_out, _ = _run(cases, snr, -25.0, False)
        ec, ev = (clean_out.double() ** 2).sum(1).cpu().numpy(), (noise_out.double() ** 2).sum(1).cpu().numpy()
        for b, (c, v, o) in enumerate(cases):
            if c.any() and R.cyclic(v, len(c), o).any():
                e = abs(10 * np.log10(ec[b] / ev[b]) - snr)
                worst = max(worst, e)
                assert e <= 1e-5, (len(c), snr, e)
    print(f"mix: realised SNR within {worst:.3e} dB")


def test_dynamic_mixtures():
    """batch(k) equals snr_mix on the rows and parameters draw_batch(k) names, bit for bit; one seed gives one stream, two seeds
    differ; order and shapes are SyntheticMixtures'; a clean recording shorter than ``samples`` comes back zero-padded."""
    M = _mix()
    dl = importlib.import_module("i-dccrn-vae_amd.dataset.dataload")
    rng = np.random.default_rng(11)
    clean = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (5000, 1601, 700, 9001, 3200)]
    noise = [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in (1, 333, 4800, 12001)]
    cp, npool = M.SignalPool(clean, "cuda"), M.SignalPool(noise, "cuda")
    assert cp.lengths == [5000, 1601, 700, 9001, 3200] and cp.offsets == [0, 5000, 6601, 7301, 16302] and cp.data.shape == (19502,)
    assert torch.equal(cp.member(2).cpu(), torch.from_numpy(clean[2]))
    batch, samples = 6, 3200
    for seg in (False, True):
        dm = M.DynamicMixtures(cp, npool, batch, samples=samples, seed=7, length=3, segmental=seg)
        short = 0
        for k in (0, 1, 2):
            d = M.draw_batch(k, 7, cp.lengths, npool.lengths, batch, samples)
            assert d == dm.draw(k)
            rows_c = [clean[c][s:s + n] for c, s, n in zip(d.clean_id, d.clean_start, d.lens)]
            got = dm.batch(k, info=True)
            want = M.snr_mix(_padded(rows_c), _padded([noise[j] for j in d.noise_id]), d.snr_db, d.level_db, lengths=d.lens,
                             noise_lengths=[len(noise[j]) for j in d.noise_id], noise_offsets=d.noise_offset, segmental=seg)
            for s in range(3):
                assert got[s].shape == (batch, samples) and got[s].dtype == torch.float32 and got[s].is_cuda
                assert torch.equal(_bits(got[s][:, :want[s].shape[1]]), _bits(want[s])) and not got[s][:, want[s].shape[1]:].any()
            for key in want[3]:
                assert torch.equal(_bits(got[3][key]), _bits(want[3][key])), key
            for b, n in enumerate(d.lens):
                short += n < samples
                assert not got[0][b, n:].any() and got[1][b, :n].any()
        assert short >= 1
        a, b = list(dm), list(M.DynamicMixtures(cp, npool, batch, samples=samples, seed=7, length=3, segmental=seg))
        assert len(a) == len(b) == 3 and all(len(t) == 3 for t in a)
        assert all(torch.equal(_bits(x), _bits(y)) for ta, tb in zip(a, b) for x, y in zip(ta, tb))
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[1], dm.batch(1)))
        c = list(M.DynamicMixtures(cp, npool, batch, samples=samples, seed=8, length=3, segmental=seg))
        assert not torch.equal(a[0][0], c[0][0])
    ref_stream = next(iter(dl.SyntheticMixtures(batch=batch, samples=samples, seed=5, length=1)))
    assert len(ref_stream) == len(a[0]) == 3 and all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(ref_stream, a[0]))
    # (noisy, clean, noise): the first is the sum of the other two within the three roundings
    noisy, cl, nz = a[0]
    assert (noisy.double() - (cl.double() + nz.double())).abs().max() <= 1.5 * float(np.spacing(np.float32(noisy.abs().max().item())))
