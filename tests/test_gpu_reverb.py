"""Reverberation on the MI355X (csrc/reverb.hip through dataset.reverb.reverb / reverb_draw and DynamicMixtures with a RirPool)
against the float64 host definition of tests/reverb_ref.py.  Rows of at most 16385 samples and 16384 taps; the references are computed
once per module.  That the dyadic set is exact in any summation order is asserted from the reference alone in
tests/test_reverb_host.py."""
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

import reverb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _rv():
    return importlib.import_module("i-dccrn-vae_amd.dataset.reverb")


def _mix():
    return importlib.import_module("i-dccrn-vae_amd.dataset.mix")


def _padded(rows, extra=0):
    """The rows in one batch, NaN at and past every row's end; ``extra``: that many more columns in the allocation (the row pitch),
    sliced away again."""
    width = max(len(r) for r in rows)
    x = torch.full((len(rows), width + extra), NAN)
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(np.asarray(r, dtype=np.float32))
    return x.cuda()[:, :width]


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


def _batch(rows, extra=0, taps=None):
    """One reverb call on all (x, h) of ``rows`` in NaN-padded batches -> [B, width] on the host."""
    RV = _rv()
    y = RV.reverb(_padded([x for x, _ in rows], extra), _padded([h for _, h in rows], extra), lengths=[len(x) for x, _ in rows],
                  rir_lengths=[len(h) for _, h in rows], taps=taps)
    return y.cpu().numpy()


@pytest.fixture(scope="module")
def table():
    rows = R.cases()
    return rows, [R.reverb(x, h) for x, h in rows], _batch(rows)


@pytest.fixture(scope="module")
def dyadic():
    rows = R.dyadic_cases()
    return rows, [R.reverb(x, h)[0] for x, h in rows], _batch(rows)


def _within(y, ref, S, K, tag):
    """|y - ref| <= ulp32 + 2 K 2^-53 S elementwise -> the worst ratio."""
    assert y.dtype == np.float32 and np.isfinite(y).all(), tag
    err = np.abs(y.astype(np.float64) - ref)
    lim = R.bound(K, S, y, ref)
    assert (err <= lim).all(), (tag, float((err / lim).max()), int(np.argmax(err / lim)))
    return float((err / lim).max()) if len(y) else 0.0


def test_accuracy(table):
    rows, want, got = table
    worst = 0.0
    for b, ((x, h), (ref, S)) in enumerate(zip(rows, want)):
        n, K = len(x), len(h)
        assert not got[b, n:].any() and not np.signbit(got[b, n:]).any(), (n, K)             # exact zeros behind the row
        worst = max(worst, _within(got[b, :n], ref, S, K, (n, K)))
    print(f"reverb: worst error over the bound ulp32 + 2 K 2^-53 S: {worst:.3f}")


def test_dyadic_set_bit_for_bit(dyadic):
    rows, want, got = dyadic
    for b, ((x, h), ref) in enumerate(zip(rows, want)):
        n = len(x)
        exp = ref.astype(np.float32) + np.float32(0.0)                                       # a zero sum is +0
        assert np.array_equal(_bits(got[b, :n]), _bits(exp)), (n, len(h), int((got[b, :n] != exp).sum()))
        assert not got[b, n:].any()


def test_identities_bit_for_bit():
    RV = _rv()
    rows = [R.speech_row(n, 200 + k) for k, n in enumerate((1, 17, 4097, 9000))]
    x = _padded(rows)
    lens = [len(r) for r in rows]
    one = torch.ones(1, 1, device="cuda")
    y = RV.reverb(x, one, lengths=lens).cpu().numpy()
    half = RV.reverb(x, 0.5 * one, lengths=lens).cpu().numpy()
    for b, r in enumerate(rows):
        assert np.array_equal(_bits(y[b, :lens[b]]), _bits(r)) and not y[b, lens[b]:].any()
        assert np.array_equal(_bits(half[b, :lens[b]]), _bits(r / np.float32(2)))
    for d in (1, 15, 16, 17, 4096):
        h = torch.zeros(1, d + 1, device="cuda")
        h[0, d] = 1.0
        y = RV.reverb(x, h, lengths=lens).cpu().numpy()
        for b, r in enumerate(rows):
            want = np.concatenate([np.zeros(d, dtype=np.float32), r])[:lens[b]]
            assert np.array_equal(_bits(y[b, :lens[b]]), _bits(want)), (d, lens[b])


def test_rows_do_not_depend_on_the_batch(table):
    """Each row alone, with 3 more columns of pitch, and in place in pools at odd offsets: the bits of the NaN-padded batch."""
    RV, M = _rv(), _mix()
    rows, _, got = table
    assert np.array_equal(_bits(_batch(rows, extra=3)), _bits(got))
    for b, (x, h) in enumerate(rows):
        alone = _batch([(x, h)])
        assert np.array_equal(_bits(alone[0]), _bits(got[b, :len(x)])), (len(x), len(h))
    # pools: a one-sample member in front makes every offset odd or even as it falls; NaN members between the rows
    nan1 = np.full(1, NAN, dtype=np.float32)
    cp = M.SignalPool([s for x, _ in rows for s in (nan1, x)])
    rp = RV.RirPool([s for _, h in rows for s in (nan1, h)])
    assert sum(o % 2 for o in cp.offsets[1::2]) >= 3 and sum(o % 2 for o in rp.offsets[1::2]) >= 3
    B = len(rows)
    L = got.shape[1]
    d = M.Draw(list(range(1, 2 * B, 2)), [0] * B, [len(x) for x, _ in rows], [0] * B, [0] * B, [0.0] * B, [-25.0] * B)
    y = RV.reverb_draw(cp, rp, d, list(range(1, 2 * B, 2)), L).cpu().numpy()
    assert np.array_equal(_bits(y), _bits(got))


def test_taps(table):
    RV = _rv()
    rows, _, _ = table
    for b in (1, 4, 6):                                                # K = 16, 33, 1024
        x, h = rows[b]
        K = len(h)
        xs, hs = torch.from_numpy(x)[None].cuda(), torch.from_numpy(h)[None].cuda()
        for t in sorted({15, 16, 17, K - 1, K} & set(range(1, K + 1))):
            a = RV.reverb(xs, hs, taps=t)
            c = RV.reverb(xs, hs[:, :t].contiguous())
            assert np.array_equal(_bits(a), _bits(c)), (K, t)
            ref, S = R.reverb(x, h, taps=t)
            _within(a.cpu().numpy()[0], ref, S, t, (K, t))


def test_history_of_a_segment():
    """reverb_draw on segments inside a recording against the whole recording convolved and cut."""
    RV, M = _rv(), _mix()
    rec = R.speech_row(9000, 300)
    worst = 0.0
    for K in (17, 1000):
        h = R.rir_row(K, 310 + K)
        ref, S = R.reverb(rec, h)
        cp, rp = M.SignalPool([R.speech_row(33, 301), rec]), RV.RirPool([h])
        starts = [0, 1, 15, K - 2, K - 1, K + 100]
        n = 4200
        d = M.Draw([1] * 6, starts, [n] * 6, [0] * 6, [0] * 6, [0.0] * 6, [-25.0] * 6)
        y = RV.reverb_draw(cp, rp, d, [0] * 6, n + 5).cpu().numpy()
        for b, s0 in enumerate(starts):
            assert not y[b, n:].any()
            worst = max(worst, _within(y[b, :n], ref[s0:s0 + n], S[s0:s0 + n], K, (K, s0)))
    print(f"reverb_draw with history: worst error over the bound {worst:.3f}")


@pytest.fixture(scope="module")
def pools():
    RV, M = _rv(), _mix()
    cp = M.SignalPool([R.speech_row(n, 400 + k) for k, n in enumerate((9000, 4096, 700, 12001))])
    npool = M.SignalPool([(0.1 * np.random.default_rng(500 + k).standard_normal(m)).astype(np.float32) for k, m in enumerate((5000, 333))])
    rp = RV.RirPool([R.rir_row(K, 600 + k) for k, K in enumerate((1024, 300, 17))])
    return cp, npool, rp


def test_dynamic_mixtures_with_a_pool(pools):
    RV, M = _rv(), _mix()
    cp, npool, rp = pools
    B, n = 4, 4096
    plain = M.DynamicMixtures(cp, npool, B, samples=n, seed=5)
    dm = M.DynamicMixtures(cp, npool, B, samples=n, seed=5, rir_pool=rp, p_reverb=0.5)
    early = M.DynamicMixtures(cp, npool, B, samples=n, seed=5, rir_pool=rp, p_reverb=0.5, target="early", early_ms=5.0)
    seen = set()
    for k in range(4):
        d = dm.draw(k)
        assert d == plain.draw(k)
        ids = RV.draw_reverb(k, 5, len(rp), B, 0.5)
        got = dm.batch(k, info=True)
        assert got[3]["rir_id"] == ids
        seen |= {r >= 0 for r in ids}
        base = plain.batch(k)
        for b, r in enumerate(ids):                                      # dry rows: the rows of the same draw without a pool
            if r < 0:
                for s in range(3):
                    assert np.array_equal(_bits(got[s][b]), _bits(base[s][b])), (k, b, s)
        wet = RV.reverb_draw(cp, rp, d, ids, n)
        want = M.mix_draw(cp, npool, d, n, clean=wet)
        for s in range(3):
            assert np.array_equal(_bits(got[s]), _bits(want[s])), (k, s)
        assert np.array_equal(got[3]["g_clean"].cpu().numpy(), want[3]["g_clean"].cpu().numpy())
        assert [len(t) for t in got[:3]] == [B] * 3 and len(dm.batch(k)) == 3
        # target="early": float32(g_clean x the row under the early taps), the mixture and the noise unchanged
        e = early.batch(k, info=True)
        short = RV.reverb_draw(cp, rp, d, ids, n, taps=rp.early_taps(5.0))
        exp = (e[3]["g_clean"].cpu().numpy()[:, None] * short.cpu().numpy().astype(np.float64)).astype(np.float32)
        assert np.array_equal(_bits(e[1]), _bits(exp)), k
        assert np.array_equal(_bits(e[0]), _bits(got[0])) and np.array_equal(_bits(e[2]), _bits(got[2]))
        for b, r in enumerate(ids):
            if r < 0:
                assert np.array_equal(_bits(e[1][b]), _bits(base[1][b]))
            elif rp.early_taps(5.0)[r] < rp.lengths[r]:
                assert not np.array_equal(_bits(e[1][b]), _bits(got[1][b]))
    assert seen == {True, False}                                        # wet and dry rows both occurred
    assert rp.peaks == RV.rir_peaks([rp.member(k).cpu() for k in range(len(rp))]) and rp.early_taps(5.0) == [min(m, pk + 81) for m, pk in
                                                                                                            zip(rp.lengths, rp.peaks)]


def test_without_a_pool_nothing_changes(pools):
    M = _mix()
    cp, npool, _ = pools
    dm = M.DynamicMixtures(cp, npool, 4, samples=4096, seed=11, rir_pool=None)
    got = dm.batch(0, info=True)
    want = M.mix_draw(cp, npool, M.draw_batch(0, 11, cp.lengths, npool.lengths, 4, 4096), 4096)
    for s in range(3):
        assert np.array_equal(_bits(got[s]), _bits(want[s]))
    assert "rir_id" not in got[3] and set(got[3]) == set(want[3])


def test_mix_draw_checks_the_clean_tensor(pools):
    M = _mix()
    cp, npool, _ = pools
    d = M.draw_batch(0, 11, cp.lengths, npool.lengths, 4, 4096)
    for clean, what in ((torch.zeros(3, 4096, device="cuda"), "\\[4, 4096\\]"), (torch.zeros(4, 4095, device="cuda"), "\\[4, 4096\\]"),
                        (torch.zeros(4, 4096, device="cuda", dtype=torch.float64), "float32"), (torch.zeros(4096, device="cuda"), "\\[B, L\\]")):
        with pytest.raises(ValueError, match=what):
            M.mix_draw(cp, npool, d, 4096, clean=clean)


def test_reverb_draw_guards_raise_before_device_work(pools):
    RV, M = _rv(), _mix()
    cp, npool, rp = pools
    d = M.Draw([0, 3], [10, 0], [4096, 4096], [0, 0], [0, 0], [5.0, 5.0], [-25.0, -25.0])
    ok = dict(clean_pool=cp, rir_pool=rp, draw=d, rir_ids=[0, -1], samples=4096)
    RV.reverb_draw(**ok)
    bad = [(dict(rir_pool=npool), "RirPool"), (dict(clean_pool=None), "SignalPool"), (dict(samples=0), "samples"), (dict(samples=4096.0), "samples"),
           (dict(samples=4095), "row 0"), (dict(rir_ids=[0]), "rir_ids"), (dict(rir_ids="ab"), "rir_ids"), (dict(rir_ids=[0, 3]), "impulse response 3"),
           (dict(rir_ids=[-2, 0]), "impulse response -2"), (dict(rir_ids=[0, 1.0]), "row 1 does not hold integers"),
           (dict(draw=d._replace(clean_id=[0, 4])), "recording 4"), (dict(draw=d._replace(clean_start=[9000 - 4095, 0])), "row 0"),
           (dict(draw=d._replace(clean_start=[-1, 0])), "row 0"), (dict(draw=d._replace(lens=[4096, 0])), "row 1"),
           (dict(draw=d._replace(clean_id=[0])), "every field"), (dict(taps=[1024, 300]), "2 values of taps"),
           (dict(taps=[1025, 300, 17]), "taps\\[0\\]"), (dict(taps=[1024, 0, 17]), "taps\\[1\\]"), (dict(taps=[1, 1, 1.5]), "integers")]
    for kw, what in bad:
        with pytest.raises(ValueError, match="reverb_draw: .*" + what):
            RV.reverb_draw(**dict(ok, **kw))
    with pytest.raises(ValueError, match="pools are on"):
        class Elsewhere(RV.RirPool):
            device = torch.device("cuda", 7)
        other = Elsewhere.__new__(Elsewhere)
        RV.reverb_draw(cp, other, d, [0, -1], 4096)
    with pytest.raises(ValueError, match="RirPool.*response 0"):
        RV.RirPool([torch.zeros((1 << 16) + 1, device="cuda")])
