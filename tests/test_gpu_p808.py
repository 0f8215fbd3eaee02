"""The P808_MOS column of DNSMOS on the MI355X (csrc/p808.hip and the pooled first layer of csrc/dnsmos.hip through dnsmos.P808,
DNSMOS.score(p808=) and inference.compute_dnsmos / dnsmos_list) against the float64 definition tests/p808_ref.py and the fixtures of
tests/golden/make_p808_golden.py.  Every case runs on 3 segments or fewer, on cut-down maps, or on the batch of
test_gpu_dnsmos.test_rows_do_not_depend_on_the_batch_or_the_workspace."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dnsmos_ref as R  # noqa: E402
import p808_ref as P  # noqa: E402
from test_gpu_dnsmos import NAMES, _conv_data, _conv_dev, _conv_ref, _cuda, _padded, _relerr, _tiled_segments  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _mod():
    return importlib.import_module("i-dccrn-vae_amd.dnsmos")


def _inf():
    return importlib.import_module("i-dccrn-vae_amd.inference")


def _lib():
    return importlib.import_module("i-dccrn-vae_amd._lib")


@pytest.fixture(scope="module")
def p808():
    return _mod().P808.from_npz(os.path.join(GOLDEN, "p808_weights.npz"))


@pytest.fixture(scope="module")
def p835():
    return _mod().DNSMOS(R.load_weights(os.path.join(GOLDEN, "dnsmos_weights.npz"), os.path.join(GOLDEN, "dnsmos_frontend.npz")))


# ------------------------------------------------------------------------------------------------------------ 1. mel power
def test_mel_power_exact_with_integer_tables(p808):
    """Integer stand-ins for the DFT table (-1 .. 1) and the mel matrix (0 .. 2), integer clips (-2 .. 2) of 1, 7, 100000 and 144161
    samples and an all-zero row, NaN behind every row's end: |re|, |im| <= 642, p < 2^20, S < 2^29, so every sum is an exact integer
    in double and S must equal the definition bit for bit.  The 144161-sample clip carries 1000 at samples 144000 and 144160: neither
    is part of audio_seg[:-160].  The 100000-sample clip wraps inside a frame, the 1-sample clip at every sample."""
    D = _mod()
    rng = np.random.default_rng(808)
    long = rng.integers(-2, 3, 144161).astype(np.float32)
    long[144000] = long[144160] = 1000.0
    rows = [np.array([2.0], dtype=np.float32), rng.integers(-2, 3, 7).astype(np.float32), rng.integers(-2, 3, 100000).astype(np.float32), long,
            np.zeros(150000, dtype=np.float32)]
    x, lens = _padded(rows, 150004)
    assert D.plan_segments(lens)[1] == [7, 5, 3, 1, 1]
    dft = np.zeros((2, 161, 324))
    dft[:, :, :321] = rng.integers(-1, 2, (2, 161, 321))
    mel = rng.integers(0, 3, (120, 161)).astype(np.float64)
    m = D.P808(p808.tensors, dft=dft, mel=mel)
    S, smax = m.mel_power(x, lens)
    S, smax = S.cpu().numpy(), smax.cpu().numpy()
    assert S.shape == (17, 900, 120) and S.dtype == np.float64 and np.isfinite(S).all()
    k = 0
    for row in rows:
        for seg in _tiled_segments(row):
            want = P.mel_power(seg[:-160], power=lambda a: P.power_table(a, (dft[0, :, :321], dft[1, :, :321])), basis=mel).T
            np.testing.assert_array_equal(S[k], want)
            assert smax[k] == want.max()
            k += 1
    assert k == 17 and not S[16].any() and 0 < S[:16].max() < 2 ** 29


def test_mel_power_with_the_real_tables(p808):
    """signal("noise", 144161) and signal("speechlike", 176000) (3 segments) against the float64 definition.  u = 2^-53; a double chain
    of n terms is off by at most g_n sum |x_k y_k|, g_n = n u / (1 - n u): dre = g_324 sum |x| |cos w| (dim alike), dp = 2 |re| dre +
    dre^2 + 2 |im| dim + dim^2 + 3 u p, dM = basis dp + g_164 basis p, r = dM / M.  The feature, 10 log10(M / max) / 40 + 1 rounded to
    float32 once, then stands within spacing(float32(want)) / 2 + (10 / (40 ln 10)) (r + r_max) of the definition, r_max the r of the
    maximum element.  Elements with r >= 2^-30 may be left out, at most 0.1 %; on these signals the largest r of an element that
    top_db keeps alive is 9.1e-11 (noise) / 1.5e-10 (speechlike), so none is.  Measured on the MI355X: the largest deviation is 2.98e-8,
    the float32 rounding of the feature itself (deviation / bound <= 1.000 in every element)."""
    rows = [R.signal("noise", 144161), R.signal("speechlike", 176000)]
    x, lens = _padded(rows)
    got = p808.features(x, lens).cpu().numpy().astype(np.float64)
    assert got.shape == (3, 900, 120)
    u = 2.0 ** -53

    def g(n):
        return n * u / (1 - n * u)
    c, s = P.dft_tables()
    basis = P.mel_basis().astype(np.float64)
    k = left_out = 0
    for row in rows:
        for seg in _tiled_segments(row):
            want = P.feature64(seg)
            fr = P.frames(seg[:-160].astype(np.float64))
            re, im = fr @ c.T, fr @ s.T
            dre, dim = g(324) * (np.abs(fr) @ np.abs(c).T), g(324) * (np.abs(fr) @ np.abs(s).T)
            p = re * re + im * im
            dp = 2 * np.abs(re) * dre + dre * dre + 2 * np.abs(im) * dim + dim * dim + 3 * u * p
            M = p @ basis.T
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(M > 0, (dp @ basis.T + g(164) * M) / M, np.inf)
            r_max = r.flat[np.argmax(M)]
            live = r < 2.0 ** -30
            bound = np.abs(np.spacing(want.astype(np.float32))).astype(np.float64) / 2 + 10 / (40 * np.log(10)) * (np.where(live, r, 0) + r_max)
            dev = np.abs(got[k] - want)
            alive = want > -1.0
            print(f"p808 feature segment {k}: max |dev - f64| {dev[live].max():.3e}, max dev / bound {(dev[live] / bound[live]).max():.3f}, "
                  f"r_max {r_max:.2e}, largest r kept alive by top_db {r[alive].max():.2e}, left out {int((~live).sum())}")
            assert r_max < 2.0 ** -30
            assert np.all(dev[live] <= bound[live])
            left_out += int((~live).sum())
            k += 1
    assert k == 3 and left_out <= 3 * 900 * 120 / 1000


# -------------------------------------------------------------------------------------------------------------- 2. decibels
def test_db_kernel_alone():
    """idv_p808_db on hand-made maps of 1000 elements, eight segments in one call (the maximum is per segment): the maximum in the first
    and in the last element; elements at exactly 1e-8 max and one double above and below; elements below amin = 1e-10, under a loud and
    under a maximum that is itself below amin; all zero; two segments 120 dB apart.  Exactly 1.0 / -1.0 where the definition is, within
    one float32 spacing elsewhere."""
    L = _lib()
    rng = np.random.default_rng(8)
    per = 1000

    def rand(scale):
        return scale * 10.0 ** rng.uniform(-11, 0, per)
    S = np.stack([rand(5.0), rand(5.0), rand(3.7), rand(1e-3), rand(5e-11), np.zeros(per), rand(1e6), rand(1e-6)])
    S[0, 0], S[1, -1], S[2, 500], S[3, 17], S[6, 3], S[7, 999] = 5.0, 5.0, 3.7, 1e-3, 1e6, 1e-6
    t = 1e-8 * 3.7
    S[2, 10:13] = np.nextafter(t, 0), t, np.nextafter(t, 1)
    S[3, 100:103] = 1e-11, 1e-12, 0.0
    S[4, 5] = 9.9e-11
    smax = S.max(axis=1)
    feat = torch.empty(8, per, dtype=torch.float32, device="cuda")
    L.call("idv_p808_db", L.p(_cuda(S, np.float64)), L.p(_cuda(smax, np.float64)), L.i(8), L.ll(per), L.p(feat), L.stream_ptr())
    got = feat.cpu().numpy()
    want = np.stack([(P.power_to_db(row) + 40) / 40 for row in S])
    w32 = want.astype(np.float32)
    exact = (want == 1.0) | (want == -1.0)
    np.testing.assert_array_equal(got[exact], w32[exact])
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.abs(np.spacing(w32)))
    assert (got[2, 10:13] == -1.0).all() and got[2, 500] == 1.0 and got[0, 0] == 1.0 and got[1, -1] == 1.0
    # under a maximum of 1e-3, M = 1e-11, 1e-12 and 0 are all held at amin: 70 dB below the maximum, one value above the clamp
    assert (got[3, 100:103] == got[3, 100]).all() and abs(float(got[3, 100]) + 0.75) < 1e-6
    assert (got[4] == 1.0).all() and (got[5] == 1.0).all()
    assert got[6, 3] == 1.0 and got[7, 999] == 1.0 and exact.sum() > per and (~exact).sum() > per
    assert got.min() == -1.0 and got.max() == 1.0


# ----------------------------------------------------------------------------------------------------- 3. the convolutions
def _c1_pool(f, w1, b1, N, H, W, C):
    L = _lib()
    y = torch.empty(N, H // 2, W // 2, C, dtype=torch.float32, device="cuda")
    L.call("idv_conv3x3_c1_pool_fwd", L.p(f), L.p(w1), L.p(b1), L.i(N), L.i(H), L.i(W), L.i(C), L.p(y), L.stream_ptr())
    return y


@pytest.mark.parametrize("N,H,W", [(2, 3, 7), (1, 2, 120), (1, 17, 19)])
@pytest.mark.parametrize("integer", [True, False])
def test_first_layer_with_its_pool(N, H, W, integer):
    """idv_conv3x3_c1_pool_fwd is bit for bit the 2x2 floor max-pool of idv_conv3x3_c1_fwd's map (odd last row / column dropped), and
    with integers the definition's."""
    L = _lib()
    rng = np.random.default_rng(N * 1000 + H * 10 + W + integer)
    if integer:
        f, w1, b1 = rng.integers(-3, 4, (N, H, W)), rng.integers(-3, 4, (32, 1, 3, 3)), rng.integers(-3, 4, 32)
    else:
        f, w1, b1 = rng.standard_normal((N, H, W)), rng.standard_normal((32, 1, 3, 3)) / 3, rng.standard_normal(32)
    f, w1, b1 = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (f, w1, b1))
    fd, w1d, b1d = _cuda(f), _cuda(w1.reshape(32, 9)), _cuda(b1)
    full = torch.empty(N, H, W, 32, dtype=torch.float32, device="cuda")
    L.call("idv_conv3x3_c1_fwd", L.p(fd), L.p(w1d), L.p(b1d), L.i(N), L.i(H), L.i(W), L.i(32), L.p(full), L.stream_ptr())
    want = F.max_pool2d(full.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    got = _c1_pool(fd, w1d, b1d, N, H, W, 32)
    assert got.shape == want.shape == (N, H // 2, W // 2, 32)
    assert torch.equal(got, want) and got.max() > 0 and (got == 0).any()
    if integer:
        np.testing.assert_array_equal(got.cpu().numpy(), _conv_ref(f[..., None], w1, b1, 1).astype(np.float32))


def test_first_layer_with_its_pool_refusals():
    L = _lib()
    f, w, b, y = (torch.zeros(n, device="cuda") for n in (64, 288, 32, 4096))
    for N, H, W, C in ((1, 1, 8, 32), (1, 8, 1, 32), (0, 4, 4, 32), (1, 4, 4, 0), (1, 4, 4, 2048)):
        with pytest.raises(L.IdvError, match="invalid argument"):
            L.call("idv_conv3x3_c1_pool_fwd", L.p(f), L.p(w), L.p(b), L.i(N), L.i(H), L.i(W), L.i(C), L.p(y), L.stream_ptr())
    with pytest.raises(L.IdvError, match="invalid argument"):
        L.call("idv_conv3x3_c1_pool_fwd", L.p(f), L.p(None), L.p(b), L.i(1), L.i(4), L.i(4), L.i(32), L.p(y), L.stream_ptr())


# (N, H, W, Cin, Cout, pool): the widths 60, 30 and 15 of this network's maps -- 15 is less than one column tile of 16 -- at heights
# that are no multiple of the row tile
P808_CONV_CASES = [(2, 18, 15, 32, 64, 0), (1, 17, 30, 32, 32, 1), (1, 5, 60, 32, 32, 1)]


@pytest.mark.parametrize("case", P808_CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_at_the_widths_of_this_network(case):
    """idv_conv3x3_fwd, unchanged, at the new shapes: exact on small integers, relerr < 2e-5 against float64 on floats (the bound of
    test_gpu_dnsmos.test_conv_float_parity)."""
    x, w, b = _conv_data(case, True)
    want = _conv_ref(x, w, b, case[5])
    got = _conv_dev(x, w, b, case[5]).cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want.astype(np.float32))
    x, w, b = (v.astype(np.float32).astype(np.float64) for v in _conv_data(case, False))
    err = _relerr(_conv_dev(x, w, b, case[5]).cpu().numpy(), _conv_ref(x, w, b, case[5]))
    print(f"conv {case}: relerr {err:.3e}")
    assert err < 2e-5


# --------------------------------------------------------------------------------------------------------- 4. independence
def test_rows_do_not_depend_on_the_batch_or_the_workspace(p808, p835):
    """Lengths [16000, 144160, 200000, 7] in one padded batch with NaN behind every row's end: P808_MOS of row b equals that clip
    scored alone bit for bit, workspace_segments 1 and 3 change nothing, and SIG / BAK / OVRL with p808= are bitwise those without."""
    D = _mod()
    lens = [16000, 144160, 200000, 7]
    rows = [R.signal(kind, n, 3 + k) for k, (kind, n) in enumerate(zip(("noise", "tone", "speechlike", "noise"), lens))]
    x, _ = _padded(rows)
    out = p808.score(x, lens, per_segment=True)
    assert out["segments"].tolist() == D.plan_segments(lens)[1] == [7, 1, 3, 5]
    assert out["P808_MOS"].dtype == torch.float64 and out["segments_p808"].shape == (16,) and torch.isfinite(out["P808_MOS"]).all()
    for ws in (1, 3):
        other = D.P808(p808.tensors, workspace_segments=ws).score(x, lens, per_segment=True)
        assert torch.equal(other["P808_MOS"], out["P808_MOS"]) and torch.equal(other["segments_p808"], out["segments_p808"]), ws
    for b, row in enumerate(rows):
        alone = p808.score(_cuda(row)[None])
        assert torch.equal(alone["P808_MOS"][0], out["P808_MOS"][b]), b
    plain = p835.score(x, lens, per_segment=True)
    both = p835.score(x, lens, per_segment=True, p808=p808)
    assert sorted(set(both) - set(plain)) == ["P808_MOS", "segments_p808"]
    for k in NAMES + ("segments_raw", "num_hops", "segments"):
        assert torch.equal(both[k], plain[k]), k
    assert torch.equal(both["P808_MOS"], out["P808_MOS"]) and torch.equal(both["segments_p808"], out["segments_p808"])
    assert "P808_MOS" not in p835.score(x[1:2], [lens[1]])


# ------------------------------------------------------------------------------------------------------------ 5. end to end
def test_end_to_end_within_four_float32_floors(p808):
    """The fixture signals (3 segments) on the real weights against tests/golden/p808_expected.npz: |device - float64| per segment <=
    4 x the worst |float32 host - float64| the fixture stores (the rule and the factor of
    test_gpu_dnsmos.test_end_to_end_within_four_float32_floors: an accumulation order that differs from the host's over K <= 288).  The
    clip means obey the same bound.

    Measured on the MI355X (profiles/p808/measure.json): the float32 host's largest deviation 2.13e-7, so the bound is
    8.51e-7; the device's largest deviation 3.21e-7 (its values 2.2027535, 2.2153683, 2.1865363)."""
    exp = np.load(os.path.join(GOLDEN, "p808_expected.npz"))
    sigs = (("tone", 144160), ("speechlike", 176000))
    floor = max(np.abs(exp[f"{k}.raw32"] - exp[f"{k}.raw64"]).max() for k, _ in sigs)
    bound = 4 * floor
    x, lens = _padded([R.signal(k, n) for k, n in sigs])
    out = p808.score(x, lens, per_segment=True)
    raw = out["segments_p808"].cpu().numpy().astype(np.float64)
    want = np.concatenate([exp[f"{k}.raw64"] for k, _ in sigs])
    dev = np.abs(raw - want).max()
    print(f"p808: float32 floor {floor:.3e}, bound {bound:.3e}, device max |raw - f64| {dev:.3e}, device values {raw.tolist()}")
    assert raw.shape == want.shape == (3,)
    assert dev <= bound
    for b, (k, _) in enumerate(sigs):
        assert abs(float(out["P808_MOS"][b]) - float(exp[f"{k}.clip64"])) <= bound, k
    speech = R.signal("speechlike", 176000)
    assert torch.equal(p808.raw(torch.stack([_cuda(speech[s:s + 144160]) for s in (0, 16000)])), out["segments_p808"][1:])


# ---------------------------------------------------------------------------------------------------- 6. list and refusals
def test_dnsmos_list_with_p808_keeps_the_callers_order(p808, p835):
    inf = _inf()
    lens = [50000, 7, 176000, 16000, 144160]
    sigs = [_cuda(R.signal(("noise", "tone", "speechlike")[k % 3], n, 20 + k)) for k, n in enumerate(lens)]
    got = inf.dnsmos_list(sigs, p835, max_batch=2, p808=p808)
    assert got["num_hops"].tolist() == [3, 5, 2, 7, 1] and got["P808_MOS"].dtype == torch.float64 and got["P808_MOS"].shape == (5,)
    for k, s in enumerate(sigs):
        one = inf.compute_dnsmos(s, p835, p808=p808)
        for name in NAMES + ("P808_MOS",):
            assert float(got[name][k]) == float(one[name]), (k, name)
        assert float(one["P808_MOS"]) == float(p808.score(s[None])["P808_MOS"][0])
    assert "P808_MOS" not in inf.compute_dnsmos(sigs[1], p835)
    with pytest.raises(ValueError):
        p835.score(sigs[1][None], p808=p835)


def test_entry_refusals():
    L = _lib()
    st = L.stream_ptr()
    x = torch.zeros(1, 200, device="cuda")
    lens, seg = torch.tensor([200], dtype=torch.int32, device="cuda"), torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    dft, mel = torch.zeros(2 * 161 * 324 + 1, dtype=torch.float64, device="cuda"), torch.zeros(120 * 161, dtype=torch.float64, device="cuda")
    S, smax, work = (torch.zeros(n, dtype=torch.float64, device="cuda") for n in (900 * 120, 1, 57))
    odd = dft.view(torch.float32)[1:]                            # 4 bytes past a double's alignment
    assert L.lib().idv_p808_mel_work_doubles(1) == 57 and L.lib().idv_p808_mel_work_doubles(0) == -1

    def mel_call(**kw):
        a = dict(x=x, ldx=200, lens=lens, B=1, seg=seg, nseg=1, dft=dft, mel=mel, S=S, smax=smax, work=work)
        a.update(kw)
        L.call("idv_p808_mel", L.p(a["x"]), L.ll(a["ldx"]), L.p(a["lens"]), L.i(a["B"]), L.p(a["seg"]), L.i(a["nseg"]), L.p(a["dft"]),
               L.p(a["mel"]), L.p(a["S"]), L.p(a["smax"]), L.p(a["work"]), st)
    mel_call()
    for kw in (dict(x=None), dict(dft=None), dict(work=None), dict(nseg=0), dict(B=0), dict(ldx=0), dict(dft=odd), dict(S=odd),
               dict(nseg=(1 << 20) + 1)):
        with pytest.raises(L.IdvError, match="invalid argument"):
            mel_call(**kw)
    feat = torch.zeros(900 * 120, device="cuda")
    for Sx, n, per in ((None, 1, 10), (S, 0, 10), (S, 1, 0), (odd, 1, 10)):
        with pytest.raises(L.IdvError, match="invalid argument"):
            L.call("idv_p808_db", L.p(Sx), L.p(smax), L.i(n), L.ll(per), L.p(feat), st)
    g, w, b, raw = (torch.zeros(n, device="cuda") for n in (64, 4096, 64, 4))
    for gx, N in ((None, 1), (g, 0)):
        with pytest.raises(L.IdvError, match="invalid argument"):
            L.call("idv_p808_head", L.p(gx), L.i(N), L.p(w), L.p(b), L.p(w), L.p(b), L.p(w), L.p(b), L.p(raw), st)
    first, count = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    for rx, nseg, B, out in ((None, 1, 1, smax), (raw, 0, 1, smax), (raw, 1, 0, smax), (raw, 1, 1, odd)):
        with pytest.raises(L.IdvError, match="invalid argument"):
            L.call("idv_p808_clip", L.p(rx), L.i(nseg), L.p(first), L.p(count), L.i(B), L.p(out), st)
    torch.cuda.synchronize()
