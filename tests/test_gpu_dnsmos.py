"""DNSMOS P.835 on the MI355X (csrc/dnsmos.hip through dnsmos.py and inference.compute_dnsmos / dnsmos_list) against the float64
definition tests/dnsmos_ref.py and the fixtures of tests/golden/make_dnsmos_golden.py.  The conv kernel is tested alone at the
smallest shapes that reach its edges; the whole network runs on 2 - 3 segments per test."""
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

import dnsmos_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("SIG_raw", "BAK_raw", "OVRL_raw", "SIG", "BAK", "OVRL")


def _mod():
    return importlib.import_module("i-dccrn-vae_amd.dnsmos")


def _inf():
    return importlib.import_module("i-dccrn-vae_amd.inference")


def _lib():
    return importlib.import_module("i-dccrn-vae_amd._lib")


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _weights(sfx=""):
    return R.load_weights(os.path.join(GOLDEN, f"dnsmos_weights{sfx}.npz"), os.path.join(GOLDEN, f"dnsmos_frontend{sfx}.npz"))


@pytest.fixture(scope="module")
def models():
    D = _mod()
    return {sfx: D.DNSMOS(_weights(sfx), personalized=bool(sfx)) for sfx in ("", "_personalized")}


def _relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


# ------------------------------------------------------------------------------------------------------- 1. the conv alone
# (N, H, W, Cin, Cout, pool).  The kernel's workgroup tile is 16 rows x 16 columns of output pixels (idv_conv3x3_tile, asserted
# below), its K chunk 32 input channels: (2, 17, 17, ..) and (1, 17, 18, ..) are one row and one (two) columns more than a tile.
CONV_CASES = [(1, 1, 1, 32, 32, 0), (2, 3, 5, 128, 64, 0), (1, 2, 161, 64, 64, 0), (3, 7, 33, 64, 32, 1), (2, 5, 40, 32, 32, 1),
              (1, 9, 80, 32, 32, 1), (1, 4, 20, 32, 64, 0), (2, 17, 17, 64, 64, 0), (1, 17, 18, 32, 32, 1)]


def _conv_ref(x, w, b, pool):
    out = []
    for img in x:
        y = R.conv3x3(img, w, b)
        out.append(R.pool2x2(y) if pool else y)
    return np.stack(out)


def _conv_data(case, integer):
    N, H, W, ci, co, pool = case
    rng = np.random.default_rng(sum(case) + 17 * integer)
    if integer:      # |sum| <= 9 * 128 * 3 * 3 + 3 < 2^24: every partial sum is an integer that fp32 holds exactly
        return (rng.integers(-3, 4, (N, H, W, ci)).astype(np.float64), rng.integers(-3, 4, (co, ci, 3, 3)).astype(np.float64),
                rng.integers(-3, 4, co).astype(np.float64))
    return rng.standard_normal((N, H, W, ci)), rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci), rng.standard_normal(co)


def _conv_dev(x, w, b, pool):
    D = _mod()
    return D.conv3x3(_cuda(x), D.conv3x3_pack(_cuda(w)), _cuda(b), w.shape[0], bool(pool))


def test_conv_tile_is_what_the_cases_assume():
    lib = _lib().lib()
    assert (lib.idv_conv3x3_tile(0), lib.idv_conv3x3_tile(1)) == (16, 16)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_exact_integer_parity(case):
    """Small-integer inputs, weights and biases: every sum is exact in fp32, so the device must equal the definition bit for bit --
    indexing, halo, padding and pooling errors show with no tolerance."""
    x, w, b = _conv_data(case, True)
    want = _conv_ref(x, w, b, case[5])
    got = _conv_dev(x, w, b, case[5]).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got, want.astype(np.float32))
    assert want.max() > 0 and (want == 0).any()          # both sides of the ReLU occur


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_float_parity(case):
    """Random floats against float64: relerr < 2e-5, the bound of the fp32 convs in tests/test_gpu_ops.py (_conv_case)."""
    x, w, b = _conv_data(case, False)
    x, w, b = (v.astype(np.float32).astype(np.float64) for v in (x, w, b))
    want = _conv_ref(x, w, b, case[5])
    got = _conv_dev(x, w, b, case[5]).cpu().numpy()
    err = _relerr(got, want)
    print(f"conv {case}: relerr {err:.3e}")
    assert err < 2e-5


@pytest.mark.parametrize("integer", [True, False])
def test_conv_global_max(integer):
    """(1, 4, 20, 32, 64, 0) followed by the global max over the map (idv_conv3x3_gmax)."""
    L = _lib()
    case = (1, 4, 20, 32, 64, 0)
    x, w, b = _conv_data(case, integer)
    x, w, b = (v.astype(np.float32).astype(np.float64) for v in (x, w, b))
    want = _conv_ref(x, w, b, 0).max(axis=(1, 2))
    y = _conv_dev(x, w, b, 0)
    g = torch.empty(1, 64, dtype=torch.float32, device="cuda")
    L.call("idv_conv3x3_gmax", L.p(y), L.i(1), L.ll(80), L.i(64), L.p(g), L.stream_ptr())
    assert torch.equal(g[0], y.reshape(80, 64).amax(dim=0))
    if integer:
        np.testing.assert_array_equal(g.cpu().numpy(), want.astype(np.float32))
    else:
        assert _relerr(g.cpu().numpy(), want) < 2e-5


@pytest.mark.parametrize("N,H,W", [(2, 3, 7), (1, 2, 161), (1, 17, 19)])
@pytest.mark.parametrize("integer", [True, False])
def test_first_layer_alone_and_fused(N, H, W, integer):
    """The 1 -> 128 layer on the vector ALU (idv_conv3x3_c1_fwd) against the definition, and the same layer evaluated inside the
    staging of the 128 -> 64 layer (idv_conv3x3_c1_fused_fwd): the same bits as the two separate launches, exact with integers
    (|layer 1| <= 9 * 3 * 3 + 3 = 84, |layer 2 sum| <= 1152 * 84 * 3 + 3 < 2^24), relerr < 2e-5 against float64 with floats."""
    D, L = _mod(), _lib()
    rng = np.random.default_rng(N * 1000 + H * 10 + W + integer)
    if integer:
        f, w1, b1 = rng.integers(-3, 4, (N, H, W)), rng.integers(-3, 4, (128, 1, 3, 3)), rng.integers(-3, 4, 128)
        w2, b2 = rng.integers(-3, 4, (64, 128, 3, 3)), rng.integers(-3, 4, 64)
    else:
        f, w1, b1 = rng.standard_normal((N, H, W)), rng.standard_normal((128, 1, 3, 3)) / 3, rng.standard_normal(128)
        w2, b2 = rng.standard_normal((64, 128, 3, 3)) / np.sqrt(1152), rng.standard_normal(64)
    f, w1, b1, w2, b2 = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (f, w1, b1, w2, b2))
    want1 = _conv_ref(f[..., None], w1, b1, 0)
    want2 = _conv_ref(want1, w2, b2, 0)
    fd, w1d, b1d, b2d = _cuda(f), _cuda(w1.reshape(128, 9)), _cuda(b1), _cuda(b2)
    wp = D.conv3x3_pack(_cuda(w2))
    y1 = torch.empty(N, H, W, 128, dtype=torch.float32, device="cuda")
    L.call("idv_conv3x3_c1_fwd", L.p(fd), L.p(w1d), L.p(b1d), L.i(N), L.i(H), L.i(W), L.i(128), L.p(y1), L.stream_ptr())
    y2 = D.conv3x3(y1, wp, b2d, 64, False)
    yf = torch.empty(N, H, W, 64, dtype=torch.float32, device="cuda")
    L.call("idv_conv3x3_c1_fused_fwd", L.p(fd), L.p(w1d), L.p(b1d), L.i(128), L.p(wp), L.p(b2d), L.i(N), L.i(H), L.i(W), L.i(64), L.i(0),
           L.p(yf), L.stream_ptr())
    assert torch.equal(yf, y2)
    if integer:
        np.testing.assert_array_equal(y1.cpu().numpy(), want1.astype(np.float32))
        np.testing.assert_array_equal(yf.cpu().numpy(), want2.astype(np.float32))
    else:
        assert _relerr(y1.cpu().numpy(), want1) < 2e-5
        assert _relerr(yf.cpu().numpy(), want2) < 2e-5


def test_conv_refusals():
    L = _lib()
    x = torch.zeros(1, 4, 4, 32, device="cuda")
    y = torch.zeros(1, 4, 4, 32, device="cuda")
    w = torch.zeros(32 * 9 * 32, device="cuda")
    b = torch.zeros(32, device="cuda")
    for N, H, W, ci, co, pool in ((0, 4, 4, 32, 32, 0), (1, 4, 4, 48, 32, 0), (1, 4, 4, 32, 16, 0), (1, 1, 4, 32, 32, 1)):
        with pytest.raises(L.IdvError, match="invalid argument"):
            L.call("idv_conv3x3_fwd", L.p(x), L.p(w), L.p(b), L.i(N), L.i(H), L.i(W), L.i(ci), L.i(co), L.i(pool), L.p(y), L.stream_ptr())
    with pytest.raises(L.IdvError, match="invalid argument"):
        L.call("idv_conv3x3_fwd", L.p(None), L.p(w), L.p(b), L.i(1), L.i(4), L.i(4), L.i(32), L.i(32), L.i(0), L.p(y), L.stream_ptr())


# ------------------------------------------------------------------------------------------------------------ 2. front end
GARBAGE = float("nan")          # behind every row's end: one read of it would poison the row


def _padded(rows, width=None):
    width = width or max(len(r) for r in rows)
    x = np.full((len(rows), width), GARBAGE, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return _cuda(x), [len(r) for r in rows]


def _tiled_segments(row):
    return R.script_segments(np.asarray(row))[0]


def test_front_end_feature_of_two_segments(models):
    """The feature maps of two segments against the float64 definition.  The bound follows from the arithmetic: an fmaf chain of n = 320
    terms is off by at most g sum|x_k m_k|, g = n u / (1 - n u), u = 2^-24; re^2, im^2, their sum, the square root and its square add
    at most 6 u to the relative error r of p; the feature ln(p) / 2.3026 is then off by at most -ln(1 - r) / 2.3026 plus one rounding
    of the result.  Elements with r >= 1/2 (a bin whose power cancels to nothing) are left out; they must stay below 0.1 %."""
    m = models[""]
    rows = [R.signal("noise", 144161), R.signal("tone", 150000, 1)]
    x, lens = _padded(rows)
    got = m.features(x, lens).cpu().numpy().astype(np.float64)
    assert got.shape == (2, 900, 161)
    t = m.tensors
    u = 2.0 ** -24
    g = 320 * u / (1 - 320 * u)
    skipped = 0
    for s, row in enumerate(rows):
        seg = _tiled_segments(row)[0]
        fr = R.frames(seg).astype(np.float64)
        want = R.feature(seg, t)
        re, im = fr @ t["fe_re"].astype(np.float64).T, fr @ t["fe_im"].astype(np.float64).T
        dre, dim = g * (np.abs(fr) @ np.abs(t["fe_re"]).astype(np.float64).T), g * (np.abs(fr) @ np.abs(t["fe_im"]).astype(np.float64).T)
        p = re * re + im * im
        r = (2 * np.abs(re) * dre + dre * dre + 2 * np.abs(im) * dim + dim * dim) / p + 6 * u
        ok = r < 0.5
        skipped += int((~ok).sum())
        bound = -np.log1p(-np.where(ok, r, 0)) / float(t["log_div"]) + u * np.abs(want) + 1e-12
        dev = np.abs(got[s] - want)
        print(f"front end segment {s}: max |dev - f64| {dev[ok].max():.3e}, max bound {bound[ok].max():.3e}, left out {int((~ok).sum())}")
        assert np.all(dev[ok] <= bound[ok])
        assert p.min() > float(t["log_floor"])           # no digital silence in these signals
    assert skipped < 2 * 900 * 161 / 1000


def _integer_front_ends(t):
    """Integer stand-ins for the two learned matrices under which p = re^2 + im^2 is a perfect square below 2^24, so sqrt and its
    square are exact and the device must equal the definition bit for bit: (a) (re, im) = (3 a, 4 a); (b) re on the even bins
    only, im on the odd bins only, from different matrices."""
    rng = np.random.default_rng(5)
    m0 = rng.integers(-1, 2, (161, 320)).astype(np.float32)
    m1, m2 = rng.integers(-2, 3, (161, 320)).astype(np.float32), rng.integers(-2, 3, (161, 320)).astype(np.float32)
    m1[1::2] = 0
    m2[0::2] = 0
    for re, im in ((3 * m0, 4 * m0), (m1, m2)):
        t2 = dict(t)
        t2["fe_re"], t2["fe_im"] = re, im
        yield t2


def test_front_end_wraps_at_the_right_sample_and_reads_nothing_behind_a_row(models):
    """Integer-valued clips of 1, 144161 and 100000 samples (the last one wraps inside its second and third segment) and one
    all-zero row, NaN behind every row's end, integer stand-ins for the matrices: bit for bit the definition applied to the clip the
    script tiles.  The all-zero row is exactly ln(1e-12) / 2.3025851 everywhere."""
    D = _mod()
    rng = np.random.default_rng(11)
    rows = [np.array([2.0], dtype=np.float32), rng.integers(-2, 3, 144161).astype(np.float32), rng.integers(-2, 3, 100000).astype(np.float32),
            np.zeros(150000, dtype=np.float32)]
    x, lens = _padded(rows, 150004)
    segs, counts = D.plan_segments(lens)
    assert counts == [7, 1, 3, 1]
    for t2 in _integer_front_ends(models[""].tensors):
        got = D.DNSMOS(t2).features(x, lens).cpu().numpy()
        assert got.shape == (12, 900, 161) and np.isfinite(got).all()
        k = 0
        for row in rows:
            for seg in _tiled_segments(row):
                want = R.feature(seg, t2).astype(np.float32)
                np.testing.assert_array_equal(got[k], want)
                k += 1
        floor = np.float32(np.log(np.float64(t2["log_floor"])) / np.float64(t2["log_div"]))
        assert np.all(got[11] == floor) and abs(float(floor) + 12.0) < 1e-5


# --------------------------------------------------------------------------------------------------------- 3. independence
def test_rows_do_not_depend_on_the_batch_or_the_workspace(models):
    """Lengths [16000, 144160, 200000, 7] in one padded batch with NaN behind every row's end: row b equals that clip scored alone
    bit for bit, the workspace bound set to one segment changes nothing, and num_hops is the planner's."""
    D = _mod()
    m = models[""]
    lens = [16000, 144160, 200000, 7]
    rows = [R.signal(kind, n, 3 + k) for k, (kind, n) in enumerate(zip(("noise", "tone", "speechlike", "noise"), lens))]
    x, _ = _padded(rows)
    out = m.score(x, lens, per_segment=True)
    assert out["num_hops"].tolist() == [D.num_hops(n)[1] for n in lens] == [7, 1, 3, 5]
    assert out["segments"].tolist() == D.plan_segments(lens)[1]
    assert all(torch.isfinite(out[k]).all() for k in NAMES)
    one = D.DNSMOS(m.tensors, workspace_segments=1).score(x, lens, per_segment=True)
    three = D.DNSMOS(m.tensors, workspace_segments=3).score(x, lens, per_segment=True)
    for k in NAMES + ("segments_raw",):
        assert torch.equal(one[k], out[k]) and torch.equal(three[k], out[k]), k
    for b, row in enumerate(rows):
        alone = m.score(_cuda(row)[None])
        for k in NAMES:
            assert torch.equal(alone[k][0], out[k][b]), (b, k)


# ------------------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("sfx", ["", "_personalized"])
def test_end_to_end_within_four_float32_floors(models, sfx):
    """The fixture signals (3 segments) on the real weights against tests/golden/dnsmos_expected.npz: |device - float64| per raw value
    <= 4 x the worst |float32 host - float64| the fixture stores for the same signals and weights (the factor 4: an accumulation order
    that differs from the host GEMM's over K up to 1152).  The clip means of the raw values obey the same bound; the polynomial
    columns the bound times the largest slope of the polynomial over the raw values' range.

    Measured on the MI355X (profiles/dnsmos/measure.json): the float32 host's largest deviation 1.77e-6 (personalized
    weights: 1.65e-6), so the bound is 7.07e-6 (6.59e-6); the device's largest deviation 2.36e-6 (1.17e-6)."""
    exp = np.load(os.path.join(GOLDEN, "dnsmos_expected.npz"))
    m = models[sfx]
    sigs = (("tone", 144160), ("speechlike", 176000))
    floor = max(np.abs(exp[f"{k}{sfx}.raw32"] - exp[f"{k}{sfx}.raw64"]).max() for k, _ in sigs)
    bound = 4 * floor
    x, lens = _padded([R.signal(k, n) for k, n in sigs])
    out = m.score(x, lens, per_segment=True)
    raw = out["segments_raw"].cpu().numpy().astype(np.float64)
    want = np.concatenate([exp[f"{k}{sfx}.raw64"] for k, _ in sigs])
    dev = np.abs(raw - want).max()
    print(f"dnsmos{sfx}: float32 floor {floor:.3e}, bound {bound:.3e}, device max |raw - f64| {dev:.3e}")
    assert raw.shape == want.shape == (3, 3)
    assert dev <= bound
    D = _mod()
    slope = max(np.abs(np.polyder(np.poly1d(c))(np.linspace(0.5, 5.5, 501))).max() for c in D.POLY[bool(sfx)])
    assert out["num_hops"].tolist() == [int(exp[f"{k}{sfx}.num_hops"]) for k, _ in sigs]
    for b, (k, _) in enumerate(sigs):
        clip = exp[f"{k}{sfx}.clip64"]
        for j, name in enumerate(NAMES):
            assert abs(float(out[name][b]) - clip[j]) <= bound * (1 if j < 3 else slope), (k, name)


# ----------------------------------------------------------------------------------------------------------- 5. dnsmos_list
def test_dnsmos_list_keeps_the_callers_order(models):
    inf = _inf()
    m = models[""]
    lens = [50000, 7, 176000, 16000, 144160]
    sigs = [_cuda(R.signal(("noise", "tone", "speechlike")[k % 3], n, 20 + k)) for k, n in enumerate(lens)]
    got = inf.dnsmos_list(sigs, m, max_batch=2)
    assert got["num_hops"].tolist() == [3, 5, 2, 7, 1]
    for k, s in enumerate(sigs):
        one = inf.compute_dnsmos(s, m)
        for name in NAMES:
            assert got[name].dtype == torch.float64 and float(got[name][k]) == float(one[name]), (k, name)
    with pytest.raises(ValueError):
        m.score(_cuda(np.zeros((2, 100))), [100, 0])
