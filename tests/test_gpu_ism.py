"""Image-source room impulse responses on the MI355X (csrc/ism.hip through dataset.rir.shoebox_rir, RirPool.shoebox and
DynamicMixtures) against the float64 definition of tests/ism_ref.py, computed once per module.

The bound per sample:  |y - ref| <= ulp32(ref) + (N_n + C) 2^-53 S_n,  N_n the images touching sample n and
S_n = sum |A_i| w_i(n), both from the reference.  C = 335 is the per-term evaluation constant in units of 2^-53 (one correctly rounded
operation = 1, a function within k ulp = 2 k), from the kernel's operation count with the OpenCL bounds for double that the device
library is held to (sqrt and division correctly rounded, sin and cos 4 ulp, pow 16 ulp), plus the reference's own:
  device  A = gx gy gz / (4 pi d): six pow 192, five products 5, (4 pi) d 1, the division 1                             199
          sin(pi f) 9, A sin 1, pi u 1, the division 1, the last product 1                                                 13
          window cos^2: table entry 10, cos / sin(pi f / 81) 10, product 1, doubled where the two products cancel
          (|u| <= 39.5: by at most 2) 42, the sum 1, squared 86 + 1                                                        87
  numpy   A 19, sin(pi f) 3, pi u 1, division 1, two products 2, the window (1 + cos(2 pi u / 81)) / 2 times |sinc| <= 1 / (pi |u|)
          relative to w 10                                                                                                 36
tau, u and f are the reference's bit for bit (the same IEEE operations in the same order), so no term moves.  The worst ratio of
every case is kept as ism_bound.json by the error-table helper of tests/test_gpu_backward.py."""
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

import ism_ref as R  # noqa: E402
from test_gpu_backward import _dump  # noqa: E402

pytestmark = pytest.mark.gpu

C_TERM = 335
FS, CS = 16000.0, 343.0
ROOM = (3.1, 2.7, 2.4)
SRC, MIC = (1.1, 0.9, 1.3), (2.2, 1.7, 1.1)
BETA = (0.9, -0.7, 0.8, 0.0, 0.6, 0.85)           # six different walls, one negative, one zero
D100 = 100 * CS / FS                              # a direct path of exactly 100 samples


def _rir():
    return importlib.import_module("i-dccrn-vae_amd.dataset.rir")


def _rv():
    return importlib.import_module("i-dccrn-vae_amd.dataset.reverb")


def _mix():
    return importlib.import_module("i-dccrn-vae_amd.dataset.mix")


def _ops():
    return importlib.import_module("i-dccrn-vae_amd.ops")


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


def _cases():
    """(tag, room, source, mic, beta, K, max_order)"""
    out = [(f"K{K}", ROOM, SRC, MIC, BETA, K, None) for K in (1, 40, 41, 63, 64, 65, 255, 256, 257, 1000, 2048)]
    near = (SRC[0] + 0.05, SRC[1], SRC[2])                                     # the direct window straddles n = 0
    out.append(("near", ROOM, SRC, near, BETA, 300, None))
    out.append(("integer", (5.0, 4.0, 3.0), (1.0, 2.0, 1.5), (1.0 + D100, 2.0, 1.5), (0.9, -0.7, 0.8, 0.5, 0.6, 0.85), 257, None))
    out.append(("large", (6.2, 5.1, 3.3), (2.1, 3.9, 1.3), (4.0, 1.7, 1.9), (0.93, 0.9, 0.88, 0.91, 0.86, 0.95), 4000, None))
    return out


def _order_cases():
    return [(f"order{o}", ROOM, SRC, MIC, BETA, 1000, o) for o in (0, 1, 3)]


def _run(cases, **kw):
    RI = _rir()
    mo = [c[6] for c in cases]
    return RI.shoebox_rir([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases],
                          max_order=None if mo[0] is None else mo, **kw)


@pytest.fixture(scope="module")
def table():
    """Every case: its reference (h32, h64, N, S, images) and its device row, from one launch per group."""
    rows = {}
    for group in (_cases(), _order_cases()):
        y = _run(group).cpu().numpy()
        for b, c in enumerate(group):
            rows[c[0]] = (c, R.rir(c[1], c[2], c[3], c[4], c[5], FS, CS, c[6], detail=True), y[b])
    return rows


def test_parity_within_the_bound(table):
    worst = {}
    for tag, (c, (h32, h64, N, S, nimg), y) in table.items():
        K = c[5]
        assert y.dtype == np.float32 and np.isfinite(y[:K]).all(), tag
        err = np.abs(y[:K].astype(np.float64) - h64)
        bound = R.ulp32(h64) + (N + C_TERM) * 2.0 ** -53 * S
        ratio = float((err / bound).max())
        worst[tag] = {"taps": K, "images": nimg, "worst_ratio": ratio, "bits_equal": bool((_bits(y[:K]) == _bits(h32)).all())}
        print(tag, worst[tag])
    _dump("ism_bound", worst)
    for tag, w in worst.items():
        assert w["worst_ratio"] <= 1.0, (tag, w)
    assert table["large"][1][4] > 20000 and table["K2048"][1][2].max() > 50      # the cases are what they are meant to be


def test_windows_straddle_both_ends(table):
    """The near case has a window over n = 0 and every long case images past K - 1 that still reach it: the reference says so, and
    the device agrees there within the bound (asserted above); here the samples themselves are looked at."""
    c, (h32, h64, N, S, _), y = table["near"]
    tau0 = 0.05 * FS / CS
    assert tau0 < 40.5 and N[0] >= 1 and h64[0] != 0.0
    c, (h32, h64, N, S, _), y = table["K1000"]
    tau, _ = R.images(c[1], c[2], c[3], c[4], c[5], FS, CS, None)
    assert (tau > c[5] - 1).any() and N[c[5] - 1] > 1
    assert abs(float(y[c[5] - 1]) - h64[-1]) <= R.ulp32(h64[-1]) + (N[-1] + C_TERM) * 2.0 ** -53 * S[-1]


def test_single_image_is_exact():
    """beta = 0 and a direct path of exactly 100 samples: one sample float32(1 / (4 pi d)) and zeros, bit for bit."""
    y = _rir().shoebox_rir((5.0, 4.0, 3.0), (1.0, 2.0, 1.5), (1.0 + D100, 2.0, 1.5), [0.0] * 6, 300).cpu().numpy()[0]
    want = np.zeros(300, dtype=np.float32)
    want[100] = np.float32(1.0 / (4.0 * np.pi * D100))
    assert (_bits(y) == _bits(want)).all()


def test_rows_end_where_their_taps_end_and_nothing_else_is_written():
    """A batch of different K written into a NaN-filled buffer of a wider pitch: zeros from taps[b] to Kmax, NaN left behind it."""
    OPS, RI = _ops(), _rir()
    cases = [c for c in _cases() if c[0] in ("K1", "K41", "K257", "near", "K65")]
    geom, tp, mo = RI.check_rooms([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases],
                                  [c[5] for c in cases])
    B, Kmax = len(cases), max(tp)
    buf = torch.full((B, Kmax + 37), float("nan"), device="cuda")
    taps = torch.tensor(tp, dtype=torch.int32).cuda()
    OPS.ism_rir(torch.from_numpy(geom).cuda(), taps, None, B, Kmax, out=buf)
    got = buf.cpu().numpy()
    assert np.isnan(got[:, Kmax:]).all()
    for b, K in enumerate(tp):
        assert np.isfinite(got[b, :K]).all() and (_bits(got[b, K:Kmax]) == 0).all(), b
    # room b of a batch of 5 equals the room run alone, bit for bit; and two calls return the same bits
    again = _run(cases).cpu().numpy()
    assert (_bits(again) == _bits(got[:, :Kmax])).all()
    for b, c in enumerate(cases):
        alone = _run([c]).cpu().numpy()
        assert alone.shape == (1, c[5]) and (_bits(alone[0]) == _bits(got[b, :c[5]])).all(), c[0]


def test_tile_counts_add_up_to_the_image_count(table):
    """The work buffer: per tile the images summed and the images owned; a row's owned images are the reference's image set."""
    OPS, RI = _ops(), _rir()
    cases = [table[tag][0] for tag in ("K1", "K257", "K1000", "large", "near")]
    geom, tp, _ = RI.check_rooms([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases],
                                 [c[5] for c in cases])
    _, counts = OPS.ism_rir(torch.from_numpy(geom).cuda(), torch.tensor(tp, dtype=torch.int32).cuda(), None, len(cases), max(tp))
    counts = counts.cpu().numpy()
    assert counts.shape == (len(cases), (max(tp) + 63) // 64, 2)
    for b, c in enumerate(cases):
        nimg, used = table[c[0]][1][4], (c[5] + 63) // 64
        assert counts[b, :, 1].sum() == nimg and (counts[b, used:] == 0).all(), c[0]
        assert counts[b, :, 0].sum() >= nimg and (counts[b, :, 0] >= counts[b, :, 1]).all(), c[0]


def test_a_shorter_response_is_the_beginning_of_a_longer_one(table):
    full = table["K2048"][2]
    for tag in ("K1", "K40", "K41", "K255", "K256", "K257", "K1000"):
        K = table[tag][0][5]
        assert (_bits(table[tag][2][:K]) == _bits(full[:K])).all(), tag


def test_peaks_first_on_ties():
    OPS, RV = _ops(), _rv()
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((6, 700)).astype(np.float32)
    taps = [700, 1, 300, 513, 256, 700]
    rows[0, 600] = rows[0, 17] = -9.0                      # a tie, of two signs in row 5: the first wins
    rows[5, 699] = 9.5
    rows[5, 3] = -9.5
    rows[2, 400] = 50.0                                    # past the row's taps: not seen
    rows[3, 512] = 20.0                                    # the last sample, in a third block of 256
    h = torch.full((6, 731), float("nan"))
    h[:, :700] = torch.from_numpy(rows)
    h = h.cuda()[:, :700]
    got = OPS.ism_peaks(h, torch.tensor(taps, dtype=torch.int32).cuda()).cpu().tolist()
    want = RV.rir_peaks([rows[b, :taps[b]] for b in range(6)])
    assert got == want and got[0] == 17 and got[5] == 3 and got[3] == 512


def test_pool_from_the_device_rows_equals_the_pool_from_the_host_rows():
    RV, MX = _rv(), _mix()
    cases = [c for c in _cases() if c[0] in ("K257", "near", "K1000", "integer")]
    args = ([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], [c[5] for c in cases])
    rows = _run(cases).cpu()
    host = RV.RirPool([rows[b, :c[5]].clone() for b, c in enumerate(cases)])
    dev = RV.RirPool.shoebox(*args)
    assert isinstance(dev, RV.RirPool) and dev.device == host.device and dev.fs == host.fs == 16000
    assert dev.lengths == host.lengths and dev.offsets == host.offsets and dev.peaks == host.peaks and dev.unit_offset == host.unit_offset
    assert dev.data.dtype == torch.float32 and (_bits(dev.data) == _bits(host.data)).all()
    assert dev.early_taps(50.0) == host.early_taps(50.0)
    rng = np.random.default_rng(11)
    clean = MX.SignalPool([torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 0.05) for n in (9000, 4000, 2500)])
    noise = MX.SignalPool([torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 0.05) for n in (5000, 7000)])
    for target in ("reverberant", "early"):
        a = MX.DynamicMixtures(clean, noise, 3, samples=4000, seed=7, rir_pool=host, p_reverb=0.7, target=target)
        b = MX.DynamicMixtures(clean, noise, 3, samples=4000, seed=7, rir_pool=dev, p_reverb=0.7, target=target)
        for k in (0, 1):
            for ta, tb in zip(a.batch(k), b.batch(k)):
                assert (_bits(ta) == _bits(tb)).all(), (target, k)
