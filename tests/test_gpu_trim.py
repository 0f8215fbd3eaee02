"""Silence trimming on the MI355X (csrc/trim.hip through inference.trim / trim_list and dataset.dataload.segment_index) against the
float64 host definition of tests/trim_ref.py.  Rows of at most 16385 samples; the references are computed once per module."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import trim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(2048, 512), (1024, 256), (256, 64)]             # (frame_length, hop_length)
TOP_DB = (20.0, 30.0, 45.0)
MARGIN_DB = 1e-6      # a frame this far from the threshold in the reference is on the same side in any double log10
LMAX = max(R.LENGTHS)


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.inference"), importlib.import_module("i-dccrn-vae_amd.ops"),
            importlib.import_module("i-dccrn-vae_amd.dataset.dataload"))


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


@pytest.fixture(scope="module")
def ref():
    """The PCM16 rows of trim_ref.cases() and, per frame size, their float64 frame powers and their bounds per top_db."""
    rows = R.cases()
    table = {"rows": rows, "lens": [len(r) for r in rows]}
    for frame, hop in SIZES:
        table[(frame, hop)] = ([R.frame_power(r, frame, hop) for r in rows],
                               {td: [R.trim(r, td, frame, hop) for r in rows] for td in TOP_DB})
    return table


@pytest.fixture(scope="module")
def noise_ref():
    """0.1 N(0, 1) float32 rows of the same lengths and their float64 frame powers at (2048, 512)."""
    rows = [(0.1 * np.random.default_rng(2000 + k).standard_normal(n)).astype(np.float32) for k, n in enumerate(R.LENGTHS)]
    return rows, [R.frame_power(r) for r in rows]


@pytest.mark.parametrize("frame,hop", SIZES)
def test_bounds_are_exact(ref, frame, hop):
    """bounds == trim_ref.trim as integers for top_db in {20, 30, 45}, every length in one NaN-padded batch.  The condition that makes
    this a statement about the kernel and not about a log10: every frame of every case stands at least 1e-6 dB from the threshold in
    the reference (the nearest one: 0.16 dB at (2048, 512), 0.036 dB at (1024, 256), 0.0074 dB at (256, 64))."""
    inf, _, _ = _mods()
    rows, lens = ref["rows"], ref["lens"]
    x = _padded(rows)
    nearest = min(R.margin_db(r, td, frame, hop) for r in rows for td in TOP_DB)
    print(f"trim ({frame}, {hop}): nearest frame {nearest:.4g} dB from a threshold")
    assert nearest >= MARGIN_DB
    for td in TOP_DB:
        want = ref[(frame, hop)][1][td]
        y, out_lens, bounds = inf.trim(x, td, lengths=lens, frame_length=frame, hop_length=hop)
        assert bounds == want, (td, [(n, g, w) for n, g, w in zip(lens, bounds, want) if g != w])
        assert out_lens == [e - s for s, e in want] and y.shape == (len(rows), max(out_lens))
        assert all(isinstance(v, int) for be in bounds for v in be)
    if (frame, hop) == (2048, 512):
        want = ref[(frame, hop)][1][30.0]
        assert sum((s > 0) + (e < n) for (s, e), n in zip(want, lens)) == 15          # the ends that are genuinely cut


@pytest.mark.parametrize("frame,hop", SIZES)
def test_frame_powers_of_pcm16_rows_are_bit_exact(ref, frame, hop):
    """Samples k / 32768: every sum of squares is an integer below 2^53 times 2^-30 and the frame length a power of two, so no order
    of summation can change P; the device's float64 powers equal the reference's bit for bit, with zeros behind a row's own frames."""
    inf, _, _ = _mods()
    rows, lens = ref["rows"], ref["lens"]
    _, _, _, P = inf.trim(_padded(rows), 30.0, lengths=lens, frame_length=frame, hop_length=hop, power=True)
    assert P.dtype == torch.float64 and P.shape == (len(rows), 1 + LMAX // hop)
    P = P.cpu().numpy()
    for b, want in enumerate(ref[(frame, hop)][0]):
        T = 1 + lens[b] // hop
        assert want.shape == (T,) and np.array_equal(P[b, :T].view(np.int64), want.view(np.int64)), (lens[b],)
        assert not P[b, T:].any()


def test_frame_powers_of_float32_rows_within_the_summation_bound(noise_ref):
    """0.1 N(0, 1) rows: |P_device - P_reference| <= 2 (frame - 1) 2^-53 P_reference = 4.6e-13 at 2048.  Derived, not measured: the
    squares are exact in double on both sides, and each of the two sums of N = frame non-negative terms errs by at most (N - 1) u
    relative to its value, u = 2^-53, whatever its order; the division by the power of two is exact.

    Measured on the MI355X: worst relative error 3.3e-16, three orders below the bound."""
    inf, _, _ = _mods()
    rows, want = noise_ref
    lens = [len(r) for r in rows]
    _, _, _, P = inf.trim(_padded(rows), 30.0, lengths=lens, power=True)
    P = P.cpu().numpy()
    bound = 2 * (R.FRAME - 1) * 2.0 ** -53
    worst = max(float((np.abs(P[b, :len(w)] - w) / w).max()) for b, w in enumerate(want))
    print(f"trim frame power, float32 rows: worst relative error {worst:.3e}, bound {bound:.3e}")
    assert all((w > 0).all() for w in want)
    assert worst <= bound


@pytest.mark.parametrize("which", ["pcm16", "float32"])
def test_rows_are_independent(ref, noise_ref, which):
    """NaN at and past every row's end; row pitches LMAX (odd: the rows start 0, 4, 8 and 12 bytes past a 16-byte boundary), LMAX + 2,
    LMAX + 3 and LMAX + 77: every row's bounds and frame powers are bit-identical to that row alone at B = 1 (16-byte aligned).  The
    float32 rows make this a statement about the order of the sums, which the exact PCM16 sums cannot see."""
    inf, _, _ = _mods()
    rows = ref["rows"] if which == "pcm16" else noise_ref[0]
    lens = [len(r) for r in rows]
    alone = []
    for r in rows:
        _, n1, b1, P1 = inf.trim(torch.from_numpy(r).cuda(), 30.0, power=True)
        assert P1.shape == (1 + len(r) // 512,) and n1 == [b1[0][1] - b1[0][0]]
        alone.append((b1[0], P1))
    for extra in (0, 2, 3, 77):
        x = _padded(rows, extra=extra)
        assert x.stride(0) == LMAX + extra
        _, _, bounds, P = inf.trim(x, 30.0, lengths=torch.tensor(lens), power=True)
        assert torch.isfinite(P).all()
        for b, (b1, P1) in enumerate(alone):
            assert bounds[b] == b1, (extra, lens[b])
            assert torch.equal(_bits(P[b, :P1.shape[0]]), _bits(P1)), (extra, lens[b])
    # no lengths: every row is full; and a batch of one is the row alone
    k = lens.index(LMAX)
    _, _, b_full, P_full = inf.trim(_padded(rows[k:k + 1]), 30.0, power=True)
    assert b_full == [alone[k][0]] and torch.equal(_bits(P_full[0]), _bits(alone[k][1]))


def test_gather(ref):
    """y[b, :n_b] is bit-equal to x[b, start:end], everything behind it exactly zero, out_lengths = end - start."""
    inf, ops, _ = _mods()
    rows, lens = ref["rows"], ref["lens"]
    for extra in (0, 3):                                                             # an odd and a 16-byte row pitch
        x = _padded(rows, extra=extra)
        y, out_lens, bounds = inf.trim(x, 30.0, lengths=lens)
        assert bounds == ref[(2048, 512)][1][30.0] and y.dtype == torch.float32 and y.shape == (len(rows), max(out_lens))
        y = y.cpu().numpy()
        for b, (s, e) in enumerate(bounds):
            assert out_lens[b] == e - s and np.array_equal(y[b, :e - s].view(np.int32), rows[b][s:e].view(np.int32)), lens[b]
            assert not y[b, e - s:].any() and np.isfinite(y[b]).all()
    # one row, 1-D in and out
    k = lens.index(12000)
    y1, n1, b1 = inf.trim(torch.from_numpy(rows[k]).cuda())
    assert b1 == [ref[(2048, 512)][1][30.0][k]] and y1.shape == (n1[0],)
    assert np.array_equal(y1.cpu().numpy(), rows[k][b1[0][0]:b1[0][1]])
    # stationary noise: nothing to cut, the values come back as they went in
    flat = [(np.round(0.1 * np.random.default_rng(3000 + k).standard_normal(n) * 32768) / 32768).astype(np.float32)
            for k, n in enumerate((513, 2049, 4097, 12000))]
    assert [R.trim(r) for r in flat] == [(0, len(r)) for r in flat]
    y, out_lens, bounds = inf.trim(_padded(flat), lengths=[len(r) for r in flat])
    assert bounds == [(0, len(r)) for r in flat] and out_lens == [len(r) for r in flat] and y.shape == (4, 12000)
    for b, r in enumerate(flat):
        assert np.array_equal(y[b, :len(r)].cpu().numpy(), r) and not y[b, len(r):].any()
    # rows of zeros and rows wholly below amin are returned untrimmed, a row of length 0 has the empty span
    n = 5000
    x = torch.full((4, n), float("nan"))
    x[0], x[1], x[2, :3000], x[3] = 0.0, 1e-6, 1e-6, 0.25
    lens4 = ops.Lengths([n, n, 3000, 0], "cuda")
    bdev, P = ops.trim_bounds(x.cuda(), 30.0, 2048, 512, lens4, power=True)
    assert bdev.dtype == torch.int32 and bdev.tolist() == [[0, n], [0, n], [0, 3000], [0, 0]]
    assert not P[0].any() and float(P[1].max()) < 1e-10 and not P[3].any()
    y = ops.trim_gather(x.cuda(), bdev, n).cpu()
    assert not y[0].any() and torch.equal(y[1], x[1]) and torch.equal(y[2, :3000], x[2, :3000]) and not y[2, 3000:].any() and not y[3].any()
    # every row trimmed to nothing: [B, 0]
    assert ops.trim_gather(x.cuda(), torch.zeros(4, 2, dtype=torch.int32, device="cuda"), 0).shape == (4, 0)


def test_trim_list_equals_the_calls_one_by_one(ref):
    """Mixed lengths in batches of three: results in the caller's order, bit-identical to the per-signal trim call."""
    inf, _, _ = _mods()
    pick = [17, 0, 12, 5, 19, 8, 14, 2, 11, 18]
    sig = [torch.from_numpy(ref["rows"][k]).cuda() for k in pick]
    got, bounds = inf.trim_list(sig, 30.0, max_batch=3)
    assert bounds == [ref[(2048, 512)][1][30.0][k] for k in pick] == inf.trim_bounds_list(sig, 30.0, max_batch=4)
    cut = 0
    for k, s, g, be in zip(pick, sig, got, bounds):
        y1, n1, b1 = inf.trim(s, 30.0)
        assert b1 == [be] and g.shape == y1.shape == (n1[0],) and torch.equal(_bits(g), _bits(y1)), R.LENGTHS[k]
        assert torch.equal(g, s[be[0]:be[1]])
        cut += g.shape[0] < s.shape[0]
    assert cut >= 5
    got45, bounds45 = inf.trim_list(sig, top_db=45.0, max_batch=64)
    assert bounds45 == [ref[(2048, 512)][1][45.0][k] for k in pick] and [g.shape[0] for g in got45] == [e - s for s, e in bounds45]


def test_segment_index_end_to_end(ref, tmp_path):
    """PCM16 wav files with silent ends: segment_index(trim=True) equals segments_from_bounds fed with the reference's bounds, in file
    order, and differs from the untrimmed index."""
    _, _, dl = _mods()
    hop, seq = 100, 31                                                               # 3000-sample segments
    files, want, plain = [], [], []
    for k in (19, 11, 17, 9, 18, 0):                                                 # 16385, 4095, 12000, 2048, 16000 and 1 samples
        f = str(tmp_path / f"mix_fileid_{k}.wav")
        wavfile.write(f, 16000, np.round(ref["rows"][k].astype(np.float64) * 32768).astype(np.int16))
        assert np.array_equal(dl.read_wav(f)[0], ref["rows"][k])
        files.append(f)
        beg, end = ref[(2048, 512)][1][30.0][k]
        want += dl.segments_from_bounds(f, beg, end, hop, seq)
        plain += dl.segments_from_bounds(f, 0, R.LENGTHS[k], hop, seq)
    empty = str(tmp_path / "mix_fileid_99.wav")
    wavfile.write(empty, 16000, np.zeros(0, dtype=np.int16))
    files.append(empty)
    assert dl.segment_index(files, hop, seq, 16000) == plain
    got = dl.segment_index(files, hop, seq, 16000, trim=True, max_batch=4)
    assert got == want and got != plain and len(want) < len(plain)
    assert [t[1] for t in want if t[0] == files[0]] == [3584, 6584, 9584]           # 10752 samples from 3584 on: three segments, not five
    assert dl.segment_index(files, hop, seq, 16000, trim=True, top_db=45.0, device="cuda:0") != got
    ds = dl.SpeechSequencesFull(files, None, name="trimmed", sr=16000, hop=hop, sequence_len=seq, cache_dir=str(tmp_path), trim=True)
    assert ds.valid_seq_list == want and np.array_equal(ds[0], ref["rows"][19][3584:6584])
    with pytest.raises(ValueError, match="sampling rate"):
        dl.segment_index(files, hop, seq, 8000, trim=True)
