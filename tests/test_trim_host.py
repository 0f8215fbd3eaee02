"""CPU tests of silence trimming: the additive C ABI and its refusals, the host reference tests/trim_ref.py (the
yardstick of tests/test_gpu_trim.py), the index arithmetic of dataset/dataload.py on trimmed bounds and the host-side guards of
inference.trim / trim_list; no GPU needed."""
import importlib
import math
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

INF = importlib.import_module("i-dccrn-vae_amd.inference")
OPS = importlib.import_module("i-dccrn-vae_amd.ops")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")
DL = importlib.import_module("i-dccrn-vae_amd.dataset.dataload")


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_trim_work_bytes", "idv_trim_bounds", "idv_trim_gather"):
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_trim_work_bytes"] == ("long long", ["int", "int", "int"])
    assert protos["idv_trim_bounds"] == ("int", ["ptr", "long long", "ptr", "int", "int", "int", "int", "double", "ptr", "long long", "ptr",
                                                 "ptr", "long long", "ptr"])
    assert protos["idv_trim_gather"] == ("int", ["ptr", "long long", "ptr", "int", "int", "ptr", "long long", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries


def test_work_bytes():
    wb = LIB.lib().idv_trim_work_bytes
    # one double per hop-sample block and row, the last block of a row may be short
    assert wb(1, 1, 512) == 8 and wb(1, 512, 512) == 8 and wb(1, 513, 512) == 16 and wb(3, 16385, 512) == 3 * 33 * 8
    assert wb(64, 160000, 512) == 64 * 313 * 8 and wb(1, 1 << 27, 4) == (1 << 25) * 8 and wb(65535, 100, 64) == 65535 * 2 * 8
    for B, L, hop in ((0, 100, 512), (-1, 100, 512), (65536, 100, 512), (1, 0, 512), (1, -5, 512), (1, (1 << 27) + 1, 512), (1, 100, 0),
                      (1, 100, -512), (1, 100, 510), (1, 100, 2), (1, 100, (1 << 27) + 4), (1, 100, 1 << 30)):
        assert wb(B, L, hop) == -1, (B, L, hop)


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()

    def bounds(**kw):
        a = dict(x=8, ldx=1 << 28, lens=None, B=2, L=4096, frame=2048, hop=512, top_db=30.0, work=8, work_bytes=1 << 40, bounds=8,
                 power=None, ldp=0)
        a.update(kw)
        return lib.idv_trim_bounds(a["x"], a["ldx"], a["lens"], a["B"], a["L"], a["frame"], a["hop"], a["top_db"], a["work"],
                                   a["work_bytes"], a["bounds"], a["power"], a["ldp"], None)
    bad = [dict(x=None), dict(work=None), dict(bounds=None), dict(B=0), dict(B=-3), dict(L=0), dict(L=-1), dict(L=(1 << 27) + 1),
           dict(ldx=4095), dict(hop=0), dict(hop=-512), dict(hop=1 << 30, frame=2048), dict(hop=1 << 30, frame=-(1 << 31)), dict(hop=510, frame=2040), dict(hop=2, frame=8),
           dict(frame=2048 + 512), dict(frame=512), dict(frame=0), dict(frame=-2048), dict(hop=4, frame=4 * 66), dict(hop=16, frame=2048),
           dict(top_db=0.0), dict(top_db=-30.0), dict(top_db=math.inf), dict(top_db=math.nan),
           dict(work_bytes=2 * 8 * 8 - 1), dict(work_bytes=0),
           dict(power=8, ldp=8), dict(power=8, ldp=0)]
    for kw in bad:
        assert bounds(**kw) == -1, kw

    def gather(**kw):
        a = dict(x=8, ldx=4096, bounds=8, B=2, Lout=1000, y=8, ldy=1000)
        a.update(kw)
        return lib.idv_trim_gather(a["x"], a["ldx"], a["bounds"], a["B"], a["Lout"], a["y"], a["ldy"], None)
    for kw in (dict(x=None), dict(bounds=None), dict(y=None), dict(B=0), dict(B=-1), dict(ldy=999), dict(Lout=0), dict(Lout=-4)):
        assert gather(**kw) == -1, kw


def test_reference_frame_count_and_the_untrimmed_rows():
    rng = np.random.default_rng(0)
    for frame, hop in ((2048, 512), (1024, 256), (256, 64)):
        for n in (1, 2, hop - 1, hop, hop + 1, frame - 1, frame, frame + 1, 5 * hop + 7):
            x = rng.standard_normal(n)
            assert R.frame_power(x, frame, hop).shape == R.frame_db(x, frame, hop).shape == (1 + n // hop,) == (R.n_frames(n, hop),)
            s, e = R.trim(x, 30.0, frame, hop)
            assert 0 <= s < e <= n
            assert R.trim(np.zeros(n), 30.0, frame, hop) == (0, n)                 # db = 0 everywhere
            assert R.trim(np.full(n, 1e-6), 30.0, frame, hop) == (0, n)            # wholly below amin: power 1e-12 < 1e-10
            assert np.all(R.frame_db(np.full(n, 1e-6), frame, hop) == 0)
    for k, x in enumerate(R.cases()):
        for top_db in (20.0, 30.0, 45.0):
            s, e = R.trim(x, top_db)
            assert 0 <= s < e <= len(x) == R.LENGTHS[k] and s % 512 == 0 and (e % 512 == 0 or e == len(x))


def test_reference_by_hand():
    """4096 samples, loud in [1024, 2560) only (amplitude 0.5 over 1e-4): frame t covers samples [512 t - 1024, 512 t + 1024)."""
    x = np.full(4096, 1e-4)
    x[1024:2560] = 0.5
    P = R.frame_power(x)
    quiet, loud = 1e-4 ** 2, 0.5 ** 2
    want = np.array([0, 512, 1024, 1536, 1536, 1024, 512, 0, 0]) * loud + np.array([1024, 1024, 1024, 512, 512, 1024, 1536, 1536, 1024]) * quiet
    assert np.abs(P - want / 2048).max() <= 1e-14 * P.max()
    # P / max(P) = 1/3, 2/3, 1, 1, 2/3, 1/3 in frames 1 .. 6: -4.77 dB, -1.76 dB, 0; frames 0, 7, 8 are 74 dB down
    assert R.trim(x, 30.0) == (512, 3584) and R.trim(x, 4.0) == (1024, 3072) and R.trim(x, 1.0) == (1536, 2560)
    assert R.trim(x, 80.0) == (0, 4096)                                            # the last frame is number 8: end = min(n, 9 * 512)
    assert R.trim(x[:4000], 80.0) == (0, 4000)
    db = R.frame_db(x)
    assert abs(db[1] - 10 * np.log10((512 * loud + 1024 * quiet) / (1536 * loud + 512 * quiet))) < 1e-12 and db[3] == 0
    # one sample: one frame that holds it, never silent against itself
    assert R.frame_power(np.array([0.5])).tolist() == [0.25 / 2048] and R.trim(np.array([0.5])) == (0, 1)


def test_pcm16_frame_powers_are_exact():
    """The sums of k^2 are integers below 2^53 and the scale 2^-30 / frame a power of two: P is exact, whatever the order of the sum."""
    x = R.fade(16385, 99)
    k = np.round(x.astype(np.float64) * 32768).astype(np.int64)
    for frame, hop in ((2048, 512), (1024, 256), (256, 64)):
        kp = np.pad(k, frame // 2)
        sums = np.array([np.sum(kp[t * hop:t * hop + frame] ** 2) for t in range(1 + len(k) // hop)])
        assert sums.max() < 2 ** 53
        assert np.array_equal(R.frame_power(x, frame, hop), sums.astype(np.float64) / 2.0 ** 30 / frame)


def test_reference_matches_librosa():
    """The pin for a machine that has librosa >= 0.10 (parity with the package is unpinned where it is not installed)."""
    librosa = pytest.importorskip("librosa")
    for x in R.cases():
        for top_db in (20.0, 30.0, 45.0):
            _, (s, e) = librosa.effects.trim(x, top_db=top_db)
            assert (int(s), int(e)) == R.trim(x, top_db), (len(x), top_db)


def _reference_segments(wav, beg, end, hop, sequence_len):
    """compute_len of dataload_nsvae.py:141-148, written out."""
    seq_length = (sequence_len - 1) * hop
    file_length = end - beg
    n_seq = (1 + int(file_length / hop)) // sequence_len
    return [(wav, i * seq_length + beg, (i + 1) * seq_length + beg) for i in range(n_seq)]


def test_segments_from_bounds():
    hop, seq = 100, 31                                       # 3000-sample segments
    for n in (0, 2999, 3000, 3099, 3100, 9100, 48000):
        got = DL.segments_from_bounds("f.wav", 0, n, hop, seq)
        assert got == _reference_segments("f.wav", 0, n, hop, seq) and len(got) == (1 + n // hop) // seq
    for beg, end in ((512, 9100), (1536, 7680), (3584, 14336), (512, 3584), (0, 0), (1024, 1024 + 3100)):
        got = DL.segments_from_bounds("g.wav", beg, end, hop, seq)
        assert got == _reference_segments("g.wav", beg, end, hop, seq)
        assert all(a == beg + 3000 * i and b == a + 3000 for i, (_, a, b) in enumerate(got))
    # trimming removes a segment: 9100 samples hold two, the 5504 between the bounds hold one, which starts at the first bound
    assert len(DL.segments_from_bounds("g.wav", 0, 9100, hop, seq)) == 2
    assert DL.segments_from_bounds("g.wav", 3584, 9088, hop, seq) == [("g.wav", 3584, 6584)]
    assert DL.segments_from_bounds("g.wav", 3584, 6583, hop, seq) == []            # 2999 samples: 30 frames, a segment needs 31


def _write(path, n, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 0.1).clip(-1, 1)
    wavfile.write(path, 16000, (x * 32767).astype(np.int16))


def test_untrimmed_index_is_unchanged(tmp_path):
    """The files of tests/test_data_path.py: trim=False is the parent's loop, n_seq = (1 + n // hop) // sequence_len from sample 0."""
    hop, seq = 100, 31
    lens = [9100, 2999, 3100, 48000, 0]
    files = [str(tmp_path / f"mix_snr5_fileid_{k}.wav") for k in range(len(lens))]
    for k, (f, n) in enumerate(zip(files, lens)):
        _write(f, n, k)
    want = []
    for f, n in zip(files, lens):
        want += [(f, i * 3000, (i + 1) * 3000) for i in range((1 + int(n / hop)) // seq)]
    assert DL.segment_index(files, hop, seq, 16000) == want == DL.segment_index(files, hop, seq, 16000, trim=False, top_db=10.0)
    assert [sum(1 for t in want if t[0] == f) for f in files] == [2, 0, 1, 15, 0]
    with pytest.raises(ValueError, match="sampling rate"):
        DL.segment_index(files, hop, seq, 8000)


def test_trimmed_index_without_a_gpu_raises_before_a_file_is_opened(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    missing = str(tmp_path / "no_such_file.wav")
    with pytest.raises(RuntimeError, match="no host fallback"):
        DL.segment_index([missing], 100, 31, 16000, trim=True)
    with pytest.raises(RuntimeError, match="no host fallback"):
        DL.SpeechSequencesFull([missing], None, name="unit", cache_dir=str(tmp_path), trim=True)
    assert not os.path.exists(tmp_path / "unit_train.pkl")


def test_one_signal_items_and_the_config_keys(tmp_path):
    hop, seq = 100, 31
    files = [str(tmp_path / f"p_{k}.wav") for k in range(2)]
    for k, f in enumerate(files):
        _write(f, 6200 + 100 * k, k)
    ds = DL.SpeechSequencesFull(files, None, name="pre", sr=16000, hop=hop, sequence_len=seq, cache_dir=str(tmp_path))
    assert len(ds) == 2 + 2
    x = ds[1]
    assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.shape == (3000,)
    assert np.array_equal(x, DL.read_wav(files[0], 3000, 6000)[0])
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=3)))
    assert isinstance(batch, torch.Tensor) and batch.shape == (3, 3000)
    # the pretrained-VAE loader's own keys; [STFT] trim is read where present and reaches that loader (not the supervised one)
    from configparser import ConfigParser
    seen = []

    class Spy(DL.SpeechSequencesFull):
        def __init__(self, *a, **kw):
            seen.append(kw)
            kw = dict(kw, trim=False)
            super().__init__(*a, **kw)
    for trim_line, want in (("", False), ("trim = True\n", True), ("trim = False\n", False)):
        cfg = ConfigParser()
        cfg.read_string(f"[User]\ntrain_data_dir = {tmp_path}\nval_data_dir = {tmp_path}\nnoisy_train_data_dir = {tmp_path}\n"
                        f"noisy_val_data_dir = {tmp_path}\nclean_train_data_dir = {tmp_path}\nclean_val_data_dir = {tmp_path}\n"
                        f"noise_train_data_dir = {tmp_path}\nnoise_val_data_dir = {tmp_path}\n"
                        "[DataFrame]\ndataset_name = cfgunit\nbatch_size = 2\nshuffle = False\nnum_workers = 0\nsuffix = wav\n"
                        f"sequence_len = {seq}\n[STFT]\nhopfrac = {hop}\nfs = 16000\n{trim_line}")
        orig, DL.SpeechSequencesFull = DL.SpeechSequencesFull, Spy
        try:
            for mode in (dict(nsvae=True), dict(), dict(pretrained=True)):
                del seen[:]
                tr, va, n_tr, n_va = DL.build_dataloader(cfg, True, cache_dir=str(tmp_path), **mode)
                assert n_tr == n_va == 4 and len(seen) == 2
                for kw in seen:
                    assert kw.get("trim", False) == (want and bool(mode))
                    assert (kw["clean_file_dir"] is None) == ("pretrained" in mode)
                    assert ("noise_file_dir" in kw) == ("nsvae" in mode)
            with pytest.raises(ValueError, match="two different loaders"):
                DL.build_dataloader(cfg, True, nsvae=True, pretrained=True)
        finally:
            DL.SpeechSequencesFull = orig
    assert next(iter(tr)).shape == (2, 3000)                                       # the last one built: one signal per item


def test_guards_raise_before_gpu_work():
    x = torch.zeros(3, 5000)
    for kw in (dict(top_db=0), dict(top_db=-30.0), dict(top_db=float("inf")), dict(top_db=float("nan")), dict(top_db="30"),
               dict(top_db=True), dict(hop_length=0), dict(hop_length=510, frame_length=2040), dict(hop_length=512.0),
               dict(frame_length=2048 + 512), dict(frame_length=512), dict(hop_length=4, frame_length=4 * 66), dict(frame_length=True)):
        with pytest.raises(ValueError, match="trim: (top_db|frame_length|hop_length)"):
            INF.trim(x, **kw)
        with pytest.raises(ValueError, match="trim: (top_db|frame_length|hop_length)"):
            INF.trim_list([x[0]], **kw)
        with pytest.raises(ValueError, match="trim: (top_db|frame_length|hop_length)"):
            INF.trim_bounds_list([x[0]], **kw)
    with pytest.raises(ValueError, match="\\[L\\] or \\[B, L\\]"):
        INF.trim(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="2\\^27"):
        INF.trim(torch.zeros(2, 0))
    with pytest.raises(ValueError, match="2\\^27"):
        INF.trim(torch.zeros(1, 1).expand(1, (1 << 27) + 1))
    with pytest.raises(ValueError, match="2\\^27"):
        INF.trim_list([torch.zeros(1).expand((1 << 27) + 1)])
    with pytest.raises(ValueError, match="2 lengths for a batch of 3"):
        INF.trim(x, lengths=[5000, 10])
    with pytest.raises(ValueError, match="exceeds"):
        INF.trim(x, lengths=[5001, 10, 10])
    with pytest.raises(ValueError, match="positive"):
        INF.trim(x, lengths=[5000, 0, 10])
    with pytest.raises(ValueError, match="max_batch"):
        INF.trim_list([x[0]], max_batch=0)
    with pytest.raises(ValueError, match="1-D"):
        INF.trim_list([x])
    with pytest.raises(ValueError, match="non-empty"):
        INF.trim_list([x[0], x[0][:0]])
    # all value guards passed: the CPU tensors are refused before any launch
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        INF.trim(x, lengths=[5000, 1500, 1])
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        INF.trim(x[0], top_db=45, power=True)
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        INF.trim_list([x[0], x[1]], max_batch=1)
    assert INF._trim_batches([5, 9, 9, 1, 7], 2) == [[1, 2], [4, 0], [3]] and INF._trim_batches([], 3) == []
    assert INF.trim_list([]) == ([], []) and INF.trim_bounds_list([]) == []
