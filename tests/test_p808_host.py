"""Host side of the P808_MOS column (no GPU): the float64 definition tests/p808_ref.py against itself in another form, against the
host-made tables of dnsmos.P808 and, where they are installed, against librosa and onnxruntime; the acceptance of model_v8.onnx."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dnsmos_ref as R  # noqa: E402
import p808_ref as P  # noqa: E402
from test_dnsmos_host import REFERENCE, _model, _tensor  # noqa: E402  (the reference checkout, the writer of small ONNX files)

GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL = os.path.join(REFERENCE, "DNSMOS", "DNSMOS", "model_v8.onnx")


def _mod():
    return importlib.import_module("i-dccrn-vae_amd.dnsmos")


def _weights():
    return R.load_weights(os.path.join(GOLDEN, "p808_weights.npz"))


# ------------------------------------------------------------------------------------------------------------ 1. the tables
def test_host_tables_equal_the_definition():
    """The window, the float32 mel basis and the windowed DFT table dnsmos.P808 makes are the definition's bit for bit."""
    D = _mod()
    np.testing.assert_array_equal(D.p808_window(), P.window())
    basis = D.p808_mel_basis()
    assert basis.dtype == np.float32 and basis.shape == (120, 161)
    np.testing.assert_array_equal(basis, P.mel_basis())
    tab = D.p808_dft_table()
    c, s = P.dft_tables()
    assert tab.dtype == np.float64 and tab.shape == (2, 161, 324)
    np.testing.assert_array_equal(tab[0, :, :321], c)
    np.testing.assert_array_equal(tab[1, :, :321], s)
    assert not tab[:, :, 321:].any()
    m = D.P808(_weights())
    np.testing.assert_array_equal(m.mel, basis.astype(np.float64))
    np.testing.assert_array_equal(m.dft, tab)


def test_frame_count_filters_and_silence():
    """900 frames of 321 samples (not 901), frame t = samples 160 t - 160 .. 160 t + 160 with zeros outside; no mel
    filter is empty (1 - 8 non-zero bins); an all-zero segment maps to exactly 1.0 everywhere."""
    a = np.arange(1, P.A + 1)
    fr = P.frames(a)
    assert fr.shape == (900, 321)
    assert (fr[0, :160] == 0).all() and fr[0, 160] == 1 and fr[0, 320] == 161
    np.testing.assert_array_equal(fr[457], np.arange(160 * 457 - 160, 160 * 457 + 161) + 1)
    assert fr[899, 160] == 160 * 899 + 1 and fr[899, 319] == P.A and fr[899, 320] == 0
    nz = (P.mel_basis() > 0).sum(axis=1)
    assert nz.min() == 1 and nz.max() == 8
    f = P.feature64(np.zeros(R.SEG, dtype=np.float32))
    assert f.shape == (900, 120) and (f == 1.0).all()


def test_rfft_form_equals_table_form():
    """abs(rfft) ** 2 against re re + im im of the table product: 1e-12 of the map's maximum (two float64 DFTs of 321 points), and
    the features within 1e-11 (the decibels of the bins 80 dB below the maximum amplify the relative error)."""
    x = R.signal("speechlike", R.SEG, 2)
    a, b = P.power_rfft(x[:-160]), P.power_table(x[:-160])
    assert a.shape == b.shape == (161, 900)
    assert np.abs(a - b).max() <= 1e-12 * a.max()
    fa, fb = P.feature64(x), P.feature64(x, P.power_table)
    assert np.abs(fa - fb).max() <= 1e-11
    assert fa.max() == 1.0 and fa.min() >= -1.0


def test_sample_144000_is_not_part_of_the_feature():
    x = R.signal("tone", R.SEG, 5)
    y = x.copy()
    y[144000:] = 100.0
    np.testing.assert_array_equal(P.feature(x), P.feature(y))
    y[143999] = 100.0
    assert not np.array_equal(P.feature(x), P.feature(y))


def test_definition_reproduces_its_fixture():
    """The float64 definition on the one-segment fixture signal equals tests/golden/p808_expected.npz (1e-9: far above what another
    BLAS / FFT does to a float64 evaluation, far below the float32 floor of 2e-7)."""
    exp = np.load(os.path.join(GOLDEN, "p808_expected.npz"))
    clip, raw = P.score_clip(R.signal("tone", 144160), _weights())
    assert raw.shape == (1,)
    np.testing.assert_allclose(raw, exp["tone.raw64"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(clip, exp["tone.clip64"], rtol=0, atol=1e-9)
    assert np.abs(exp["tone.raw32"] - exp["tone.raw64"]).max() < 1e-6


# ------------------------------------------------------------------------------------------------------------ 2. the file
def _fake_file(D, t, op_types, names=None):
    names = names or D.P808_ONNX_NAMES
    return _model(op_types, [_tensor(name, t[k].reshape(shape), "raw" if t[k].ndim <= 2 else "typed") for k, (name, shape) in names.items()])


def test_from_onnx_accepts_the_graph_and_rejects_others(tmp_path):
    D = _mod()
    t = _weights()
    good = tmp_path / "good.onnx"
    good.write_bytes(_fake_file(D, t, D.P808_OP_SEQUENCE))
    m = D.P808.from_onnx(str(good))
    assert sorted(m.tensors) == sorted(D.P808_SHAPES) and len(D.P808_SHAPES) == 16
    for k in D.P808_SHAPES:
        np.testing.assert_array_equal(m.tensors[k], t[k])
    other = list(D.P808_OP_SEQUENCE)
    other[4] = "AveragePool"
    for name, ops_ in (("pool", other), ("short", D.P808_OP_SEQUENCE[:-1]), ("sig_bak_ovr", D.OP_SEQUENCE)):
        bad = tmp_path / f"{name}.onnx"
        bad.write_bytes(_fake_file(D, t, ops_))
        with pytest.raises(ValueError, match="not the DNSMOS P.808"):
            D.P808.from_onnx(str(bad))
    # the tensors of sig_bak_ovr.onnx behind the right op sequence: conv2d_5 / dense_3 are not among its names
    t835 = R.load_weights(os.path.join(GOLDEN, "dnsmos_weights.npz"), os.path.join(GOLDEN, "dnsmos_frontend.npz"))
    bad = tmp_path / "names.onnx"
    bad.write_bytes(_fake_file(D, t835, D.P808_OP_SEQUENCE, D.ONNX_NAMES))
    with pytest.raises(ValueError, match="conv2d_5/kernel:0"):
        D.P808.from_onnx(str(bad))
    t2 = dict(t)
    t2["dense2_w"] = np.zeros((64, 3), dtype=np.float32)
    bad = tmp_path / "shape.onnx"
    bad.write_bytes(_model(D.P808_OP_SEQUENCE, [_tensor(name, t2[k], "raw") for k, (name, _) in D.P808_ONNX_NAMES.items()]))
    with pytest.raises(ValueError, match="dense_5/MatMul"):
        D.P808.from_onnx(str(bad))
    # and the other way round: the P.835 class refuses this file
    with pytest.raises(ValueError, match="not the DNSMOS"):
        D.DNSMOS.from_onnx(str(good))


def test_from_npz_and_guards():
    D = _mod()
    m = D.P808.from_npz(os.path.join(GOLDEN, "p808_weights.npz"))
    assert m.workspace_segments == 32 and m.tensors["conv4_w"].shape == (64, 32, 3, 3)
    with pytest.raises(ValueError, match="conv0_w"):
        D.P808.from_npz(os.path.join(GOLDEN, "dnsmos_frontend.npz"))
    with pytest.raises(ValueError):
        D.P808(m.tensors, workspace_segments=0)
    with pytest.raises(ValueError):
        D.P808(m.tensors, mel=np.zeros((120, 160)))
    with pytest.raises(ValueError):
        D.P808(m.tensors, dft=np.ones((2, 161, 324)))


def test_from_onnx_equals_the_committed_weights():
    if not os.path.exists(MODEL):
        pytest.skip("no checkout of the reference here")
    m = _mod().P808.from_onnx(MODEL)
    t = _weights()
    assert sorted(t) == sorted(m.tensors)
    for k, v in t.items():
        assert v.dtype == m.tensors[k].dtype and v.tobytes() == m.tensors[k].tobytes(), k


# ----------------------------------------------------------------------------------------------- 3. librosa and onnxruntime
def test_feature_equals_librosa():
    """Parity with librosa is unpinned where it is not installed."""
    librosa = pytest.importorskip("librosa")
    x = R.signal("speechlike", R.SEG, 1)
    a = x[:-160].astype(np.float64)
    np.testing.assert_array_equal(P.mel_basis(), librosa.filters.mel(sr=16000, n_fft=321, n_mels=120))
    mel = librosa.feature.melspectrogram(y=a, sr=16000, n_fft=321, hop_length=160, n_mels=120)
    want = ((librosa.power_to_db(mel, ref=np.max) + 40) / 40).T
    assert want.shape == (900, 120)
    np.testing.assert_allclose(P.feature64(x), want, rtol=0, atol=1e-9)


def test_definition_equals_onnxruntime():
    """Parity with onnxruntime is unpinned where it is not installed."""
    ort = pytest.importorskip("onnxruntime")
    if not os.path.exists(MODEL):
        pytest.skip("no checkout of the reference here")
    x = R.signal("tone", 144160)
    got = ort.InferenceSession(MODEL).run(None, {"input_1": P.feature(x)[None]})[0][0][0]
    np.testing.assert_allclose(got, P.network(x, _weights()), rtol=0, atol=2e-5)
