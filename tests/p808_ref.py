"""Float64 definition of the P808_MOS column of DNSMOS as the device computes it (csrc/p808.hip, dnsmos.py P808), written without the
product code: numpy (and scipy's window) only.

Sources: the script ``DNSMOS/dnsmos_local.py:27-31, 77-80, 99`` (``audio_melspec`` of ``audio_seg[:-160]``, the mean of the
segments), librosa 0.10.2 (``environment.yml`` pins ``librosa==0.10.2.post1``): ``feature.melspectrogram`` -> ``core.spectrum.stft`` /
``_spectrogram`` / ``filters.mel``, ``core.spectrum.power_to_db``, and the graph of ``DNSMOS/DNSMOS/model_v8.onnx`` (25 nodes).
``t`` is a dict of the initializers under the names of ``dnsmos.P808_SHAPES`` (conv0_w .. conv4_b, dense0_w .. dense2_b).
"""
import numpy as np
import scipy.signal

import dnsmos_ref as R

SR, N_FFT, HOP, N_MELS = 16000, 321, 160, 120
A = 144000                    # len(audio_seg[:-160])
T = 900
POOLED = (True, True, False, True, False)      # a MaxPool node follows conv2d_5, conv2d_6 and conv2d_8


# ---- librosa.filters.mel
def hz_to_mel(f):
    """convert.hz_to_mel, htk=False, of a scalar: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)."""
    f_sp = 200.0 / 3
    if f >= 1000.0:
        return 1000.0 / f_sp + np.log(f / 1000.0) / (np.log(6.4) / 27.0)
    return f / f_sp


def mel_to_hz(m):
    """convert.mel_to_hz, htk=False, of an array."""
    f_sp = 200.0 / 3
    min_log_mel = 1000.0 / f_sp
    high = m >= min_log_mel
    return np.where(high, 1000.0 * np.exp((np.log(6.4) / 27.0) * (np.where(high, m, min_log_mel) - min_log_mel)), f_sp * m)


def mel_basis():
    """filters.mel(sr=16000, n_fft=321, n_mels=120): fmin 0, fmax 8000, Slaney scale and norm, dtype float32 -> float32 [120, 161].
    The triangle min(lower, upper) clipped at 0 is rounded to float32 when it is stored; ``weights *= enorm[:, None]`` multiplies
    that float32 by the float64 enorm in double and rounds to float32 again."""
    freqs = np.fft.rfftfreq(n=N_FFT, d=1.0 / SR)
    mels = np.linspace(hz_to_mel(0.0), hz_to_mel(SR / 2.0), N_MELS + 2)
    mel_f = mel_to_hz(mels)
    out = np.zeros((N_MELS, len(freqs)), dtype=np.float32)
    for i in range(N_MELS):
        lower = (freqs - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - freqs) / (mel_f[i + 2] - mel_f[i + 1])
        tri = np.maximum(0, np.minimum(lower, upper)).astype(np.float32)
        out[i] = (tri.astype(np.float64) * (2.0 / (mel_f[i + 2] - mel_f[i]))).astype(np.float32)
    return out


def window():
    return scipy.signal.get_window("hann", N_FFT, fftbins=True)


# ---- librosa.stft, center=True, pad_mode="constant"
def frames(a):
    """[900, 321]: frame t is samples 160 t - 160 .. 160 t + 160 of a, zero outside [0, 144000)."""
    a = np.asarray(a)
    assert a.shape == (A,)
    y = np.concatenate([np.zeros(N_FFT // 2, a.dtype), a, np.zeros(N_FFT // 2, a.dtype)])
    n = 1 + (len(y) - N_FFT) // HOP
    return np.stack([y[HOP * t:HOP * t + N_FFT] for t in range(n)])


def power_rfft(a):
    """abs(stft) ** 2 -> [161 bins, 900 frames], float64."""
    fr = frames(np.asarray(a, dtype=np.float64)) * window()
    return (np.abs(np.fft.rfft(fr, n=N_FFT, axis=1)) ** 2).T


def dft_tables(win=None):
    """cos(2 pi k n / 321) w[n] and -sin(2 pi k n / 321) w[n], [161, 321] each, the angle of k n mod 321."""
    w = window() if win is None else win
    kn = np.outer(np.arange(N_FFT // 2 + 1), np.arange(N_FFT)) % N_FFT
    ang = 2.0 * np.pi * kn / N_FFT
    return np.cos(ang) * w, -np.sin(ang) * w


def power_table(a, tables=None):
    """The same power as a product with the windowed DFT tables: re re + im im -> [161, 900]."""
    c, s = dft_tables() if tables is None else tables
    fr = frames(np.asarray(a, dtype=np.float64))
    re, im = fr @ c.T, fr @ s.T
    return (re * re + im * im).T


def mel_power(a, power=power_rfft, basis=None):
    """melspectrogram(y=a, sr=16000, n_fft=321, hop_length=160, n_mels=120) -> [120, 900] float64."""
    b = mel_basis() if basis is None else basis
    return b.astype(np.float64) @ power(a)


def power_to_db(M):
    """power_to_db(M, ref=np.max, amin=1e-10, top_db=80.0)."""
    ls = 10.0 * np.log10(np.maximum(1e-10, M))
    ls -= 10.0 * np.log10(np.maximum(1e-10, np.max(M)))
    return np.maximum(ls, ls.max() - 80.0)


def feature64(seg, power=power_rfft):
    """((power_to_db(mel) + 40) / 40).T of seg[:-160] -> [900, 120] float64; the script rounds it to float32."""
    seg = np.asarray(seg)
    assert seg.shape == (R.SEG,)
    return ((power_to_db(mel_power(seg[:-160], power)) + 40) / 40).T


def feature(seg):
    return feature64(seg).astype(np.float32)


# ---- model_v8.onnx
def network_from_feature(f, t):
    """Unsqueeze / Transpose to one channel, conv2d_5 .. conv2d_9 with the three MaxPool nodes, ReduceMax over the map, dense_3 .. 5."""
    x = np.asarray(f, dtype=np.float64)[:, :, None]
    for k in range(5):
        x = R.conv3x3(x, t[f"conv{k}_w"], t[f"conv{k}_b"])
        if POOLED[k]:
            x = R.pool2x2(x)
    g = x.max(axis=(0, 1))
    h = R.dense(g, t["dense0_w"], t["dense0_b"], True)
    h = R.dense(h, t["dense1_w"], t["dense1_b"], True)
    return float(R.dense(h, t["dense2_w"], t["dense2_b"], False)[0])


def network(seg, t):
    """The float64 definition: the float32 feature (the graph's input type) through the float64 network."""
    return network_from_feature(feature(seg), t)


def network_float32(seg, t):
    """The float64 feature rounded to float32, then the network in float32 by torch on the CPU."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        x = torch.from_numpy(feature(seg))[None, None]
        for k in range(5):
            x = F.relu(F.conv2d(x, torch.from_numpy(t[f"conv{k}_w"]), torch.from_numpy(t[f"conv{k}_b"]), padding=1))
            if POOLED[k]:
                x = F.max_pool2d(x, 2)
        g = x.amax(dim=(2, 3))[0]
        h = F.relu(g @ torch.from_numpy(t["dense0_w"]) + torch.from_numpy(t["dense0_b"]))
        h = F.relu(h @ torch.from_numpy(t["dense1_w"]) + torch.from_numpy(t["dense1_b"]))
        return float((h @ torch.from_numpy(t["dense2_w"]) + torch.from_numpy(t["dense2_b"]))[0])


def score_clip(audio, t, raw_fn=network):
    """(P808_MOS of the clip, the per-segment values [S]): the mean over the segments the script's loop evaluates, as a double sum in
    segment order.  (The script's np.mean of a list of float32 values is a float32 mean; the library keeps the double.)"""
    segs, _, _ = R.script_segments(np.asarray(audio))
    raw = np.array([np.float64(raw_fn(np.asarray(s, dtype=np.float32), t)) for s in segs])
    return raw.mean(), raw
