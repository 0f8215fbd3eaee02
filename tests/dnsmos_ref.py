"""Float64 definition of DNSMOS P.835 (SIG / BAK / OVRL) as the device computes it (csrc/dnsmos.hip, dnsmos.py), written without the
product code: numpy only, the convolution as nine shifted sums.

Sources: the graph of the reference's ``DNSMOS/DNSMOS/sig_bak_ovr.onnx`` (its 48 nodes in file order, cited by node name below) and the
script ``DNSMOS/dnsmos_local.py:49-100``.  ``t`` is a dict of the initializers under the names of ``dnsmos.SHAPES`` (fe_re, fe_im,
log_floor, log_div, pow, conv0_w .. conv6_b, dense0_w .. dense2_b).
"""
import numpy as np

FS = 16000                    # dnsmos_local.py:19 SAMPLING_RATE
INPUT_LENGTH = 9.01           # dnsmos_local.py:20
SEG = 144160
POOLED = (False, False, False, True, True, True, False)      # a MaxPool node follows conv2d_3, conv2d_4, conv2d_5


# ---- the graph
def frames(seg):
    """Slice input_1:01_cropping (samples 0 .. 143999) and input_1:01_cropping_1 (160 .. 144159), Reshape to [900, 160] each, Concat on
    the last axis: frame t = samples 160 t .. 160 t + 319."""
    seg = np.asarray(seg)
    assert seg.shape == (SEG,)
    return np.concatenate([seg[:144000].reshape(900, 160), seg[160:].reshape(900, 160)], axis=1)


def feature(seg, t, dtype=np.float64):
    """Conv stft-real / stft-imag (kernel size 1 over the 320 'channels' = a matrix product), Mul x2 (squares), Add, Sqrt, Pow (y = 2),
    Max (x = 1e-12), Log, Div (y = 2.3025851) -> [900, 161]."""
    fr = frames(seg).astype(dtype)
    re = fr @ t["fe_re"].astype(dtype).T
    im = fr @ t["fe_im"].astype(dtype).T
    mag = np.sqrt(re * re + im * im)
    p = mag ** dtype(t["pow"])
    return np.log(np.maximum(dtype(t["log_floor"]), p)) / dtype(t["log_div"])


def conv3x3(x, w, b):
    """Conv (kernel 3x3, pads 1, strides 1) + Relu on one image: x [H, W, Cin], w [Cout, Cin, 3, 3], b [Cout] -> [H, W, Cout].  Nine shifted
    sums over the zero-padded image, tap (ky, kx) reading input (y + ky - 1, x + kx - 1): cross-correlation, as ONNX Conv."""
    H, W, Cin = x.shape
    xp = np.zeros((H + 2, W + 2, Cin), dtype=x.dtype)
    xp[1:H + 1, 1:W + 1] = x
    out = np.zeros((H, W, w.shape[0]), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += xp[ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].astype(x.dtype).T
    return np.maximum(out + b.astype(x.dtype), 0)


def pool2x2(x):
    """MaxPool (kernel 2x2, strides 2, VALID, ceil_mode 0): [H, W, C] -> [H // 2, W // 2, C]; an odd last row / column is dropped."""
    H, W, C = x.shape
    v = x[:H // 2 * 2, :W // 2 * 2].reshape(H // 2, 2, W // 2, 2, C)
    return v.max(axis=(1, 3))


def dense(v, w, b, relu):
    """MatMul (weights [in, out]) + Add (+ Relu)."""
    y = v @ w.astype(v.dtype) + b.astype(v.dtype)
    return np.maximum(y, 0) if relu else y


def network_from_feature(f, t):
    """Unsqueeze / Transpose to one channel, conv2d .. conv2d_6 with the three MaxPool nodes, ReduceMax over the map, the dense layers
    -> (SIG_raw, BAK_raw, OVRL_raw) (the order of Identity:0 as dnsmos_local.py:81 unpacks it)."""
    x = f[:, :, None]
    for k in range(7):
        x = conv3x3(x, t[f"conv{k}_w"], t[f"conv{k}_b"])
        if POOLED[k]:
            x = pool2x2(x)
    g = x.max(axis=(0, 1))
    h = dense(g, t["dense0_w"], t["dense0_b"], True)
    h = dense(h, t["dense1_w"], t["dense1_b"], True)
    return dense(h, t["dense2_w"], t["dense2_b"], False)


def network(seg, t):
    return network_from_feature(feature(seg, t), t)


def network_float32(seg, t):
    """The same network evaluated in float32 by torch on the CPU (its conv2d / max_pool2d / matmul): the yardstick for what float32
    arithmetic costs on this network."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        fr = torch.from_numpy(frames(np.asarray(seg, dtype=np.float32)))
        re = fr @ torch.from_numpy(t["fe_re"]).T
        im = fr @ torch.from_numpy(t["fe_im"]).T
        p = torch.sqrt(re * re + im * im) ** float(t["pow"])
        f = torch.log(torch.maximum(torch.tensor(np.float32(t["log_floor"])), p)) / torch.tensor(np.float32(t["log_div"]))
        x = f[None, None]
        for k in range(7):
            x = F.relu(F.conv2d(x, torch.from_numpy(t[f"conv{k}_w"]), torch.from_numpy(t[f"conv{k}_b"]), padding=1))
            if POOLED[k]:
                x = F.max_pool2d(x, 2)
        g = x.amax(dim=(2, 3))[0]
        h = F.relu(g @ torch.from_numpy(t["dense0_w"]) + torch.from_numpy(t["dense0_b"]))
        h = F.relu(h @ torch.from_numpy(t["dense1_w"]) + torch.from_numpy(t["dense1_b"]))
        return (h @ torch.from_numpy(t["dense2_w"]) + torch.from_numpy(t["dense2_b"])).numpy()


# ---- the script
def polyfit(sig, bak, ovr, personalized):
    """dnsmos_local.py:33-47 get_polyfit_val."""
    if personalized:
        p_ovr = np.poly1d([-0.00533021, 0.005101, 1.18058466, -0.11236046])
        p_sig = np.poly1d([-0.01019296, 0.02751166, 1.19576786, -0.24348726])
        p_bak = np.poly1d([-0.04976499, 0.44276479, -0.1644611, 0.96883132])
    else:
        p_ovr = np.poly1d([-0.06766283, 1.11546468, 0.04602535])
        p_sig = np.poly1d([-0.08397278, 1.22083953, 0.0052439])
        p_bak = np.poly1d([-0.13166888, 1.60915514, -0.39604546])
    return p_sig(sig), p_bak(bak), p_ovr(ovr)


def script_segments(audio, fs=FS):
    """dnsmos_local.py:56-76 on an array: tile by appending the clip to itself, num_hops, the slices of the loop ->
    (segments, num_hops, number of times the ``len(audio_seg) < len_samples`` guard of :73 fired)."""
    len_samples = int(INPUT_LENGTH * fs)
    while len(audio) < len_samples:
        audio = np.append(audio, audio)
    num_hops = int(np.floor(len(audio) / fs) - INPUT_LENGTH) + 1
    hop_len_samples = fs
    segs, fired = [], 0
    for idx in range(num_hops):
        audio_seg = audio[int(idx * hop_len_samples): int((idx + INPUT_LENGTH) * hop_len_samples)]
        if len(audio_seg) < len_samples:
            fired += 1
            continue
        segs.append(audio_seg)
    return segs, num_hops, fired


def score_clip(audio, t, personalized=False, raw_fn=network):
    """dnsmos_local.py:49-100 without the file, the resampler and P808_MOS -> (dict of the clip's seven values, raw [S, 3]).  The device
    rounds a segment's raw values to float32 (the network's output type) before the polynomials; the means are double sums in segment
    order.  (The script's np.mean of a list of float32 raw values is a float32 mean; the library keeps the double.)"""
    segs, num_hops, _ = script_segments(np.asarray(audio))
    raw = np.stack([np.asarray(raw_fn(np.asarray(s, dtype=np.float32), t), dtype=np.float64) for s in segs])
    sig, bak, ovr = polyfit(raw[:, 0], raw[:, 1], raw[:, 2], personalized)
    out = {"num_hops": num_hops, "SIG_raw": raw[:, 0].mean(), "BAK_raw": raw[:, 1].mean(), "OVRL_raw": raw[:, 2].mean(),
           "SIG": sig.mean(), "BAK": bak.mean(), "OVRL": ovr.mean()}
    return out, raw


# ---- deterministic test signals (no digital silence)
def _tri(k, period):
    """Triangle wave of an integer period in [-1, 1]: integer arithmetic and one exactly rounded division, the same on every machine."""
    ph = (k * 2) % (2 * period)
    return (np.abs(ph - period) * 2 - period) / float(period)


def signal(kind, n, seed=0):
    """Test signals from integers and exactly rounded + - * / only (no libm call), so every machine builds the same float32 samples."""
    k = np.arange(n, dtype=np.int64)
    white = np.random.default_rng(1000 + seed).integers(-32768, 32768, n).astype(np.float64) / 32768.0
    if kind == "noise":
        x = 0.1 * white
    elif kind == "tone":
        x = 0.3 * _tri(k, 36) * (0.6 + 0.4 * _tri(k, 5333)) + 0.003 * white
    elif kind == "speechlike":
        x = sum(_tri(k * h, 133) / h for h in range(1, 9)) * 0.08 * (0.5 + 0.5 * _tri(k, 6400)) ** 2 + 0.01 * white
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def load_weights(*paths):
    t = {}
    for path in paths:
        with np.load(path) as z:
            t.update({k: z[k] for k in z.files})
    return t
