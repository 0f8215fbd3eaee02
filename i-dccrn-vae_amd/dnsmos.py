"""DNSMOS P.835 on the device: SIG / BAK / OVRL of recordings without a clean reference (csrc/dnsmos.hip).

The definition is the reference's ``DNSMOS/dnsmos_local.py:49-100`` around the network of ``sig_bak_ovr.onnx`` (the personalized
model: another file with the same graph, and other polynomials), restated in float64 in ``tests/dnsmos_ref.py``.  Parity with
onnxruntime itself is unpinned (it is not installed where this library is tested).  The script's fourth column, ``P808_MOS``
(``model_v8.onnx`` on a librosa mel spectrogram), is NOT provided.

The network reads 9.01 s = 144160 samples at 16 kHz:

* frames: frame t (900 of them) is samples 160 t .. 160 t + 319;
* front end: two learned [161, 320] matrices give re and im; feature = ln(max(floor, (sqrt(re^2 + im^2))^2)) / div with the file's
  constants (1e-12, 2.3025851), viewed as a [900 (time), 161 (bin)] map of one channel;
* seven 3x3 convolutions (stride 1, zero pad 1, bias, ReLU), channels 1 -> 128 -> 64 -> 64 -> 32, 2x2 max-pool, 32 -> 32, pool,
  32 -> 32, pool, 32 -> 64; global max over the map; dense 64 -> 128 ReLU, 128 -> 64 ReLU, 64 -> 3 = (SIG_raw, BAK_raw, OVRL_raw).

Everything from the padded batch to the per-clip means runs in HIP kernels; there is no fallback.
"""
from __future__ import annotations

import math
import struct
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import call, f, i, ll, p, stream_ptr

FS = 16000
SEG_SAMPLES = 144160                 # int(9.01 * 16000) of the script; the graph's input width
FRAMES, BINS, WIN, HOP = 900, 161, 320, 160
INPUT_LENGTH = 9.01
MAX_LEN = 2 ** 27                    # samples per row, as for the other row kernels

# (in, out, pooled) of the seven convolutions
CONVS = ((1, 128, False), (128, 64, False), (64, 64, False), (64, 32, True), (32, 32, True), (32, 32, True), (32, 64, False))
DENSE = ((64, 128), (128, 64), (64, 3))

# np.poly1d coefficients (highest power first) of get_polyfit_val, in the network's output order SIG, BAK, OVRL
POLY = {
    False: ((-0.08397278, 1.22083953, 0.0052439), (-0.13166888, 1.60915514, -0.39604546), (-0.06766283, 1.11546468, 0.04602535)),
    True: ((-0.01019296, 0.02751166, 1.19576786, -0.24348726), (-0.04976499, 0.44276479, -0.1644611, 0.96883132),
           (-0.00533021, 0.005101, 1.18058466, -0.11236046)),
}

# the graph of sig_bak_ovr.onnx: its nodes' op types in file order
OP_SEQUENCE = (
    "Slice", "Slice", "Reshape", "Reshape", "Concat", "Transpose", "Transpose", "Conv", "Conv", "Transpose", "Transpose", "Mul", "Mul",
    "Add", "Sqrt", "Pow", "Max", "Log", "Div", "Unsqueeze", "Transpose",
    "Conv", "Relu", "Conv", "Relu", "Conv", "Relu", "Conv", "Relu", "MaxPool", "Conv", "Relu", "MaxPool", "Conv", "Relu", "MaxPool", "Conv",
    "Relu", "Transpose", "ReduceMax", "MatMul", "Add", "Relu", "MatMul", "Add", "Relu", "MatMul", "Add")

_DENSE_NAME = "mos_estimator_logpow/dense{}/{}/ReadVariableOp/resource:0"
# name here -> (initializer name in the file, shape in the file)
ONNX_NAMES: Dict[str, Tuple[str, Tuple[int, ...]]] = {
    "fe_re": ("time2freq/stft-real/kernel:0", (BINS, WIN, 1)),
    "fe_im": ("time2freq/stft-imag/kernel:0", (BINS, WIN, 1)),
    "log_floor": ("mos_estimator_logpow/Maximum/x:0", ()),
    "log_div": ("mos_estimator_logpow/truediv/y:0", ()),
    "pow": ("mos_estimator_logpow/pow/y:0", ()),
}
for _k, (_ci, _co, _) in enumerate(CONVS):
    _n = "conv2d" if _k == 0 else f"conv2d_{_k}"
    ONNX_NAMES[f"conv{_k}_w"] = (f"{_n}/kernel:0", (_co, _ci, 3, 3))
    ONNX_NAMES[f"conv{_k}_b"] = (f"{_n}/bias:0", (_co,))
for _k, ((_ci, _co), _sfx) in enumerate(zip(DENSE, ("", "_1", "_3"))):
    ONNX_NAMES[f"dense{_k}_w"] = (_DENSE_NAME.format(_sfx, "MatMul"), (_ci, _co))
    ONNX_NAMES[f"dense{_k}_b"] = (_DENSE_NAME.format(_sfx, "BiasAdd"), (_co,))

# shapes as this module keeps them (the front-end matrices without their trailing 1)
SHAPES = {k: (shape[:2] if k.startswith("fe_") else shape) for k, (_, shape) in ONNX_NAMES.items()}


# ------------------------------------------------------------------------------------------------ ONNX protobuf wire format
def _varint(b, pos: int) -> Tuple[int, int]:
    v = shift = 0
    while True:
        if pos >= len(b):
            raise ValueError("truncated varint")
        c = b[pos]
        pos += 1
        v |= (c & 0x7F) << shift
        shift += 7
        if c < 0x80:
            return v, pos
        if shift > 70:
            raise ValueError("varint longer than 10 bytes")


def _fields(b):
    """(field number, wire type, value) of every field of one protobuf message; value: an int (varint), or a memoryview."""
    pos, n = 0, len(b)
    while pos < n:
        key, pos = _varint(b, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(b, pos)
        elif wt in (1, 5):
            w = 8 if wt == 1 else 4
            v, pos = b[pos:pos + w], pos + w
        elif wt == 2:
            ln, pos = _varint(b, pos)
            v, pos = b[pos:pos + ln], pos + ln
        else:
            raise ValueError(f"wire type {wt} is not used by ONNX")
        if pos > n:
            raise ValueError("truncated field")
        yield num, wt, v


_DTYPES = {1: "<f4", 6: "<i4", 7: "<i8", 11: "<f8"}     # TensorProto.DataType
_TYPED_FIELD = {1: 4, 6: 5, 7: 7, 11: 10}               # float_data, int32_data, int64_data, double_data


def _tensor(b) -> Tuple[str, np.ndarray]:
    """A TensorProto: dims = 1, data_type = 2, float_data = 4, int32_data = 5, int64_data = 7, name = 8, raw_data = 9, double_data = 10."""
    dims: List[int] = []
    name, dtype, raw = "", None, None
    typed: Dict[int, list] = {}
    for num, wt, v in _fields(b):
        if num == 1:
            if wt == 0:
                dims.append(v)
            else:
                pos = 0
                while pos < len(v):
                    x, pos = _varint(v, pos)
                    dims.append(x)
        elif num == 2:
            dtype = v
        elif num == 8:
            name = bytes(v).decode()
        elif num == 9:
            raw = bytes(v)
        elif num in (4, 5, 7, 10):
            typed.setdefault(num, []).append((wt, v))
    if dtype not in _DTYPES:
        raise ValueError(f"initializer {name!r}: data type {dtype} is not supported")
    dt = np.dtype(_DTYPES[dtype])
    if raw is not None:
        a = np.frombuffer(raw, dtype=dt)
    else:
        vals: list = []
        for wt, v in typed.get(_TYPED_FIELD[dtype], []):
            if dt.kind == "f":
                vals.extend(np.frombuffer(bytes(v), dtype=dt).tolist() if wt == 2 else [struct.unpack("<f" if wt == 5 else "<d", bytes(v))[0]])
            elif wt == 0:
                vals.append(v)
            else:
                pos = 0
                while pos < len(v):
                    x, pos = _varint(v, pos)
                    vals.append(x)
        if dt.kind == "i":
            vals = [x - (1 << 64) if x >= (1 << 63) else x for x in vals]      # two's-complement varints
        a = np.asarray(vals, dtype=dt)
    n = int(np.prod(dims)) if dims else 1
    if a.size != n:
        raise ValueError(f"initializer {name!r}: {a.size} values for dims {dims}")
    return name, a.reshape(dims).copy()


def read_onnx(path: str) -> Tuple[List[str], Dict[str, np.ndarray]]:
    """The node op types in file order and the initializers by name of an ONNX file: ModelProto.graph = 7; GraphProto.node = 1,
    .initializer = 5; NodeProto.op_type = 4.  Nothing else of the file is interpreted."""
    with open(path, "rb") as fh:
        data = memoryview(fh.read())
    graph = None
    for num, wt, v in _fields(data):
        if num == 7 and wt == 2:
            graph = v
    if graph is None:
        raise ValueError(f"{path}: no graph")
    ops_: List[str] = []
    inits: Dict[str, np.ndarray] = {}
    for num, wt, v in _fields(graph):
        if num == 1 and wt == 2:
            ops_.append(next((bytes(u).decode() for g, w2, u in _fields(v) if g == 4 and w2 == 2), ""))
        elif num == 5 and wt == 2:
            name, a = _tensor(v)
            inits[name] = a
    return ops_, inits


# --------------------------------------------------------------------------------------------------------------- host planner
def num_hops(length: int) -> Tuple[int, int]:
    """(tiled length, num_hops) of a clip of ``length`` samples at 16 kHz, as dnsmos_local.py:56-61: the clip is appended to itself
    while it is shorter than 144160 samples, then ``int(floor(len / 16000) - 9.01) + 1``."""
    n = int(length)
    if n < 1:
        raise ValueError(f"a clip of {length} samples cannot be scored")
    while n < SEG_SAMPLES:
        n *= 2
    return n, int(math.floor(n / FS) - INPUT_LENGTH) + 1


def hop_is_scored(idx: int) -> bool:
    """Whether the script's loop evaluates hop ``idx``: its slice ends at ``int((idx + 9.01) * 16000)``, which in double arithmetic is
    one sample short of 144160 for idx = 7 .. 23, 119 .. 122, ...; the ``len(audio_seg) < len_samples`` guard of dnsmos_local.py:73
    then skips the hop, and the clip's means are taken over the others."""
    return int((idx + INPUT_LENGTH) * FS) - idx * FS >= SEG_SAMPLES


def plan_segments(lengths: Sequence[int]) -> Tuple[List[Tuple[int, int]], List[int]]:
    """Host planner -> ``(segments, counts)``: ``segments`` the ``(row, start)`` of every 144160-sample segment the script's loop
    evaluates, clip by clip in row order, hop idx of a clip starting at ``16000 * idx`` of its tiled signal (sample j of which is
    ``x[j mod length]``); ``counts[b]`` the number of segments of clip b: its :func:`num_hops` less the hops the script skips
    (:func:`hop_is_scored`; hop 0 is never skipped).  Raises for a length < 1."""
    segs: List[Tuple[int, int]] = []
    counts: List[int] = []
    for b, n in enumerate(lengths):
        if isinstance(n, bool) or int(n) != n or n < 1:
            raise ValueError(f"lengths[{b}] = {n!r}: a clip needs at least one sample")
        _, hops = num_hops(int(n))
        mine = [(b, FS * idx) for idx in range(hops) if hop_is_scored(idx)]
        counts.append(len(mine))
        segs.extend(mine)
    return segs, counts


# ------------------------------------------------------------------------------------------------------------------ the model
class _Packs:
    """The device-side form of one model on one device: the weights in the order the kernels stream them, made once."""

    def __init__(self, t: Dict[str, np.ndarray], personalized: bool, device):
        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        st = stream_ptr()
        re, im = dev(t["fe_re"]), dev(t["fe_im"])
        self.fe = torch.empty(int(ops.L.lib().idv_dnsmos_frontend_wfloats()), dtype=torch.float32, device=device)
        call("idv_dnsmos_frontend_pack", p(re), p(im), p(self.fe), st)
        self.w1 = dev(t["conv0_w"].reshape(CONVS[0][1], 9))
        self.b1 = dev(t["conv0_b"])
        self.conv = []
        for k, (ci, co, pool) in enumerate(CONVS[1:], start=1):
            self.conv.append((conv3x3_pack(dev(t[f"conv{k}_w"])), dev(t[f"conv{k}_b"]), ci, co, pool))
        self.dense = [(dev(t[f"dense{k}_w"]), dev(t[f"dense{k}_b"])) for k in range(3)]
        poly = np.zeros((3, 4), dtype=np.float64)
        for j, c in enumerate(POLY[bool(personalized)]):
            poly[j, 4 - len(c):] = c
        self.poly = torch.from_numpy(poly).to(device)
        torch.cuda.current_stream().synchronize()       # the float sources may go; the packs stay


def conv3x3_pack(w: torch.Tensor) -> torch.Tensor:
    """idv_conv3x3_pack: w [Cout, Cin, 3, 3] (device, float32) -> the packed weights idv_conv3x3_fwd streams."""
    ops.check_dev_f32(w, "w")
    co, ci = int(w.shape[0]), int(w.shape[1])
    n = int(ops.L.lib().idv_conv3x3_wfloats(ci, co))
    if w.dtype != torch.float32 or tuple(w.shape[2:]) != (3, 3) or n < 0:
        raise ValueError(f"conv3x3_pack: float32 [Cout in (32, 64), Cin in (32, 64, 128), 3, 3] expected, got {tuple(w.shape)}")
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    call("idv_conv3x3_pack", p(w.contiguous()), i(ci), i(co), p(out), stream_ptr())
    return out


def conv3x3(x: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, cout: int, pool: bool = False) -> torch.Tensor:
    """idv_conv3x3_fwd: x [N, H, W, Cin] -> ReLU(conv3x3 + bias) as [N, H, W, Cout], or its 2x2 max-pool [N, H // 2, W // 2, Cout]."""
    ops.check_dev_f32(x, "x")
    N, H, W, ci = (int(v) for v in x.shape)
    y = torch.empty((N, H // 2, W // 2, cout) if pool else (N, H, W, cout), dtype=torch.float32, device=x.device)
    call("idv_conv3x3_fwd", p(x.contiguous()), p(wp), p(bias), i(N), i(H), i(W), i(ci), i(cout), i(1 if pool else 0), p(y), stream_ptr())
    return y


class DNSMOS:
    """The SIG / BAK / OVRL network of DNSMOS P.835 with the script's polynomials.  ``tensors``: name -> float32 array, the names and
    shapes of :data:`SHAPES`.  Build it with :meth:`from_onnx` or :meth:`from_npz`.

    ``workspace_segments`` (default 8): at most that many segments are in flight at once; one segment needs
    :data:`WORKSPACE_BYTES_PER_SEGMENT` (about 80 MB: two 900 x 161 x 64 maps), so the default bounds the workspace at about 0.65 GB
    whatever the batch.  No bit of any result depends on it."""

    WORKSPACE_BYTES_PER_SEGMENT = 4 * (FRAMES * BINS * (1 + 64 + 64) + 450 * 80 * 32 + 225 * 40 * 32 + 112 * 20 * (32 + 64))

    def __init__(self, tensors: Dict[str, np.ndarray], personalized: bool = False, workspace_segments: int = 8):
        t = {}
        for k, shape in SHAPES.items():
            if k not in tensors:
                raise ValueError(f"DNSMOS: tensor {k!r} is missing")
            a = np.asarray(tensors[k])
            if a.dtype != np.float32 or tuple(a.shape) != shape:
                raise ValueError(f"DNSMOS: tensor {k!r} is {a.dtype} {tuple(a.shape)}, expected float32 {shape}")
            t[k] = a
        if float(t["pow"]) != 2.0 or not float(t["log_floor"]) > 0 or not float(t["log_div"]) > 0:
            raise ValueError("DNSMOS: the feature is ln(max(floor, magnitude ** 2)) / div with floor, div > 0")
        if isinstance(workspace_segments, bool) or not isinstance(workspace_segments, int) or workspace_segments < 1:
            raise ValueError("DNSMOS: workspace_segments must be a positive integer")
        self.tensors = t
        self.personalized = bool(personalized)
        self.workspace_segments = workspace_segments
        self._packs: Dict[torch.device, _Packs] = {}

    # ---- construction
    @classmethod
    def from_onnx(cls, path: str, personalized: bool = False, **kw) -> "DNSMOS":
        """Read ``sig_bak_ovr.onnx`` (or ``pDNSMOS/sig_bak_ovr.onnx`` with ``personalized=True``: the polynomials differ) with the
        reader of this module; ``onnx`` / ``onnxruntime`` are not needed.  Raises ValueError unless the file's node op types are
        :data:`OP_SEQUENCE` and every tensor of :data:`ONNX_NAMES` is there with its shape."""
        ops_, inits = read_onnx(path)
        if tuple(ops_) != OP_SEQUENCE:
            raise ValueError(f"{path}: not the DNSMOS P.835 graph: its {len(ops_)} nodes are {ops_}")
        t = {}
        for k, (name, shape) in ONNX_NAMES.items():
            if name not in inits:
                raise ValueError(f"{path}: initializer {name!r} is missing")
            a = inits[name]
            if a.dtype != np.float32 or tuple(a.shape) != shape:
                raise ValueError(f"{path}: initializer {name!r} is {a.dtype} {tuple(a.shape)}, expected float32 {shape}")
            t[k] = a.reshape(SHAPES[k])
        return cls(t, personalized, **kw)

    @classmethod
    def from_npz(cls, *paths: str, personalized: bool = False, **kw) -> "DNSMOS":
        """The same tensors from ``.npz`` files under the names of :data:`SHAPES`; several files are merged (a set of weights may be
        stored as a front-end file and a network file)."""
        t: Dict[str, np.ndarray] = {}
        for path in paths:
            with np.load(path) as z:
                t.update({k: z[k] for k in z.files if k in SHAPES})
        return cls(t, personalized, **kw)

    def packs(self, device) -> _Packs:
        device = torch.device(device)
        if device.type != "cuda":
            raise ops.L.IdvError(f"DNSMOS: expected a CUDA (ROCm) device, got {device}; the HIP hot path has no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._packs:
            with torch.cuda.device(device):
                self._packs[device] = _Packs(self.tensors, self.personalized, device)
        return self._packs[device]

    # ---- the pieces
    def _features(self, x, lens: ops.Lengths, seg_dev: torch.Tensor, nseg: int) -> torch.Tensor:
        pk = self.packs(x.device)
        feat = torch.empty(nseg, FRAMES, BINS, dtype=torch.float32, device=x.device)
        call("idv_dnsmos_frontend", p(x), ll(x.stride(0)), p(lens.dev), i(x.shape[0]), p(seg_dev), i(nseg), p(pk.fe),
             f(float(self.tensors["log_floor"])), f(float(self.tensors["log_div"])), p(feat), stream_ptr())
        return feat

    def _network(self, feat: torch.Tensor, raw: torch.Tensor) -> None:
        """feat [n, 900, 161] -> raw [n, 3] (written in place)."""
        pk = self.packs(feat.device)
        n = int(feat.shape[0])
        st = stream_ptr()
        wp, bias, ci, co, pool = pk.conv[0]
        y = torch.empty(n, FRAMES, BINS, co, dtype=torch.float32, device=feat.device)
        # the 1 -> 128 layer is evaluated while the 128 -> 64 layer stages its input: its 74 MB map per segment never exists
        call("idv_conv3x3_c1_fused_fwd", p(feat), p(pk.w1), p(pk.b1), i(ci), p(wp), p(bias), i(n), i(FRAMES), i(BINS), i(co), i(0), p(y),
             st)
        for wp, bias, ci, co, pool in pk.conv[1:]:
            y = conv3x3(y, wp, bias, co, pool)
        g = torch.empty(n, 64, dtype=torch.float32, device=feat.device)
        call("idv_conv3x3_gmax", p(y), i(n), ll(y.shape[1] * y.shape[2]), i(64), p(g), st)
        (w0, b0), (w1, b1), (w2, b2) = pk.dense
        call("idv_dnsmos_head", p(g), i(n), p(w0), p(b0), p(w1), p(b1), p(w2), p(b2), p(raw), st)

    def _prepare(self, x, lengths, who: str):
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError(f"{who}: x must be a padded batch [B, L]")
        ops.check_dev_f32(x, "x")
        B, L = (int(v) for v in x.shape)
        if L < 1 or L > MAX_LEN:
            raise ValueError(f"{who}: rows of {L} samples; 1 .. 2^27 are supported")
        host = [L] * B if lengths is None else ops.check_lengths(lengths, B, L, None)
        lens = lengths if isinstance(lengths, ops.Lengths) else ops.Lengths(host, x.device)
        segs, counts = plan_segments(host)
        return ops._ragged_rows(x), lens, segs, counts

    def features(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """The feature maps [S, 900, 161] of every segment of the padded batch x [B, L] (clip by clip, :func:`plan_segments`)."""
        x, lens, segs, _ = self._prepare(x, lengths, "features")
        seg_dev = torch.tensor(segs, dtype=torch.int32, device=x.device).reshape(-1, 2)
        return self._features(x, lens, seg_dev, len(segs))

    def _raw(self, x, lens, segs) -> torch.Tensor:
        S = len(segs)
        raw = torch.empty(S, 3, dtype=torch.float32, device=x.device)
        seg_dev = torch.tensor(segs, dtype=torch.int32, device=x.device).reshape(-1, 2)
        step = self.workspace_segments
        for s0 in range(0, S, step):
            n = min(step, S - s0)
            feat = self._features(x, lens, seg_dev[s0:s0 + n], n)
            self._network(feat, raw[s0:s0 + n])
        return raw

    def raw(self, segments: torch.Tensor) -> torch.Tensor:
        """segments [N, 144160] (device, float32, 16 kHz) -> [N, 3] = (SIG_raw, BAK_raw, OVRL_raw): the network alone."""
        if not isinstance(segments, torch.Tensor) or segments.dim() != 2 or segments.shape[1] != SEG_SAMPLES:
            raise ValueError(f"raw: segments must be [N, {SEG_SAMPLES}]")
        ops.check_dev_f32(segments, "segments")
        N = int(segments.shape[0])
        x = ops._ragged_rows(segments)
        return self._raw(x, ops.Lengths([SEG_SAMPLES] * N, x.device), [(n, 0) for n in range(N)])

    def score(self, x: torch.Tensor, lengths=None, fs: int = 16000, per_segment: bool = False) -> Dict[str, torch.Tensor]:
        """Score the padded batch x [B, L] (device, float32) -> ``{"OVRL_raw", "SIG_raw", "BAK_raw", "OVRL", "SIG", "BAK"}``: float64
        device tensors [B], the clip's means over its segments (double sums in segment order), and ``"num_hops"``: int64 [B] on the
        host, the script's column of that name (it counts the hops the script skips too, :func:`hop_is_scored`).  ``lengths`` (a
        python sequence or a CPU integer tensor): row b holds lengths[b] >= 1 samples; nothing behind them is read and a row's
        values do not depend on the rest of the batch.  A clip shorter than 9.01 s is continued with itself, as the script does.
        ``fs != 16000`` goes through :func:`inference.resample` first -- the script calls ``librosa.resample``, a different filter,
        so that case is unpinned.  ``per_segment``: also ``"segments_raw"`` [S, 3] float32 (SIG, BAK, OVRL of every segment, clip by
        clip) and ``"segments"`` (int64 [B], segments per clip)."""
        if fs != FS:
            from . import inference
            x, lengths = inference.resample(x, fs, FS, lengths)
        x, lens, segs, counts = self._prepare(x, lengths, "score")
        B = int(x.shape[0])
        raw = self._raw(x, lens, segs)
        first = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int32)
        first_dev = torch.from_numpy(first).to(x.device)
        count_dev = torch.tensor(counts, dtype=torch.int32, device=x.device)
        out = torch.empty(B, 6, dtype=torch.float64, device=x.device)
        call("idv_dnsmos_clip", p(raw), i(len(segs)), p(first_dev), p(count_dev), i(B), p(self.packs(x.device).poly), p(out), stream_ptr())
        res = {k: out[:, j] for j, k in enumerate(("SIG_raw", "BAK_raw", "OVRL_raw", "SIG", "BAK", "OVRL"))}
        res["num_hops"] = torch.tensor([num_hops(v)[1] for v in lens.host], dtype=torch.int64)
        if per_segment:
            res["segments_raw"] = raw
            res["segments"] = torch.tensor(counts, dtype=torch.int64)
        return res
