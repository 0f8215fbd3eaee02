"""DNSMOS P.835 on the device: SIG / BAK / OVRL of recordings without a clean reference (csrc/dnsmos.hip).

The definition is the reference's ``DNSMOS/dnsmos_local.py:49-100`` around the network of ``sig_bak_ovr.onnx`` (the personalized
model: another file with the same graph, and other polynomials), restated in float64 in ``tests/dnsmos_ref.py``.  Parity with
onnxruntime itself is unpinned (it is not installed where this library is tested).  The script's fourth column, ``P808_MOS``
(``model_v8.onnx`` on a librosa mel spectrogram), is the class :class:`P808` at the end of this module (csrc/p808.hip, the float64
definition in ``tests/p808_ref.py``; parity with librosa and onnxruntime themselves is unpinned for the same reason).

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


def _prepare_batch(x, lengths, who: str):
    """The checks and the planned segment table both models share -> (rows, Lengths, segments, counts)."""
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


def _clip_tables(counts, device):
    first = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int32)
    return torch.from_numpy(first).to(device), torch.tensor(counts, dtype=torch.int32, device=device)


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
        return _prepare_batch(x, lengths, who)

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

    def score(self, x: torch.Tensor, lengths=None, fs: int = 16000, per_segment: bool = False, p808=None) -> Dict[str, torch.Tensor]:
        """Score the padded batch x [B, L] (device, float32) -> ``{"OVRL_raw", "SIG_raw", "BAK_raw", "OVRL", "SIG", "BAK"}``: float64
        device tensors [B], the clip's means over its segments (double sums in segment order), and ``"num_hops"``: int64 [B] on the
        host, the script's column of that name (it counts the hops the script skips too, :func:`hop_is_scored`).  ``lengths`` (a
        python sequence or a CPU integer tensor): row b holds lengths[b] >= 1 samples; nothing behind them is read and a row's
        values do not depend on the rest of the batch.  A clip shorter than 9.01 s is continued with itself, as the script does.
        ``fs != 16000`` goes through :func:`inference.resample` first -- the script calls ``librosa.resample``, a different filter,
        so that case is unpinned.  ``per_segment``: also ``"segments_raw"`` [S, 3] float32 (SIG, BAK, OVRL of every segment, clip by
        clip) and ``"segments"`` (int64 [B], segments per clip).  ``p808`` (a :class:`P808` model): also ``"P808_MOS"``, float64 [B],
        the mean of ``model_v8.onnx`` over the same segments (one planned segment table serves both models), and with
        ``per_segment`` ``"segments_p808"`` [S] float32; without it the keys and bits are those of the call without the argument."""
        if fs != FS:
            from . import inference
            x, lengths = inference.resample(x, fs, FS, lengths)
        x, lens, segs, counts = self._prepare(x, lengths, "score")
        if p808 is not None and not isinstance(p808, P808):
            raise ValueError("score: p808 must be a dnsmos.P808 model or None")
        B = int(x.shape[0])
        raw = self._raw(x, lens, segs)
        first_dev, count_dev = _clip_tables(counts, x.device)
        out = torch.empty(B, 6, dtype=torch.float64, device=x.device)
        call("idv_dnsmos_clip", p(raw), i(len(segs)), p(first_dev), p(count_dev), i(B), p(self.packs(x.device).poly), p(out), stream_ptr())
        res = {k: out[:, j] for j, k in enumerate(("SIG_raw", "BAK_raw", "OVRL_raw", "SIG", "BAK", "OVRL"))}
        res["num_hops"] = torch.tensor([num_hops(v)[1] for v in lens.host], dtype=torch.int64)
        if per_segment:
            res["segments_raw"] = raw
            res["segments"] = torch.tensor(counts, dtype=torch.int64)
        if p808 is not None:
            raw8 = p808._raw(x, lens, segs)
            res["P808_MOS"] = p808._clip(raw8, first_dev, count_dev)
            if per_segment:
                res["segments_p808"] = raw8
        return res


# ---------------------------------------------------------------------------------------------------------- P.808 (P808_MOS)
P808_SAMPLES = 144000                # audio_seg[:-160]: sample 144000 .. 144159 of a segment are not part of the feature
P808_NFFT, P808_MELS, P808_KPAD = 321, 120, 324

# (in, out, pooled) of the five convolutions of model_v8.onnx
P808_CONVS = ((1, 32, True), (32, 32, True), (32, 32, False), (32, 32, True), (32, 64, False))
P808_DENSE = ((64, 64), (64, 64), (64, 1))

# the graph of model_v8.onnx: its nodes' op types in file order
P808_OP_SEQUENCE = (
    "Unsqueeze", "Transpose", "Conv", "Relu", "MaxPool", "Conv", "Relu", "MaxPool", "Conv", "Relu", "Conv", "Relu", "MaxPool", "Conv", "Relu",
    "Transpose", "ReduceMax", "MatMul", "Add", "Relu", "MatMul", "Add", "Relu", "MatMul", "Add")

_P808_DENSE_NAME = "mos_estimator_small_1/dense_{}/{}/ReadVariableOp/resource:0"
P808_ONNX_NAMES: Dict[str, Tuple[str, Tuple[int, ...]]] = {}
for _k, (_ci, _co, _) in enumerate(P808_CONVS):
    P808_ONNX_NAMES[f"conv{_k}_w"] = (f"conv2d_{_k + 5}/kernel:0", (_co, _ci, 3, 3))
    P808_ONNX_NAMES[f"conv{_k}_b"] = (f"conv2d_{_k + 5}/bias:0", (_co,))
for _k, (_ci, _co) in enumerate(P808_DENSE):
    P808_ONNX_NAMES[f"dense{_k}_w"] = (_P808_DENSE_NAME.format(_k + 3, "MatMul"), (_ci, _co))
    P808_ONNX_NAMES[f"dense{_k}_b"] = (_P808_DENSE_NAME.format(_k + 3, "BiasAdd"), (_co,))
P808_SHAPES = {k: shape for k, (_, shape) in P808_ONNX_NAMES.items()}


def p808_window() -> np.ndarray:
    """``scipy.signal.get_window("hann", 321, fftbins=True)`` as scipy makes it (``general_cosine`` of the extended, then truncated,
    window): ``fac = linspace(-pi, pi, 322)``, ``w = 0.5 cos(0 fac) + 0.5 cos(1 fac)``, the last sample dropped."""
    fac = np.linspace(-np.pi, np.pi, P808_NFFT + 1)
    w = np.zeros(P808_NFFT + 1)
    for k, a in enumerate((0.5, 0.5)):
        w += a * np.cos(k * fac)
    return w[:-1]


def p808_dft_table(window: np.ndarray = None) -> np.ndarray:
    """The windowed DFT of 321 points as a table [2, 161, 324] (float64): ``[0, k, n] = cos(2 pi k n / 321) w[n]``, ``[1, k, n] =
    -sin(2 pi k n / 321) w[n]``, zeros for n = 321 .. 323.  The angle is reduced in integers (k n mod 321) before it is formed."""
    w = p808_window() if window is None else np.asarray(window, dtype=np.float64)
    k, n = np.arange(BINS)[:, None], np.arange(P808_NFFT)[None, :]
    ang = 2.0 * np.pi * ((k * n) % P808_NFFT).astype(np.float64) / P808_NFFT
    tab = np.zeros((2, BINS, P808_KPAD))
    tab[0, :, :P808_NFFT] = np.cos(ang) * w
    tab[1, :, :P808_NFFT] = -np.sin(ang) * w
    return tab


def _hz_to_mel(f: float) -> float:
    """librosa.convert.hz_to_mel (Slaney) of a scalar."""
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = (min_log_hz - 0.0) / f_sp
    logstep = np.log(6.4) / 27.0
    if f >= min_log_hz:
        return min_log_mel + np.log(f / min_log_hz) / logstep
    return (f - 0.0) / f_sp


def _mel_to_hz(mels: np.ndarray) -> np.ndarray:
    """librosa.convert.mel_to_hz (Slaney) of an array."""
    f_sp = 200.0 / 3
    freqs = 0.0 + f_sp * mels
    min_log_hz = 1000.0
    min_log_mel = (min_log_hz - 0.0) / f_sp
    logstep = np.log(6.4) / 27.0
    log_t = mels >= min_log_mel
    freqs[log_t] = min_log_hz * np.exp(logstep * (mels[log_t] - min_log_mel))
    return freqs


def p808_mel_basis() -> np.ndarray:
    """``librosa.filters.mel(sr=16000, n_fft=321, n_mels=120)`` of librosa 0.10.2 (Slaney scale, fmin = 0, fmax = 8000, norm = "slaney",
    dtype float32) -> float32 [120, 161].  The triangles are stored into a float32 array, which is then multiplied in place by the
    float64 ``enorm``: two float32 roundings."""
    weights = np.zeros((P808_MELS, 1 + P808_NFFT // 2), dtype=np.float32)
    fftfreqs = np.arange(0, P808_NFFT // 2 + 1, dtype=int) * (1.0 / (P808_NFFT * (1.0 / FS)))        # np.fft.rfftfreq
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(FS / 2), P808_MELS + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for m in range(P808_MELS):
        lower = -ramps[m] / fdiff[m]
        upper = ramps[m + 2] / fdiff[m + 1]
        weights[m] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:P808_MELS + 2] - mel_f[:P808_MELS])
    weights *= enorm[:, np.newaxis]
    return weights


class _P808Packs:
    def __init__(self, model: "P808", device):
        t = model.tensors

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        self.dft = torch.from_numpy(np.ascontiguousarray(model.dft, dtype=np.float64)).to(device)
        self.mel = torch.from_numpy(np.ascontiguousarray(model.mel, dtype=np.float64)).to(device)
        self.w1 = dev(t["conv0_w"].reshape(P808_CONVS[0][1], 9))
        self.b1 = dev(t["conv0_b"])
        self.conv = [(conv3x3_pack(dev(t[f"conv{k}_w"])), dev(t[f"conv{k}_b"]), co, pool)
                     for k, (ci, co, pool) in enumerate(P808_CONVS[1:], start=1)]
        self.dense = [(dev(t[f"dense{k}_w"]), dev(t[f"dense{k}_b"])) for k in range(3)]
        torch.cuda.current_stream().synchronize()


class P808:
    """The network of ``model_v8.onnx`` behind the librosa mel front end of ``dnsmos_local.py`` (``audio_melspec``): the script's
    ``P808_MOS`` column.  ``tensors``: name -> float32 array, the names and shapes of :data:`P808_SHAPES`.  Build it with
    :meth:`from_onnx` or :meth:`from_npz` and hand it to :meth:`DNSMOS.score`, :func:`inference.compute_dnsmos` or
    :func:`inference.dnsmos_list` as ``p808=``.

    The Hann window, the windowed DFT table and the mel basis are made here in float64 numpy by the rules of scipy / librosa 0.10.2
    (:func:`p808_window`, :func:`p808_dft_table`, :func:`p808_mel_basis`); ``dft`` [2, 161, 324] and ``mel`` [120, 161] replace them
    (tests pass integer stand-ins).  ``workspace_segments`` (default 32): at most that many segments are in flight at once (about
    7 MB each: the double mel power, the feature and the 450 x 60 x 32 map); no bit of any result depends on it."""

    def __init__(self, tensors: Dict[str, np.ndarray], workspace_segments: int = 32, dft: np.ndarray = None, mel: np.ndarray = None):
        t = {}
        for k, shape in P808_SHAPES.items():
            if k not in tensors:
                raise ValueError(f"P808: tensor {k!r} is missing")
            a = np.asarray(tensors[k])
            if a.dtype != np.float32 or tuple(a.shape) != shape:
                raise ValueError(f"P808: tensor {k!r} is {a.dtype} {tuple(a.shape)}, expected float32 {shape}")
            t[k] = a
        if isinstance(workspace_segments, bool) or not isinstance(workspace_segments, int) or workspace_segments < 1:
            raise ValueError("P808: workspace_segments must be a positive integer")
        self.tensors = t
        self.workspace_segments = workspace_segments
        self.dft = p808_dft_table() if dft is None else np.asarray(dft, dtype=np.float64)
        self.mel = p808_mel_basis().astype(np.float64) if mel is None else np.asarray(mel, dtype=np.float64)
        if self.dft.shape != (2, BINS, P808_KPAD) or self.mel.shape != (P808_MELS, BINS) or np.any(self.dft[:, :, P808_NFFT:] != 0):
            raise ValueError(f"P808: dft must be [2, {BINS}, {P808_KPAD}] with zeros from column {P808_NFFT} on, mel [{P808_MELS}, {BINS}]")
        self._packs: Dict[torch.device, _P808Packs] = {}

    @classmethod
    def from_onnx(cls, path: str, **kw) -> "P808":
        """Read ``model_v8.onnx`` with :func:`read_onnx`.  Raises ValueError unless the file's node op types are
        :data:`P808_OP_SEQUENCE` and the 16 tensors of :data:`P808_ONNX_NAMES` are there with their shapes."""
        ops_, inits = read_onnx(path)
        if tuple(ops_) != P808_OP_SEQUENCE:
            raise ValueError(f"{path}: not the DNSMOS P.808 graph: its {len(ops_)} nodes are {ops_}")
        t = {}
        for k, (name, shape) in P808_ONNX_NAMES.items():
            if name not in inits:
                raise ValueError(f"{path}: initializer {name!r} is missing")
            a = inits[name]
            if a.dtype != np.float32 or tuple(a.shape) != shape:
                raise ValueError(f"{path}: initializer {name!r} is {a.dtype} {tuple(a.shape)}, expected float32 {shape}")
            t[k] = a
        return cls(t, **kw)

    @classmethod
    def from_npz(cls, path: str, **kw) -> "P808":
        """The same tensors from an ``.npz`` file under the names of :data:`P808_SHAPES`."""
        with np.load(path) as z:
            t = {k: z[k] for k in z.files if k in P808_SHAPES}
        return cls(t, **kw)

    def packs(self, device) -> _P808Packs:
        device = torch.device(device)
        if device.type != "cuda":
            raise ops.L.IdvError(f"P808: expected a CUDA (ROCm) device, got {device}; the HIP hot path has no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._packs:
            with torch.cuda.device(device):
                self._packs[device] = _P808Packs(self, device)
        return self._packs[device]

    # ---- the pieces
    def _mel_power(self, x, lens: ops.Lengths, seg_dev: torch.Tensor, nseg: int) -> Tuple[torch.Tensor, torch.Tensor]:
        pk = self.packs(x.device)
        S = torch.empty(nseg, FRAMES, P808_MELS, dtype=torch.float64, device=x.device)
        smax = torch.empty(nseg, dtype=torch.float64, device=x.device)
        work = torch.empty(int(ops.L.lib().idv_p808_mel_work_doubles(nseg)), dtype=torch.float64, device=x.device)
        call("idv_p808_mel", p(x), ll(x.stride(0)), p(lens.dev), i(x.shape[0]), p(seg_dev), i(nseg), p(pk.dft), p(pk.mel), p(S), p(smax),
             p(work), stream_ptr())
        return S, smax

    def _features(self, x, lens, seg_dev, nseg: int) -> torch.Tensor:
        S, smax = self._mel_power(x, lens, seg_dev, nseg)
        feat = torch.empty(nseg, FRAMES, P808_MELS, dtype=torch.float32, device=x.device)
        call("idv_p808_db", p(S), p(smax), i(nseg), ll(FRAMES * P808_MELS), p(feat), stream_ptr())
        return feat

    def _network(self, feat: torch.Tensor, raw: torch.Tensor) -> None:
        """feat [n, 900, 120] -> raw [n] (written in place)."""
        pk = self.packs(feat.device)
        n, H, W = (int(v) for v in feat.shape)
        st = stream_ptr()
        c1 = P808_CONVS[0][1]
        # the first layer and its pool in one launch: the 900 x 120 x 32 map never exists
        y = torch.empty(n, H // 2, W // 2, c1, dtype=torch.float32, device=feat.device)
        call("idv_conv3x3_c1_pool_fwd", p(feat), p(pk.w1), p(pk.b1), i(n), i(H), i(W), i(c1), p(y), st)
        for wp, bias, co, pool in pk.conv:
            y = conv3x3(y, wp, bias, co, pool)
        g = torch.empty(n, 64, dtype=torch.float32, device=feat.device)
        call("idv_conv3x3_gmax", p(y), i(n), ll(y.shape[1] * y.shape[2]), i(64), p(g), st)
        (w0, b0), (w1, b1), (w2, b2) = pk.dense
        call("idv_p808_head", p(g), i(n), p(w0), p(b0), p(w1), p(b1), p(w2), p(b2), p(raw), st)

    def _seg_table(self, segs, device) -> torch.Tensor:
        return torch.tensor(segs, dtype=torch.int32, device=device).reshape(-1, 2)

    def mel_power(self, x: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(S [S, 900, 120], max [S])`` in float64: the mel power of every segment of the padded batch x [B, L] before the
        decibels, and each segment's maximum."""
        x, lens, segs, _ = _prepare_batch(x, lengths, "mel_power")
        return self._mel_power(x, lens, self._seg_table(segs, x.device), len(segs))

    def features(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """The feature maps [S, 900 (time), 120 (mel)] of every segment of the padded batch x [B, L] (clip by clip,
        :func:`plan_segments`): ``((power_to_db(melspectrogram(seg[:-160]), ref=max) + 40) / 40).T`` as float32."""
        x, lens, segs, _ = _prepare_batch(x, lengths, "features")
        return self._features(x, lens, self._seg_table(segs, x.device), len(segs))

    def _raw(self, x, lens, segs) -> torch.Tensor:
        S = len(segs)
        raw = torch.empty(S, dtype=torch.float32, device=x.device)
        seg_dev = self._seg_table(segs, x.device)
        step = self.workspace_segments
        for s0 in range(0, S, step):
            n = min(step, S - s0)
            self._network(self._features(x, lens, seg_dev[s0:s0 + n], n), raw[s0:s0 + n])
        return raw

    def _clip(self, raw: torch.Tensor, first_dev: torch.Tensor, count_dev: torch.Tensor) -> torch.Tensor:
        B = int(first_dev.shape[0])
        out = torch.empty(B, dtype=torch.float64, device=raw.device)
        call("idv_p808_clip", p(raw), i(raw.shape[0]), p(first_dev), p(count_dev), i(B), p(out), stream_ptr())
        return out

    def raw(self, segments: torch.Tensor) -> torch.Tensor:
        """segments [N, 144160] (device, float32, 16 kHz) -> [N] float32: the front end and the network alone (the last 160 samples
        of a segment are not read, as the script's ``audio_seg[:-160]``)."""
        if not isinstance(segments, torch.Tensor) or segments.dim() != 2 or segments.shape[1] != SEG_SAMPLES:
            raise ValueError(f"raw: segments must be [N, {SEG_SAMPLES}]")
        ops.check_dev_f32(segments, "segments")
        N = int(segments.shape[0])
        x = ops._ragged_rows(segments)
        return self._raw(x, ops.Lengths([SEG_SAMPLES] * N, x.device), [(n, 0) for n in range(N)])

    def score(self, x: torch.Tensor, lengths=None, per_segment: bool = False) -> Dict[str, torch.Tensor]:
        """``{"P808_MOS"}`` (float64 [B], the mean over a clip's segments as a double sum in segment order) of the padded batch x
        [B, L] at 16 kHz; ``per_segment``: also ``"segments_p808"`` [S] float32 and ``"segments"`` (int64 [B])."""
        x, lens, segs, counts = _prepare_batch(x, lengths, "score")
        raw = self._raw(x, lens, segs)
        res = {"P808_MOS": self._clip(raw, *_clip_tables(counts, x.device))}
        if per_segment:
            res["segments_p808"] = raw
            res["segments"] = torch.tensor(counts, dtype=torch.int64)
        return res
