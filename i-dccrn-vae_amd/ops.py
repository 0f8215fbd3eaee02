"""Thin host wrappers over the C ABI: planar-J activation buffers and one python function per
idv_* operator.  PyTorch is used for device memory and streams only; all arithmetic of the hot
path happens inside libidccrn_hip.so."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._lib import call, p, i, f, d, ll, stream_ptr

SLACK = 256

# Arithmetic of the complex conv / transposed-conv contraction:
#   "fp32"   exact fp32 MFMA (v_mfma_f32_32x32x2_f32)                       -- default
#   "bf16x3" split-precision bf16 MFMA, fp32 accumulate (3 MFMAs per k block) -- ~1e-5 waveform error, ~2x faster
PRECISION = os.environ.get("IDV_PRECISION", "fp32")


def set_precision(mode: str):
    global PRECISION
    if mode not in ("fp32", "bf16x3"):
        raise ValueError("precision must be 'fp32' or 'bf16x3'")
    PRECISION = mode


def bucket(n: int) -> int:
    """Round a buffer length up to one of 8 size classes per octave (<= 12.5 % slack).  Layer outputs of
    slightly different sizes then land in the same class, so the caching allocator re-uses whole blocks
    instead of splitting multi-GB ones and calling hipMalloc again on the next step."""
    if n <= 4096:
        return n
    step = 1 << (n.bit_length() - 4)
    return (n + step - 1) // step * step


ROWS_MAX_LEN = 1 << 27         # samples per row of the row-signal kernels (csrc/rows.hpp)
ROWS_MAX_ROWS = 65535          # rows of one call
_WORK = {}                     # (device, stream, tag, dtype) -> work buffer, grow-only


def _scratch(n: int, device, tag="w", dtype=torch.float32) -> torch.Tensor:
    """The grow-only work buffer of (device, its current stream, tag, dtype), at least ``n`` elements: weight-gradient partials
    reused across layers and steps, the window sums of trimming and mixing (a corpus of many batch sizes keeps the largest only)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, torch.cuda.current_stream(device).cuda_stream, tag, dtype)
    t = _WORK.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(bucket(n), dtype=dtype, device=device)
        _WORK[key] = t
    return t


class Planar:
    """A planar-J activation  act[2][C][F][Jp]  (see include/idccrn_hip.h).

    ``T`` is the number of valid frames (t_valid); ``Tp`` = T_stft + 1 columns per utterance.
    ``tensor5()`` exposes it with the reference's shape [B, C, F, T, 2] as a strided view.
    ``lengths``: the :class:`Lengths` of a batch of utterances of different lengths (set by ``stft(..., lengths=)`` on the
    spectrum it returns, None everywhere else); ``T`` is then the longest utterance's frame count.
    """

    __slots__ = ("buf", "C", "F", "B", "T", "Tp", "Jp", "lengths")

    def __init__(self, buf, C, F, B, T, Tp, Jp, lengths=None):
        self.buf, self.C, self.F, self.B, self.T, self.Tp, self.Jp, self.lengths = buf, C, F, B, T, Tp, Jp, lengths

    @staticmethod
    def jp_for(B: int, Tp: int) -> int:
        return (B * Tp + 3) // 4 * 4

    @classmethod
    def empty(cls, C, F, B, T, Tp, device, zero=False):
        Jp = cls.jp_for(B, Tp)
        n = bucket(2 * C * F * Jp + 2 * SLACK)
        buf = (torch.zeros if zero else torch.empty)(n, dtype=torch.float32, device=device)
        return cls(buf, C, F, B, T, Tp, Jp)

    @property
    def data(self) -> torch.Tensor:
        return self.buf[SLACK:SLACK + 2 * self.C * self.F * self.Jp]

    def ptr(self, plane_offset: int = 0):
        """Device pointer to plane `plane_offset` (planes are F*Jp floats... of size Jp per row)."""
        return L._P(self.buf.data_ptr() + 4 * (SLACK + plane_offset * self.F * self.Jp))

    def planes(self) -> torch.Tensor:
        """[2, C, F, B, Tp] view (requires Jp == B*Tp padding handled by as_strided)."""
        return torch.as_strided(self.buf, (2, self.C, self.F, self.B, self.Tp),
                                (self.C * self.F * self.Jp, self.F * self.Jp, self.Jp, self.Tp, 1), SLACK)

    def tensor5(self) -> torch.Tensor:
        """Reference-shaped view [B, C, F, T, 2]."""
        return self.planes()[..., 1:1 + self.T].permute(3, 1, 2, 4, 0)

    def tensor4(self) -> torch.Tensor:
        """[B, F, T, 2] view for C == 1 (or [B, C*F...] callers reshape themselves)."""
        return self.tensor5()[:, 0]

    def channel_slice(self, c0: int, c1: int) -> torch.Tensor:
        """[B, T, c1-c0, 2] view for F == 1 activations (LSTM outputs / latents)."""
        assert self.F == 1
        return self.planes()[:, c0:c1, 0, :, 1:1 + self.T].permute(2, 3, 1, 0)

    @classmethod
    def from_tensor5(cls, x: torch.Tensor, Tp: Optional[int] = None):
        """Copy a reference-layout tensor [B, C, F, T, 2] into a fresh planar buffer."""
        B, C, F, T, _ = x.shape
        Tp = Tp or T + 1
        out = cls.empty(C, F, B, T, Tp, x.device, zero=True)
        out.tensor5().copy_(x)
        return out


IMG_SLACK = 4096          # bf16 elements kept readable before, between and after the two planes of an Image
IMAGE_PATH = os.environ.get("IDV_IMAGE_PATH", "1") != "0"     # eval bf16x3: keep inter-layer activations as split images
IMAGE_TRAIN = os.environ.get("IDV_IMAGE_TRAIN", "1") != "0"   # bf16x3 training: feed the conv kernels split images too


class Image:
    """A split-bf16 activation image  img[hi|lo][(2C+7)//8][F][Jp][8]  (include/idccrn_hip.h, "split image"): what the
    bf16x3 conv kernels stage into LDS verbatim.  Same (C, F, B, T, Tp, Jp) meaning as Planar."""

    __slots__ = ("buf", "C", "F", "B", "T", "Tp", "Jp", "lo_off")

    def __init__(self, buf, C, F, B, T, Tp, Jp, lo_off):
        self.buf, self.C, self.F, self.B, self.T, self.Tp, self.Jp, self.lo_off = buf, C, F, B, T, Tp, Jp, lo_off

    @classmethod
    def empty(cls, C, F, B, T, Tp, device):
        Jp = Planar.jp_for(B, Tp)
        plane = (2 * C + 7) // 8 * F * Jp * 8
        lo_off = plane + IMG_SLACK
        buf = torch.empty(bucket(2 * IMG_SLACK + lo_off + plane), dtype=torch.int16, device=device)
        return cls(buf, C, F, B, T, Tp, Jp, lo_off)

    def ptr(self):
        return L._P(self.buf.data_ptr() + 2 * IMG_SLACK)

    @property
    def lo_slots(self) -> int:
        return self.lo_off // 8


def to_image(x: Planar) -> Image:
    out = Image.empty(x.C, x.F, x.B, x.T, x.Tp, x.buf.device)
    call("idv_planar_to_image", x.ptr(), i(x.C), i(x.F), i(x.B * x.Tp), i(x.Jp), out.ptr(), ll(out.lo_off), stream_ptr())
    return out


def to_image_repeat(x: Planar, n: int) -> Image:
    """to_image(repeat_batch(x, n)) in one pass: each utterance n times in a row, straight into the split image."""
    out = Image.empty(x.C, x.F, x.B * n, x.T, x.Tp, x.buf.device)
    call("idv_planar_to_image_repeat", x.ptr(), i(x.C), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(n), out.ptr(), ll(out.lo_off),
         i(out.Jp), stream_ptr())
    return out


def to_planar(x: Image) -> Planar:
    out = Planar.empty(x.C, x.F, x.B, x.T, x.Tp, x.buf.device)
    call("idv_image_to_planar", x.ptr(), ll(x.lo_off), i(x.C), i(x.F), i(x.B * x.Tp), i(x.Jp), out.ptr(), stream_ptr())
    return out


class KImage:
    """K-major split image  kimg[hi|lo][nplanes/8][Jp][8]  (octet o = planes 8o..8o+7): the activation operand of the
    bf16x3 point-wise contractions (LSTM projection, DFT, dense)."""

    __slots__ = ("buf", "nplanes", "Jp", "lo_off")

    def __init__(self, nplanes: int, Jp: int, device):
        assert nplanes % 8 == 0
        plane = nplanes // 8 * Jp * 8
        self.nplanes, self.Jp, self.lo_off = nplanes, Jp, plane + IMG_SLACK
        self.buf = torch.empty(bucket(2 * IMG_SLACK + self.lo_off + plane), dtype=torch.int16, device=device)

    def ptr(self, octet: int = 0):
        return L._P(self.buf.data_ptr() + 2 * IMG_SLACK + 16 * octet * self.Jp)

    @property
    def lo_slots(self) -> int:
        return self.lo_off // 8

    @classmethod
    def from_planes(cls, x_ptr, nvalid: int, J: int, Jp: int, device, pad_to: int = 8):
        nplanes = (nvalid + pad_to - 1) // pad_to * pad_to
        out = cls(nplanes, Jp, device)
        call("idv_planar_to_kimage", x_ptr, i(nvalid), i(nplanes), i(J), i(Jp), out.ptr(), ll(out.lo_off), stream_ptr())
        return out


def pack_pw_bf16(w):
    M, K = w.shape
    wf = torch.empty(int(L.lib().idv_pw_bf16_wfrag_bytes(i(M), i(K))), dtype=torch.uint8, device=w.device)
    call("idv_pack_pw_bf16", p(w.contiguous()), i(M), i(K), p(wf), stream_ptr())
    return wf


def pw_bf16x3(kimg: KImage, octet0: int, K: int, wfrag16, bias, M: int, B: int, Tp: int, t_valid: int, out_ptr):
    call("idv_pw_bf16x3", kimg.ptr(octet0), ll(kimg.lo_slots), i(K), p(wfrag16), p(bias), out_ptr, i(M), i(B), i(Tp), i(kimg.Jp),
         i(t_valid), stream_ptr())


def pw_bf16x3_rows(kimg: KImage, K: int, wfrag16, bias, M: int, ldo: int, B: int, T: int, Tp: int, out_ptr):
    """out[(t*B + b)*ldo + m] = sum_k W[m][k] x[k][(b, t)] + bias[m] over the valid frames (row-major, as idv_lstm_bptt reads)."""
    call("idv_pw_bf16x3_rows", kimg.ptr(), ll(kimg.lo_slots), i(K), p(wfrag16), p(bias), out_ptr, i(M), i(ldo), i(B), i(T), i(Tp),
         i(kimg.Jp), stream_ptr())


def _dev_scratch(n: int, device, dtype=torch.float32, zero=False):
    return (torch.zeros if zero else torch.empty)(n, dtype=dtype, device=device)


# ----------------------------------------------------------------------------- packing
def mtiles_alloc(M: int) -> int:
    return (M + 127) // 128 * 4


def cbn_fold(moments, g_rr, g_ri, g_ii, b_r, b_i):
    """moments: [5, C] tensor (mean_r, mean_i, Vrr, Vri, Vii) -> fold [C, 6]."""
    C = g_rr.numel()
    fold = torch.empty(C, 6, dtype=torch.float32, device=g_rr.device)
    call("idv_cbn_fold", p(moments), p(g_rr), p(g_ri), p(g_ii), p(b_r), p(b_i), i(C), p(fold), stream_ptr())
    return fold


def _conv_channels(w_re, cin_used: Optional[int], transposed: bool):
    """-> (cout, cin_total, cin_used) of a conv weight [Cout][Cin][5][2] / transposed conv weight [Cin][Cout][5][2]; cin_used None:
    all input channels."""
    cin_total, cout = (w_re.shape[0], w_re.shape[1]) if transposed else (w_re.shape[1], w_re.shape[0])
    return cout, cin_total, cin_total if cin_used is None else cin_used


def pack_cconv(w_re, w_im, b_re, b_im, fold, cin_used: Optional[int] = None, transposed=False):
    """-> (wfrag, bias) for idv_cconv2d_fwd."""
    cout, cin_total, cin_used = _conv_channels(w_re, cin_used, transposed)
    cck = L.lib().idv_cconv_cck(cin_used)
    ccp = (2 * cin_used + cck - 1) // cck * cck
    mt = mtiles_alloc(2 * cout)
    wfrag = torch.empty(mt * ccp * 5 * 64, dtype=torch.float32, device=w_re.device)
    bias = torch.empty(mt * 32, dtype=torch.float32, device=w_re.device)
    call("idv_pack_cconv", p(w_re.contiguous()), p(w_im.contiguous()), p(b_re.contiguous()), p(b_im.contiguous()),
         p(fold), i(cout), i(cin_total), i(cin_used), i(1 if transposed else 0), p(wfrag), p(bias), stream_ptr())
    return wfrag, bias


SKIP_ONCE = os.environ.get("IDV_SKIP_ONCE", "1") != "0"      # fp32 eval, repeated skips: skip half of a decoder conv once per utterance
GAUSS_FWD = os.environ.get("IDV_GAUSS_FWD", "1") != "0"      # A/B switches: forward / data gradient on cgemm_kernel instead
GAUSS_BWD = os.environ.get("IDV_GAUSS_BWD", "1") != "0"


def gauss_supported(c0: int, c1: int, cout: int, bwd: bool = False) -> bool:
    """fp32 mode: does the three-product (Gauss) contraction kernel serve this layer (csrc/cgemm_gauss.hip)?"""
    if not (GAUSS_BWD if bwd else GAUSS_FWD):
        return False
    return bool(L.lib().idv_cconv_gauss_supported(i(c0), i(c1), i(cout)))


class GaussPack(NamedTuple):
    """Operands of one exact-fp32 conv / transposed conv for the kernels that take the three-product (Gauss) form."""
    wfrag3: torch.Tensor             # three-product fragments (idv_cconv2d_gauss_fwd)
    epi: torch.Tensor                # epilogue table: bias and, with has_fold, the folded batch norm
    has_fold: int
    wino: Optional[torch.Tensor]     # Winograd fragments (idv_cconv2d_wino_fwd), None: not packed (WINO off)
    tw: Optional[torch.Tensor]       # time-Winograd fragments of the operator's form (idv_ctconv2d_tw_fwd / idv_cconv2d_tw_fwd) or None


def pack_cconv_gauss(w_re, w_im, b_re, b_im, fold, cin_used: Optional[int] = None, transposed=False, *, adjoint_of=None) -> GaussPack:
    """-> GaussPack for cconv2d(gauss=) / cconv_dgrad(gauss=).  adjoint_of=(cout_adj, cin_total_adj, cin_used_adj, adj_transposed):
    the data-gradient operator (conjugate-transposed weights, no bias), arguments describing the adjoint as pack_cconv_adjoint."""
    if adjoint_of is not None:
        cout, cin_total, cin_used, transposed = adjoint_of
    else:
        cout, cin_total, cin_used = _conv_channels(w_re, cin_used, transposed)
    lib = L.lib()
    wfrag = torch.empty(int(lib.idv_cconv_gauss_wfrag_floats(i(cout), i(cin_used))), dtype=torch.float32, device=w_re.device)
    epi = torch.empty(int(lib.idv_cconv_gauss_epi_rows(i(cout))) * 8, dtype=torch.float32, device=w_re.device)
    if adjoint_of is not None:
        # adjoint of a conv [Cout][Cin] is a transposed conv whose [Cin'][Cout'] weight IS that tensor (Cin' = Cout), and vice
        # versa: same memory, the other interpretation, W_i negated (idv_pack_cconv_adjoint does the same)
        call("idv_pack_cconv_gauss", p(w_re), p(w_im), p(None), p(None), p(None), i(cout), i(cin_total), i(cin_used),
             i(1 if transposed else 0), i(1), p(wfrag), p(epi), stream_ptr())
        return GaussPack(wfrag, epi, 0, *_pack_wino_tw(w_re, w_im, cout, cin_total, cin_used, transposed, 1))
    w_re, w_im = w_re.contiguous(), w_im.contiguous()
    call("idv_pack_cconv_gauss", p(w_re), p(w_im), p(b_re.contiguous()), p(b_im.contiguous()), p(fold),
         i(cout), i(cin_total), i(cin_used), i(1 if transposed else 0), i(0), p(wfrag), p(epi), stream_ptr())
    return GaussPack(wfrag, epi, 1 if fold is not None else 0, *_pack_wino_tw(w_re, w_im, cout, cin_total, cin_used, transposed, 0))


# fp32 convs / transposed convs with Winograd-transformed frequency taps on top of the three-product form (csrc/cgemm_wino.hip):
# 7 instead of 10 real products per input channel and pair of rows.  IDV_WINO=0 (or ops.WINO = False) keeps cgemm_gauss.
WINO = os.environ.get("IDV_WINO", "1") != "0"
WINO_CFG = 4000000               # LAUNCH_LOG ids: WINO_CFG + (1000 if transposed) + idv_cconv_wino_config


def _pack_wino(w_re, w_im, cout: int, cin_total: int, cin_used: int, transposed: bool, conj: int):
    """Winograd-transformed Gauss planes of an operator (transposed = the OPERATOR's mode: a ComplexConvTranspose2d or the adjoint
    of a ComplexConv2d; a ComplexConv2d or the adjoint of a transposed one), flags exactly as idv_pack_cconv_gauss gets them."""
    if not WINO:
        return None
    n = int(_ll_fn("idv_cconv_wino_wfrag_floats")(i(1 if transposed else 0), i(cout), i(cin_used)))
    wf = torch.empty(n, dtype=torch.float32, device=w_re.device)
    call("idv_pack_cconv_wino", p(w_re), p(w_im), i(cout), i(cin_total), i(cin_used), i(1 if transposed else 0), i(conj), p(wf),
         stream_ptr())
    return wf


# ... and, for the transposed operators, with the TIME taps in Winograd form too (csrc/cgemm_tw.hip): 3 instead of 4 products per pair
# of output columns.  IDV_TW=0 (or ops.TW = False before the weights
# are packed) keeps cgemm_wino.  Measured at B = 64: dec0-3 38.9 -> 35.2 ms, headline 823 -> 864 utt/s on the same box.
TW = os.environ.get("IDV_TW", "1") != "0"
TW_CONV = os.environ.get("IDV_TW_CONV", "1") != "0"      # the conv form (csrc/cgemm_tw2.hip); 0: cgemm_wino's conv form
TW_CFG = 5000000                 # LAUNCH_LOG ids of a launch on the time-Winograd kernels: TW_CFG (+ 1: taps (x[t-1], x[t]); + 2: the conv form)
# Two co tiles per workgroup in the time-Winograd kernels (one staging of the raw rows for both; bit-identical outputs).  A bit mask:
# 1 = transposed form, even-row phase; 2 = transposed form, odd-row phase; 4 = conv form; 0 = one co tile per workgroup everywhere.
# None: the library's value (IDV_TW_PAIR in the environment, default all).  Assigning it takes effect at the next launch.
TW_PAIR = None
_tw_pair_lib = None              # the library's own value, read before the first assignment reaches it
_tw_pair_pushed = None


def _sync_tw_pair():
    global _tw_pair_lib, _tw_pair_pushed
    if TW_PAIR == _tw_pair_pushed:
        return
    if _tw_pair_lib is None:
        _tw_pair_lib = int(L.lib().idv_tw_pair(-1))
    L.lib().idv_tw_pair(_tw_pair_lib if TW_PAIR is None else int(TW_PAIR))
    _tw_pair_pushed = TW_PAIR


def tw_pair_launches(reset: bool = False) -> int:
    """Launches of the paired time-Winograd kernels by this process so far."""
    return int(L.lib().idv_tw_pair_launches(1 if reset else 0))


def _pack_wino_tw(w_re, w_im, cout: int, cin_total: int, cin_used: int, transposed: bool, conj: int):
    """-> (wino fragments | None, time-Winograd fragments | None): the `wino` and `tw` fields of a GaussPack (the time-Winograd fragments
    are those of the OPERATOR's form: csrc/cgemm_tw.hip for a transposed conv, csrc/cgemm_tw2.hip for a conv)."""
    wf = _pack_wino(w_re, w_im, cout, cin_total, cin_used, transposed, conj)
    if wf is None or not TW or (not transposed and not TW_CONV):
        return wf, None
    if transposed:
        tw = torch.empty(int(_ll_fn("idv_cconv_tw_wfrag_floats")(i(cout), i(cin_used))), dtype=torch.float32, device=w_re.device)
        call("idv_pack_cconv_tw", p(wf), i(cout), i(cin_used), p(tw), stream_ptr())
    else:
        tw = torch.empty(int(_ll_fn("idv_cconv_tw2_wfrag_floats")(i(cout), i(cin_used))), dtype=torch.float32, device=w_re.device)
        call("idv_pack_cconv_tw2", p(wf), i(cout), i(cin_used), p(tw), stream_ptr())
    return wf, tw


def _tw2_ok(gauss, x: Planar, c1: int, cout: int) -> bool:
    return (gauss is not None and TW and TW_CONV and WINO and c1 == 0 and gauss.tw is not None and x.Jp % 4 == 0
            and bool(L.lib().idv_cconv_tw2_supported(i(x.C), i(cout), i(x.F))))


def _tw_ok(gauss, x: Planar, c1: int, cout: int, skip_jp: Optional[int]) -> bool:
    return (gauss is not None and TW and WINO and gauss.tw is not None and x.Jp % 4 == 0
            and (skip_jp is None or skip_jp == x.Jp) and bool(L.lib().idv_cconv_tw_supported(i(x.C), i(c1), i(cout), i(x.F))))


def _wino_ok(gauss, transposed: bool, x: Planar, c1: int, cout: int, skip_jp: Optional[int]) -> bool:
    return (gauss is not None and WINO and gauss.wino is not None and x.Jp % 4 == 0
            and (skip_jp is None or skip_jp == x.Jp)
            and bool(L.lib().idv_cconv_wino_supported(i(1 if transposed else 0), i(x.C), i(c1), i(cout), i(x.F))))


def pack_cconv_gauss_skip_part(w_re, w_im, c0: int):
    """Gauss operands of the SKIP half of a transposed conv [Cin][Cout][5][2] (input channels c0 .. Cin), no bias, no fold:
    the once-per-utterance addend of the repeated-skip decoder (see cconv2d(addend=...))."""
    wr, wi = w_re[c0:].contiguous(), w_im[c0:].contiguous()
    cout, cin, _ = _conv_channels(wr, None, True)
    lib = L.lib()
    wfrag = torch.empty(int(lib.idv_cconv_gauss_wfrag_floats(i(cout), i(cin))), dtype=torch.float32, device=wr.device)
    epi = torch.empty(int(lib.idv_cconv_gauss_epi_rows(i(cout))) * 8, dtype=torch.float32, device=wr.device)
    call("idv_pack_cconv_gauss", p(wr), p(wi), p(None), p(None), p(None), i(cout), i(cin), i(cin), i(1), i(0), p(wfrag), p(epi),
         stream_ptr())
    return GaussPack(wfrag, epi, 0, *_pack_wino_tw(wr, wi, cout, cin, cin, True, 0))


def bf16_supported(transposed: bool, c0: int, c1: int, skip_div: int, cout: int) -> bool:
    return bool(L.lib().idv_cconv_bf16_supported(i(1 if transposed else 0), i(c0), i(c1), i(skip_div), i(cout)))


def pack_cconv_bf16(w_re, w_im, fold, cin_used: Optional[int] = None, transposed=False):
    """-> split-bf16 weight fragments (uint8 tensor) for idv_cconv2d_bf16x3_fwd."""
    cout, cin_total, cin_used = _conv_channels(w_re, cin_used, transposed)
    nbytes = L.lib().idv_cconv_bf16_wfrag_bytes(i(cout), i(cin_used))
    wfrag = torch.empty(int(nbytes), dtype=torch.uint8, device=w_re.device)
    call("idv_pack_cconv_bf16", p(w_re.contiguous()), p(w_im.contiguous()), p(fold), i(cout), i(cin_total), i(cin_used),
         i(1 if transposed else 0), p(wfrag), stream_ptr())
    return wfrag


def pack_ctconv_c1(w_re, w_im, fold, cin_used: Optional[int] = None):
    """Split-bf16 fragments for the Cout = 1 transposed conv (idv_ctconv_c1_bf16x3_fwd)."""
    _, cin_total, cin_used = _conv_channels(w_re, cin_used, True)
    wfrag = torch.empty(int(L.lib().idv_ctconv_c1_wfrag_bytes(i(cin_used))), dtype=torch.uint8, device=w_re.device)
    call("idv_pack_ctconv_c1_bf16", p(w_re.contiguous()), p(w_im.contiguous()), p(fold), i(cin_total), i(cin_used), p(wfrag),
         stream_ptr())
    return wfrag


def ctconv_c1(x, wfrag_c1, bias, *, slope=None, skip=None) -> Planar:
    """Causal transposed conv with one output channel on the split-bf16 path; x / skip both Planar or both Image."""
    out = Planar.empty(1, 2 * x.F - 1, x.B, x.T, x.Tp, x.buf.device)
    c1 = skip.C if skip is not None else 0
    timer = _launch_timer()
    if isinstance(x, Image):
        if skip is not None and not isinstance(skip, Image):
            raise RuntimeError("ctconv_c1: x and skip must have the same format")
        call("idv_ctconv_c1_img_fwd", x.ptr(), ll(x.lo_slots), i(x.C), skip.ptr() if skip is not None else p(None),
             ll(skip.lo_slots if skip is not None else 0), i(c1), p(wfrag_c1), p(bias), p(slope), out.ptr(), i(x.F), i(x.B),
             i(x.Tp), i(x.Jp), i(x.T), stream_ptr())
    else:
        call("idv_ctconv_c1_bf16x3_fwd", x.ptr(), i(x.C), skip.ptr() if skip is not None else p(None), i(c1),
             i(skip.Jp if skip is not None else 0), p(wfrag_c1), p(bias), p(slope), out.ptr(), i(x.F), i(x.B), i(x.Tp), i(x.Jp),
             i(x.T), stream_ptr())
    if timer is not None:
        _launch_logged(timer, -98 if isinstance(x, Image) else -99, 4 * (x.C + c1) * 10 * x.B * x.T * x.F)
    return out


def pack_pw(w, bias):
    M, K = w.shape
    mt = mtiles_alloc(M)
    ks = (K + 7) // 8 * 4
    wfrag = torch.empty(mt * ks * 64, dtype=torch.float32, device=w.device)
    bout = torch.empty(mt * 32, dtype=torch.float32, device=w.device)
    call("idv_pack_pw", p(w.contiguous()), p(None if bias is None else bias.contiguous()), i(M), i(K), p(wfrag),
         p(bout), stream_ptr())
    return wfrag, bout


# ----------------------------------------------------------------------------- forward ops
# When set to a list, every cconv2d launch appends (config id, algorithmic MACs, start event, end event);
# bench.py uses it to time the dominant kernel with events on the launching stream.
LAUNCH_LOG = None


def _launch_timer():
    """Start of the timed span of one LAUNCH_LOG entry: its (start, end) events, the start recorded on the current stream; None (and
    nothing created) when launches are not logged."""
    if LAUNCH_LOG is None:
        return None
    timer = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    timer[0].record()
    return timer


def _launch_logged(timer, cfg: int, macs: int):
    """End of the span `timer` started: LAUNCH_LOG gets (config id, algorithmic MACs, start event, end event)."""
    timer[1].record()
    LAUNCH_LOG.append((cfg, macs, timer[0], timer[1]))


def _conv_macs(cin: int, cout: int, x, transposed: bool, Fout: int) -> int:
    """Algorithmic MACs of a complex conv: 4 real convolutions of the reference, kernel 5x2, per kept output position
    (transposed: per INPUT position, each input feeds 5x2 taps)."""
    return 4 * cin * cout * 10 * x.B * x.T * (x.F if transposed else Fout)


def _conv_geometry(F: int, T: int, transposed: bool, causal: bool, adjoint: bool = False):
    """-> (Fout, t_out, tshift) of a conv / transposed conv over F rows and T frames.  tshift -1: the time taps read (x[t-1], x[t]);
    0: (x[t], x[t+1]).  adjoint: the operator is the data gradient of a block; of a causal one it has the time taps reversed (tshift 0)
    and keeps all T frames (x[T] is the next utterance's zero guard column), of a non-causal one it is the operator's own form."""
    Fout = 2 * F - 1 if transposed else (F - 1) // 2 + 1
    t_out = T if causal else (T + 1 if transposed else T - 1)
    tshift = -1 if (causal or transposed) else 0
    return Fout, t_out, 0 if (adjoint and causal) else tshift


# Eval-mode sub-batch pipelining (model/pvae_module.py DCCRN_.forward): number of HIP streams a batch is split over.
# Concurrent queues are only safe because the library is built without packed-fp32 VALU code (__graft_entry__.build,
# -fno-slp-vectorize): on MI355X v_pk_fma_f32 / v_pk_mul_f32 results of one kernel came out wrong in 16-lane slices
# while an MFMA-saturating kernel of another stream shared its SIMDs.
STREAM_SPLIT = int(os.environ.get("IDV_STREAM_SPLIT", "1"))     # opt-in: 2 = sub-batch pipelining
CONCURRENT = os.environ.get("IDV_CONCURRENT", "0") != "0"      # opt-in: ops.concurrent really uses several streams
STREAM_STAGGER = os.environ.get("IDV_STREAM_STAGGER", "1") != "0"   # part k+1 starts when part k reaches its LSTM
STREAM_STAGGER_BELOW = 1 << 30                   # parts below this size are staggered; measured +6 / +4 / +2 % at B = 64 / 96 / 128
STREAM_SPLIT_MIN_BATCH = 16                      # per-stream utterances below which launch overhead dominates
_SIDE_STREAMS = {}


def stream_split(batch: int) -> int:
    n = max(1, STREAM_SPLIT)
    while n > 1 and batch < n * STREAM_SPLIT_MIN_BATCH:
        n -= 1
    return n


def side_streams(n: int, device):
    key = (torch.device(device).index or 0)
    pool = _SIDE_STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def on_side_stream(device) -> bool:
    """True while the current stream of `device` is one of side_streams(): inside a part of a split batch."""
    pool = _SIDE_STREAMS.get(torch.device(device).index or 0)
    return bool(pool) and any(torch.cuda.current_stream(device) == s for s in pool)


def repeat_batch(x: Planar, n: int) -> Planar:
    """Each utterance n times in a row (`skip.repeat_interleave(n, 0)`, reference pvae_module.py:2563-2567) as a new
    planar buffer, so the repeated-skip decoder can use the kernels that take x1_div == 1 sources (bf16x3 / images)."""
    out = Planar.empty(x.C, x.F, x.B * n, x.T, x.Tp, x.buf.device)
    dst = torch.as_strided(out.buf, (2, x.C, x.F, x.B, n, x.Tp),
                           (x.C * x.F * out.Jp, x.F * out.Jp, out.Jp, n * x.Tp, x.Tp, 1), SLACK)
    dst.copy_(x.planes().unsqueeze(4).expand(2, x.C, x.F, x.B, n, x.Tp))      # planes(): [2, C, F, B, Tp]
    return out


def concurrent(fns, device=None):
    """Run independent callables (e.g. the frozen clean / noise encoders and the noisy encoder of the NSVAE step) on
    separate HIP streams and join: their latency-bound phases (the per-step recurrences) overlap.  Results may be
    used on the current stream afterwards; they return to their stream's pool, whose next use through this function
    starts behind everything enqueued on the current stream until then."""
    if not CONCURRENT:
        return [fn() for fn in fns]
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    main = torch.cuda.current_stream(device)
    streams = side_streams(len(fns), device)
    ready = torch.cuda.Event()
    ready.record(main)
    outs = []
    for fn, st in zip(fns, streams):
        st.wait_event(ready)
        with torch.cuda.stream(st):
            outs.append(fn())
    for st in streams:
        main.wait_stream(st)
    hand_over(outs, main)
    return outs


def hand_over(obj, stream):
    """Tell the caching allocator that `stream` reads every tensor reachable from `obj` (nested tuples / lists, the planar
    buffer a reference-shaped view carries as `_idv`): blocks that came from another stream's pool are then not handed
    out again before `stream` has passed the point where they are released.  Explicit cross-stream ownership instead of an
    argument about what the other stream does next."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            obj.record_stream(stream)
        pl = getattr(obj, "_idv", None)
        if pl is not None and isinstance(getattr(pl, "buf", None), torch.Tensor) and pl.buf.is_cuda:
            pl.buf.record_stream(stream)
    elif isinstance(obj, (Planar, Image)):
        obj.buf.record_stream(stream)
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            hand_over(o, stream)


class CoopTimeout(RuntimeError):
    """A cooperative (spin-synchronised) recurrence ran into its spin bound: its outputs are NaN-poisoned."""


def coop_check(sync: bool = True, clear: bool = True) -> None:
    """Report a cooperative recurrence's time-out AT THE OPERATION THAT OWNS IT: call after the forward / step whose result is
    about to be used (inference.py's entry points, bench.py's timed region and smoke() do).  `sync` synchronises the current
    stream first -- the status word is written by the device when the kernel aborts.  Raises CoopTimeout and, with `clear`,
    acknowledges the fault so that the next cooperative launch runs again; without it every cooperative entry keeps refusing
    with status -3 (sticky, like a device error), csrc/coop.hpp."""
    if sync:
        torch.cuda.current_stream().synchronize()
    if L.lib().idv_coop_last_status(1 if clear else 0) != 0:
        raise CoopTimeout("a cooperative LSTM recurrence timed out on this device (a sibling workgroup never became resident, e.g. "
                          "a CU-masked or shared GPU): results computed since the last check are NaN-poisoned"
                          + ("" if clear else "; cooperative launches are refused until ops.coop_clear()"))


def coop_clear() -> bool:
    """Acknowledge a cooperative time-out without raising; True if there was one."""
    return L.lib().idv_coop_last_status(1) != 0


# Train-mode moment sums: the conv epilogues spread their atomic adds over this many replicas of the [Cout][5] sums
# (idv_cconv2d_fwd / idv_cconv2d_gauss_fwd stats_work); IDV_STATS_REP=1 keeps one set
STATS_REP = int(os.environ.get("IDV_STATS_REP", "32"))


def _stats_work(stats, cout: int):
    if stats is None or STATS_REP < 2:
        return None
    return torch.zeros(STATS_REP, cout, 5, dtype=torch.float64, device=stats.device)


def cconv2d(x: Planar, wfrag, bias, cout: int, *, transposed=False, causal=True, slope=None, skip: Optional[Planar] = None,
            skip_div: int = 1, stats: Optional[torch.Tensor] = None, out: Optional[Planar] = None,
            wfrag_bf16: Optional[torch.Tensor] = None, image: str = "", adjoint_time: bool = False, gauss=None,
            addend: Optional[Planar] = None, addend_div: int = 1):
    """(causal_)ComplexConv2d / (causal_)ComplexConvTranspose2d forward on planar activations.
    image="also" / "only": the exact-fp32 kernel additionally / only writes a split-bf16 image -> (Planar|None, Image)."""
    # adjoint_time: the transposed conv reading (x[t+1], x[t]); with conjugate-transposed weights the data gradient of the causal conv
    assert not adjoint_time or (transposed and causal)
    Fout, t_out, tshift = _conv_geometry(x.F, x.T, transposed, causal, adjoint_time)
    if out is None and image != "only":
        out = Planar.empty(cout, Fout, x.B, t_out, x.Tp, x.buf.device)
    c1 = skip.C if skip is not None else 0
    if image:
        assert stats is None and skip_div == 1 and wfrag_bf16 is None
        img = Image.empty(cout, Fout, x.B, t_out, x.Tp, x.buf.device)
        call("idv_cconv2d_fwd_img", x.ptr(), i(x.C), skip.ptr() if skip is not None else p(None), i(c1),
             i(skip.Jp if skip is not None else 0), p(wfrag), p(bias), p(slope), out.ptr() if out is not None else p(None),
             img.ptr(), ll(img.lo_off), i(1 if transposed else 0), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp),
             i(t_out), stream_ptr())
        return out, img
    timer = _launch_timer()
    if wfrag_bf16 is not None:
        swork = _stats_work(stats, cout)
        call("idv_cconv2d_bf16x3_fwd", x.ptr(), i(x.C), skip.ptr() if skip is not None else p(None), i(c1),
             i(skip.Jp if skip is not None else 0), i(skip_div), p(wfrag_bf16), p(bias), p(slope), out.ptr(), p(stats), p(swork),
             i(STATS_REP), i(1 if transposed else 0), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(t_out), stream_ptr())
        cfg = _bf16_cfg(transposed, cout, x.F) if timer is not None else None
    else:
        cfg = _cconv2d_fp32(x, out, wfrag, bias, gauss, cout, transposed=transposed, tshift=tshift, t_out=t_out,
                            has_fold=gauss.has_fold if gauss is not None else 0, stats_rep=STATS_REP, slope=slope, skip=skip,
                            skip_div=skip_div, stats=stats, addend=addend, addend_div=addend_div)
    if timer is not None:
        _launch_logged(timer, cfg, _conv_macs(x.C + c1, cout, x, transposed, Fout))
    return out


def _bf16_cfg(transposed: bool, cout: int, F: int) -> int:
    """LAUNCH_LOG id of a launch of idv_cconv2d_bf16x3_fwd."""
    return -(1000000 + L.lib().idv_cconv_bf16_config(i(1 if transposed else 0), i(cout), i(F)))


def _cconv2d_fp32(x: Planar, out: Planar, wfrag, bias, gauss: Optional[GaussPack], cout: int, *, transposed: bool, tshift: int,
                  t_out: int, has_fold: int, stats_rep: int, slope, skip: Optional[Planar], skip_div: int, stats,
                  addend: Optional[Planar], addend_div: int) -> Optional[int]:
    """The one launch of an exact-fp32 conv / transposed conv, forward or data gradient, on the first kernel of the ladder
    time-Winograd -> Winograd -> three products -> plain  that serves it (gauss None: the plain kernel on wfrag / bias).  has_fold and
    stats_rep are the caller's to say: the data gradient runs without the pack's fold and without moment sums.
    -> the LAUNCH_LOG id of the kernel taken (None when launches are not logged)."""
    log = LAUNCH_LOG is not None
    cfg = None
    c1 = skip.C if skip is not None else 0
    skip_jp = skip.Jp if skip is not None else None
    swork = _stats_work(stats, cout)
    if transposed and skip_div == 1 and _tw_ok(gauss, x, c1, cout, skip_jp):
        # Winograd-transformed frequency and time taps (csrc/cgemm_tw.hip)
        if log:
            cfg = TW_CFG + (1 if tshift else 0)
        _sync_tw_pair()
        call("idv_ctconv2d_tw_fwd", x.ptr(), i(x.C), skip.ptr() if skip is not None else p(None), i(c1), p(gauss.tw), p(gauss.epi),
             i(has_fold), p(slope), out.ptr(), p(stats), p(swork), i(stats_rep), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp),
             i(t_out), addend.ptr() if addend is not None else p(None), i(addend_div), i(addend.Jp if addend is not None else 0),
             stream_ptr())
    elif not transposed and addend is None and _tw2_ok(gauss, x, c1, cout):
        # conv: Winograd-transformed frequency and time taps (csrc/cgemm_tw2.hip)
        if log:
            cfg = TW_CFG + 2 + (1 if tshift else 0)
        _sync_tw_pair()
        call("idv_cconv2d_tw_fwd", x.ptr(), i(x.C), p(gauss.tw), p(gauss.epi), i(has_fold), p(slope), out.ptr(), p(stats), p(swork),
             i(stats_rep), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(t_out), stream_ptr())
    elif skip_div == 1 and _wino_ok(gauss, transposed, x, c1, cout, skip_jp):
        # Winograd-transformed frequency taps on top of the three products (csrc/cgemm_wino.hip)
        if log:
            cfg = WINO_CFG + (1000 if transposed else 0) + L.lib().idv_cconv_wino_config(i(1 if transposed else 0), i(x.C + c1), i(cout))
        call("idv_cconv2d_wino_fwd", x.ptr(), i(x.C), skip.ptr() if skip is not None else p(None), i(c1), p(gauss.wino), p(gauss.epi),
             i(has_fold), p(slope), out.ptr(), p(stats), p(swork), i(stats_rep), i(1 if transposed else 0), i(tshift), i(cout), i(x.F),
             i(x.B), i(x.Tp), i(x.Jp), i(t_out), addend.ptr() if addend is not None else p(None), i(addend_div),
             i(addend.Jp if addend is not None else 0), stream_ptr())
    elif gauss is not None:
        # three real products per complex product (csrc/cgemm_gauss.hip)
        if log:
            cfg = L.lib().idv_cconv_gauss_config(i(1 if transposed else 0), i(x.C + c1), i(cout), i(x.F))
        call("idv_cconv2d_gauss_fwd", x.ptr(), i(x.C), skip.ptr() if skip is not None else p(None), i(c1),
             i(skip.Jp if skip is not None else 0), i(skip_div), p(gauss.wfrag3), p(gauss.epi), i(has_fold), p(slope), out.ptr(),
             p(stats), p(swork), i(stats_rep), i(1 if transposed else 0), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(t_out),
             addend.ptr() if addend is not None else p(None), i(addend_div), i(addend.Jp if addend is not None else 0), stream_ptr())
    else:
        if log:
            cfg = L.lib().idv_cconv_config(i(1 if transposed else 0), i(x.C + c1), i(cout), i(x.F))
        call("idv_cconv2d_fwd", x.ptr(), i(x.C), skip.ptr() if skip is not None else p(None), i(c1),
             i(skip.Jp if skip is not None else 0), i(skip_div), p(wfrag), p(bias), p(slope), out.ptr(), p(stats), p(swork),
             i(stats_rep), i(1 if transposed else 0), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(t_out), stream_ptr())
    return cfg


def cconv2d_img(x, wfrag_bf16, bias, cout: int, *, transposed=False, causal=True, slope=None, skip=None,
                want_planar=False, want_image=True, adjoint=False):
    """Eval-mode conv / transposed conv on the split-bf16 path with image and/or planar sources (x and skip must share
    one format) -> (Planar or None, Image or None).  adjoint: the data-gradient form (time taps reversed, all T frames kept,
    see cconv_dgrad)."""
    src_img = isinstance(x, Image)
    if skip is not None and isinstance(skip, Image) != src_img:
        raise RuntimeError("cconv2d_img: x and skip must have the same format")
    assert causal or not adjoint
    Fout, t_out, tshift = _conv_geometry(x.F, x.T, transposed, causal, adjoint)
    dev = x.buf.device
    outp = Planar.empty(cout, Fout, x.B, t_out, x.Tp, dev) if want_planar else None
    outi = Image.empty(cout, Fout, x.B, t_out, x.Tp, dev) if want_image else None
    c1 = skip.C if skip is not None else 0
    timer = _launch_timer()
    call("idv_cconv2d_img_fwd", i(1 if src_img else 0), x.ptr(), ll(x.lo_slots if src_img else 0), i(x.C),
         skip.ptr() if skip is not None else p(None), ll(skip.lo_slots if (skip is not None and src_img) else 0), i(c1),
         p(wfrag_bf16), p(bias), p(slope), outp.ptr() if outp is not None else p(None),
         outi.ptr() if outi is not None else p(None), ll(outi.lo_off if outi is not None else 0),
         i(1 if transposed else 0), i(tshift), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(t_out), stream_ptr())
    if timer is not None:
        _launch_logged(timer, _img_cfg(src_img, transposed, x.C + c1, cout, x.F), _conv_macs(x.C + c1, cout, x, transposed, Fout))
    return outp, outi


def _img_cfg(src_img: bool, transposed: bool, cin: int, cout: int, F: int) -> int:
    """LAUNCH_LOG id of a launch of the split-image conv kernels."""
    return -(100000000 + L.lib().idv_cconv_img_config(i(1 if src_img else 0), i(1 if transposed else 0), i(cin), i(cout), i(F)))


def cconv2d_img_train(x: Image, wfrag_bf16, bias, cout: int, stats, *, transposed=False, skip: Optional[Image] = None) -> Planar:
    """Training forward of a causal conv block from split images: planar fp32 y + the batch-norm moments (`stats`)."""
    Fout, _, _ = _conv_geometry(x.F, x.T, transposed, True)
    out = Planar.empty(cout, Fout, x.B, x.T, x.Tp, x.buf.device)
    c1 = skip.C if skip is not None else 0
    timer = _launch_timer()
    swork = _stats_work(stats, cout)
    call("idv_cconv2d_img_train_fwd", x.ptr(), ll(x.lo_slots), i(x.C), skip.ptr() if skip is not None else p(None),
         ll(skip.lo_slots if skip is not None else 0), i(c1), p(wfrag_bf16), p(bias), out.ptr(), p(stats), p(swork), i(STATS_REP),
         i(1 if transposed else 0), i(cout), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(x.T), stream_ptr())
    if timer is not None:
        _launch_logged(timer, _img_cfg(True, transposed, x.C + c1, cout, x.F), _conv_macs(x.C + c1, cout, x, transposed, Fout))
    return out


def pw_gemm(x_ptr, K: int, wfrag, bias, M: int, B: int, Tp: int, Jp: int, t_valid: int, out_ptr, *, slope=None,
            swap=False, ldo=0):
    call("idv_pw_gemm", x_ptr, i(K), p(wfrag), p(bias), p(slope), out_ptr, i(M), i(B), i(Tp), i(Jp), i(t_valid),
         i(1 if swap else 0), i(ldo), stream_ptr())


class LstmPack(NamedTuple):
    """Packed weights of one layer of a ComplexLSTM (both parts)."""
    wih: torch.Tensor                # W_ih fragments for idv_pw_gemm
    bih: torch.Tensor                # b_ih + b_hh
    whh: torch.Tensor                # W_hh in the recurrence's fragment order
    wih16: Optional[torch.Tensor]    # split-bf16 W_ih (bf16x3 input projection) or None
    wih_hh: Optional[torch.Tensor]   # layer 1, H = 128: W_ih in the recurrence's fragment order (two-layer launch) or None


def pack_lstm(sd_get, H: int, K: int, layer: int, device) -> LstmPack:
    """sd_get(name) -> tensor for names like 'lstm_re.weight_ih_l0'."""
    g = lambda n: sd_get(n).contiguous()
    l = layer
    M = 8 * H
    mt = mtiles_alloc(M)
    ks = (K + 7) // 8 * 4
    wih = torch.empty(mt * ks * 64, dtype=torch.float32, device=device)
    bih = torch.empty(mt * 32, dtype=torch.float32, device=device)
    call("idv_pack_lstm_ih", p(g(f"lstm_re.weight_ih_l{l}")), p(g(f"lstm_re.bias_ih_l{l}")), p(g(f"lstm_re.bias_hh_l{l}")),
         p(g(f"lstm_im.weight_ih_l{l}")), p(g(f"lstm_im.bias_ih_l{l}")), p(g(f"lstm_im.bias_hh_l{l}")), i(H), i(K),
         p(wih), p(bih), stream_ptr())
    whh = torch.empty(4 * 4 * H * H, dtype=torch.float32, device=device)
    call("idv_pack_lstm_hh", p(g(f"lstm_re.weight_hh_l{l}")), p(g(f"lstm_im.weight_hh_l{l}")), i(H), p(whh), stream_ptr())
    wih16 = None
    if L.lib().idv_lstm_proj_bf16_supported(i(H), i(K)) and (layer == 0 or (4 * H) % 256 == 0):
        wih16 = torch.empty(int(L.lib().idv_lstm_ih_bf16_bytes(i(H), i(K))), dtype=torch.uint8, device=device)
        call("idv_pack_lstm_ih_bf16", p(g(f"lstm_re.weight_ih_l{l}")), p(g(f"lstm_im.weight_ih_l{l}")), i(H), i(K), p(wih16),
             stream_ptr())
    # layer 1 at H = 128: W_ih ([4H][H] like W_hh) in the recurrence's fragment order too, for the two-layer cooperative
    # launch of the fp32 evaluation (csrc/lstm_stack2_f32.hip)
    wih_hh = None
    if layer == 1 and K == H and H == 128:
        wih_hh = torch.empty(4 * 4 * H * H, dtype=torch.float32, device=device)
        call("idv_pack_lstm_hh", p(g(f"lstm_re.weight_ih_l{l}")), p(g(f"lstm_im.weight_ih_l{l}")), i(H), p(wih_hh), stream_ptr())
    return LstmPack(wih, bih, whh, wih16, wih_hh)


# bf16x3 mode, H = 384 / 768: one persistent cooperative launch per layer (csrc/lstm_pers.hip) instead of one launch per
# time step; IDV_LSTM_PERSISTENT=0 keeps the per-step kernels
LSTM_PERSISTENT = os.environ.get("IDV_LSTM_PERSISTENT", "1") != "0"
# fp32 evaluation, H = 128: both layers in one cooperative launch (csrc/lstm_stack2_f32.hip); 0 keeps one launch per layer
LSTM_STACK2 = os.environ.get("IDV_LSTM_STACK2", "1") != "0"


def clstm(x: Planar, packed0: LstmPack, packed1: LstmPack, H: int) -> Planar:
    """ComplexLSTM forward: x planar with C*F = K feature planes per part -> planar [2][H][Jp] (F = 1)."""
    K = x.C * x.F
    out = Planar.empty(H, 1, x.B, x.T, x.Tp, x.buf.device)
    nwork = L.lib().idv_clstm_work_floats(i(H), i(x.B), i(x.T), i(x.Jp))
    work = torch.empty(bucket(int(nwork)), dtype=torch.float32, device=x.buf.device)
    flags = 1 if PRECISION == "bf16x3" else 0
    if not LSTM_PERSISTENT:
        flags |= 8
    if on_side_stream(x.buf.device):
        # sub-batch pipelining: the other part's encoder runs on the CUs this part's recurrence leaves empty, so the layer-0
        # projection stays hoisted instead of taking them for its producer workgroups (csrc/lstm_stack2_f32.hip)
        flags |= 16
    if (flags & 1) and packed0.wih16 is not None:
        # layer-0 input projection on the bf16 MFMA: K-major split image of the 2K input planes, then G into `work`
        kimg = KImage.from_planes(x.ptr(), 2 * K, x.B * x.Tp, x.Jp, x.buf.device)
        call("idv_lstm_proj_bf16x3", kimg.ptr(), ll(kimg.lo_slots), i(K), p(packed0.wih16), p(packed0.bih), p(work), i(H), i(x.B),
             i(x.T), i(x.Tp), i(x.Jp), stream_ptr())
        flags |= 2
    call("idv_clstm_fwd2", x.ptr(), i(K), p(packed0.wih), p(packed0.bih), p(packed0.whh), p(packed1.wih), p(packed1.bih),
         p(packed1.whh), p(packed1.wih_hh if LSTM_STACK2 else None), i(H), i(x.B), i(x.T), i(x.Tp), i(x.Jp), p(work), out.ptr(),
         i(flags), p(packed1.wih16 if (flags & 1) else None), stream_ptr())
    return out


def cdense(x: Planar, packed_r, packed_i, M: int, C_out: int, F_out: int) -> Planar:
    """ComplexDense on a planar [2][K][Jp] activation -> planar [2][C_out][F_out][Jp] (M = C_out*F_out)."""
    K = x.C * x.F
    out = Planar.empty(C_out, F_out, x.B, x.T, x.Tp, x.buf.device)
    if PRECISION == "bf16x3" and K % 64 == 0 and len(packed_r) > 2 and packed_r[2] is not None:
        kimg = KImage.from_planes(x.ptr(), 2 * K, x.B * x.Tp, x.Jp, x.buf.device)
        for ri, pk in enumerate((packed_r, packed_i)):
            pw_bf16x3(kimg, ri * K // 8, K, pk[2], pk[1], M, x.B, x.Tp, x.T, out.ptr(ri * C_out))
        return out
    for ri, pk in enumerate((packed_r, packed_i)):
        pw_gemm(x.ptr(ri * x.C), K, pk[0], pk[1], M, x.B, x.Tp, x.Jp, x.T, out.ptr(ri * C_out))
    return out


class DftPlan:
    """Windowed DFT / inverse DFT matrices for one (n_fft, win, hop, T), packed for idv_pw_gemm."""

    def __init__(self, n_fft, win, hop, T, device):
        self.n_fft, self.win, self.hop, self.T = n_fft, win, hop, T
        self.F = n_fft // 2 + 1
        F = self.F
        w_fwd = torch.empty(2 * F, win, dtype=torch.float32, device=device)
        w_inv = torch.empty(win, 2 * F, dtype=torch.float32, device=device)
        self.env_inv = torch.empty(n_fft + hop * (T - 1), dtype=torch.float32, device=device)
        call("idv_make_dft", i(n_fft), i(win), i(hop), i(T), p(w_fwd), p(w_inv), p(self.env_inv), stream_ptr())
        self.fwd = pack_pw(w_fwd, None)
        self.inv = pack_pw(w_inv, None)
        self.fwd16 = pack_pw_bf16(w_fwd)          # split-bf16 fragments of the same matrices (bf16x3 mode)
        self.inv16 = pack_pw_bf16(w_inv)
        self._w_fwd, self._w_inv = w_fwd, w_inv
        self._fwd_T = self._inv_T = None

    def fwd_T(self):
        """Packed transposed DFT matrix [win][2F]: the adjoint (signal gradient) of the STFT contraction."""
        if self._fwd_T is None:
            self._fwd_T = pack_pw(self._w_fwd.t().contiguous(), None)
        return self._fwd_T

    def inv_T(self):
        """Packed transposed inverse-DFT matrix [2F][win]: the adjoint (spectrum gradient) of the ISTFT contraction."""
        if self._inv_T is None:
            self._inv_T = pack_pw(self._w_inv.t().contiguous(), None)
        return self._inv_T


def check_lengths(lengths, B: int, L: int, n_fft: Optional[int]) -> list:
    """The guards on per-utterance sample counts (host only, no device use) -> list of ints.  ``lengths``: a python sequence
    or a CPU integer tensor with one entry per row of the padded [B, L] batch, each n_fft/2 < length <= L (n_fft None: a
    signal that is not framed, 0 < length <= L)."""
    if isinstance(lengths, Lengths):
        lengths = lengths.host
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda:
            raise ValueError("lengths must be a python sequence or a CPU integer tensor: they size the batch on the host, and "
                             "a GPU tensor would have to be fetched with a synchronisation")
        if lengths.dim() != 1 or lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
            raise ValueError("lengths must be a 1-D integer tensor")
        lengths = lengths.tolist()
    elif isinstance(lengths, (str, bytes)) or not isinstance(lengths, Sequence):
        raise ValueError("lengths must be a python sequence or a CPU integer tensor")
    if any(isinstance(v, bool) or not isinstance(v, int) for v in lengths):
        raise ValueError("lengths must be integers (sample counts)")
    if len(lengths) != B:
        raise ValueError(f"{len(lengths)} lengths for a batch of {B} utterances")
    for b, v in enumerate(lengths):
        if n_fft is None and v <= 0:
            raise ValueError(f"lengths[{b}] = {v}: a length must be positive")
        if n_fft is not None and v <= n_fft // 2:
            raise ValueError(f"lengths[{b}] = {v}: torch.stft's reflect padding needs more than n_fft/2 = {n_fft // 2} samples")
        if v > L:
            raise ValueError(f"lengths[{b}] = {v} exceeds the {L} samples per row of the padded batch")
    return list(lengths)


class Lengths:
    """Sample counts of a batch of utterances of different lengths: ``host`` (list of ints, sizes the launch) and ``dev``
    (int32 on the device, read by idv_stft_frames_ragged / idv_istft_ola_ragged / idv_sisdr_ragged)."""

    __slots__ = ("host", "dev")

    def __init__(self, host, device, dev=None):
        self.host = list(host)
        self.dev = torch.tensor(self.host, dtype=torch.int32, device=device) if dev is None else dev

    def __len__(self):
        return len(self.host)

    def part(self, b0: int, b1: int) -> "Lengths":
        """Rows b0 .. b1-1 (a sub-batch of a stream split); shares the device array."""
        return Lengths(self.host[b0:b1], None, self.dev[b0:b1])

    def outputs(self, hop: int) -> "Lengths":
        """The lengths of the enhanced signals, hop * (length // hop)."""
        return Lengths([hop * (v // hop) for v in self.host], self.dev.device)


def _ragged_rows(x: torch.Tensor) -> torch.Tensor:
    """The padded batch as the ragged framing kernels take it: fp32 rows at any pitch (a column slice of a wider buffer is
    passed as it is), unit stride inside a row."""
    if x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.float().contiguous()
    return x


def stft(x: torch.Tensor, plan: DftPlan, Tp: Optional[int] = None, lengths=None) -> Planar:
    """STFT.forward: x [B, L] -> planar [2][1][F][Jp].  ``lengths`` (a :class:`Lengths`, a python sequence or a CPU integer
    tensor): row b holds lengths[b] samples and is mirrored at its own end; the frames past its 1 + lengths[b] // hop are
    zeros (whatever x holds there) and the returned spectrum carries the lengths."""
    if lengths is not None:
        return _stft_ragged(x, plan, Tp, lengths)
    B, Lx = x.shape
    T = 1 + Lx // plan.hop
    assert T == plan.T, "DftPlan built for another length"
    Tp = Tp or T + 1
    x = x.contiguous()
    if PRECISION == "bf16x3":
        Jp = Planar.jp_for(B, Tp)
        kimg = KImage((plan.win + 63) // 64 * 64, Jp, x.device)
        call("idv_stft_frames_kimage", p(x), i(B), i(Lx), i(plan.n_fft), i(plan.win), i(plan.hop), i(T), kimg.ptr(),
             ll(kimg.lo_off), i(Tp), i(Jp), stream_ptr())
        out = Planar.empty(1, plan.F, B, T, Tp, x.device)
        pw_bf16x3(kimg, 0, plan.win, plan.fwd16, None, 2 * plan.F, B, Tp, T, out.ptr())
        return out
    fr = Planar.empty(1, plan.win // 2, B, T, Tp, x.device)      # [win][Jp] scratch (2*C*F = win planes)
    assert plan.win % 2 == 0
    call("idv_stft_frames", p(x), i(B), i(Lx), i(plan.n_fft), i(plan.win), i(plan.hop), i(T), fr.ptr(), i(Tp), i(fr.Jp),
         stream_ptr())
    out = Planar.empty(1, plan.F, B, T, Tp, x.device)
    pw_gemm(fr.ptr(), plan.win, plan.fwd[0], plan.fwd[1], 2 * plan.F, B, Tp, fr.Jp, T, out.ptr())
    return out


def _stft_ragged(x: torch.Tensor, plan: DftPlan, Tp: Optional[int], lengths) -> Planar:
    B, Lx = x.shape
    T = 1 + Lx // plan.hop
    assert T == plan.T, "DftPlan built for another length"
    host = check_lengths(lengths, B, Lx, plan.n_fft)
    if not isinstance(lengths, Lengths):
        lengths = Lengths(host, x.device)
    Tp = Tp or T + 1
    x = _ragged_rows(x)
    assert plan.win % 2 == 0
    out = Planar.empty(1, plan.F, B, T, Tp, x.device)
    out.lengths = lengths
    if PRECISION == "bf16x3":
        kimg = KImage((plan.win + 63) // 64 * 64, out.Jp, x.device)
        call("idv_stft_frames_kimage_ragged", p(x), ll(x.stride(0)), p(lengths.dev), i(B), i(plan.n_fft), i(plan.win), i(plan.hop),
             i(T), kimg.ptr(), ll(kimg.lo_off), i(Tp), i(out.Jp), stream_ptr())
        pw_bf16x3(kimg, 0, plan.win, plan.fwd16, None, 2 * plan.F, B, Tp, T, out.ptr())
        return out
    fr = Planar.empty(1, plan.win // 2, B, T, Tp, x.device)      # [win][Jp] scratch (2*C*F = win planes)
    call("idv_stft_frames_ragged", p(x), ll(x.stride(0)), p(lengths.dev), i(B), i(plan.n_fft), i(plan.win), i(plan.hop), i(T),
         fr.ptr(), i(Tp), i(fr.Jp), stream_ptr())
    pw_gemm(fr.ptr(), plan.win, plan.fwd[0], plan.fwd[1], 2 * plan.F, B, Tp, fr.Jp, T, out.ptr())
    return out


def istft(spec: Planar, plan: DftPlan, lengths=None) -> torch.Tensor:
    """ISTFT.forward: planar [2][1][F][Jp] -> y [B, hop*(T-1)].  ``lengths`` (the input signals' sample counts, as for
    :func:`stft`): row b is the overlap-add of its own 1 + length // hop frames over their own envelope, hop * (length // hop)
    samples followed by zeros.  Fewer lengths than rows: each serves ``B // len(lengths)`` consecutive rows (the VAE decoders'
    num_samples rows per utterance)."""
    B, T = spec.B, spec.T
    if lengths is not None:
        nl = len(lengths)
        if nl < 1 or B % nl:
            raise ValueError(f"{nl} lengths for {B} rows: the row count must be a multiple of the number of lengths")
        if not isinstance(lengths, Lengths):
            lengths = Lengths(check_lengths(lengths, nl, plan.hop * T + plan.hop - 1, plan.n_fft), spec.buf.device)
        if max(lengths.host) // plan.hop + 1 > T:
            raise ValueError("a length needs more frames than the spectrum holds")
    fr = Planar.empty(1, plan.win // 2, B, T, spec.Tp, spec.buf.device)
    if PRECISION == "bf16x3":
        kimg = KImage.from_planes(spec.ptr(), 2 * plan.F, B * spec.Tp, spec.Jp, spec.buf.device, pad_to=64)
        pw_bf16x3(kimg, 0, 2 * plan.F, plan.inv16, None, plan.win, B, spec.Tp, T, fr.ptr())
    else:
        pw_gemm(spec.ptr(), 2 * plan.F, plan.inv[0], plan.inv[1], plan.win, B, spec.Tp, spec.Jp, T, fr.ptr())
    y = torch.empty(B, plan.hop * (T - 1), dtype=torch.float32, device=spec.buf.device)
    if lengths is not None:
        call("idv_istft_ola_ragged", fr.ptr(), p(lengths.dev), i(B // len(lengths)), i(B), i(plan.n_fft), i(plan.win), i(plan.hop),
             i(T), i(spec.Tp), i(fr.Jp), p(y), ll(y.stride(0)), stream_ptr())
        return y
    call("idv_istft_ola", fr.ptr(), p(plan.env_inv), i(B), i(plan.n_fft), i(plan.win), i(plan.hop), i(T), i(spec.Tp),
         i(fr.Jp), p(y), stream_ptr())
    return y


# ----------------------------------------------------------------------------- corpus preparation
RESAMPLE_MAX_M = 640           # max(up, down) after reduction: 8 / 11.025 / 22.05 / 24 / 32 / 44.1 / 48 / 96 kHz <-> 16 kHz all fit
RESAMPLE_MAX_LEN = ROWS_MAX_LEN
PAD_MODES = {"reflect": 0, "constant": 1}      # IDV_PAD_REFLECT / IDV_PAD_CONSTANT
_RESAMPLE_TAPS = {}            # (up, down, device) -> fp32 taps on the device


def resample_ratio(fs_in, fs_out):
    """(up, down) = (fs_out, fs_in) reduced by their gcd; the guards on the rates (host only, no device use)."""
    for name, v in (("fs_in", fs_in), ("fs_out", fs_out)):
        if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
            raise ValueError(f"{name} = {v!r}: a sampling rate must be a positive integer")
    import math
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    if max(up, down) > RESAMPLE_MAX_M:
        raise ValueError(f"{fs_in} -> {fs_out} Hz reduces to {up}/{down}: max(up, down) may not exceed {RESAMPLE_MAX_M}")
    return up, down


def resample_len(L: int, up: int, down: int) -> int:
    """ceil(L * up / down): the number of output samples of L input samples."""
    return -((-L * up) // down)


def resample_taps_host(up: int, down: int):
    """scipy.signal.resample_poly's default filter for the reduced ratio, in float64: 2 * half + 1 taps, half = 10 * max(up, down),
    kaiser(5.0) * sinc(t / m) / m normalised to sum 1."""
    import numpy as np
    m = max(up, down)
    half = 10 * m
    t = np.arange(-half, half + 1, dtype=np.float64)
    h = np.kaiser(2 * half + 1, 5.0) * np.sinc(t / m) / m
    return h / h.sum()


def resample_taps(up: int, down: int, device) -> torch.Tensor:
    """The taps as the kernel reads them, formed once per (up, down, device) and cached."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (up, down, device)
    if key not in _RESAMPLE_TAPS:
        _RESAMPLE_TAPS[key] = torch.from_numpy(resample_taps_host(up, down).astype("float32")).to(device)
    return _RESAMPLE_TAPS[key]


def resample(x: torch.Tensor, up: int, down: int, lengths: Optional[Lengths] = None) -> torch.Tensor:
    """idv_resample: x [B, L] -> y [B, ceil(L * up / down)] for a reduced (up, down) of :func:`resample_ratio`; with ``lengths`` row b
    holds ceil(lengths[b] * up / down) samples followed by zeros, and nothing at or past lengths[b] is read."""
    B, Lx = x.shape
    if Lx < 1 or Lx > RESAMPLE_MAX_LEN:
        raise ValueError(f"resample: rows of {Lx} samples; 1 .. 2^27 are supported")
    if B < 1 or B > ROWS_MAX_ROWS:
        raise ValueError(f"resample: a batch of {B} rows; 1 .. {ROWS_MAX_ROWS} are supported")
    n = resample_len(Lx, up, down)
    if n > 2 ** 31 - 1 - 256:
        raise ValueError(f"resample: {n} output samples per row are not supported")
    check_dev_f32(x, "x")
    x = _ragged_rows(x)
    taps = resample_taps(up, down, x.device)
    y = torch.empty(B, n, dtype=torch.float32, device=x.device)
    call("idv_resample", p(x), ll(x.stride(0)), p(None if lengths is None else lengths.dev), i(B), i(Lx), i(up), i(down), p(taps), p(y),
         ll(y.stride(0)), stream_ptr())
    return y


# ---- the stateful form of the resampler (csrc/stream_resample.hip)
SR_ROW_FIELDS = ("P0", "count", "n0", "m", "parity", "end", "idle")      # IDV_SR_ROW_* of include/idccrn_hip.h
SR_TAPS_MODES = {"auto": 0, "mem": 1, "lds": 2}                          # IDV_SR_TAPS_*


def stream_resample_hist(up: int, down: int) -> int:
    """H = floor(2 * half / up) + 1: the input samples a stream keeps from call to call (idv_stream_resample_hist)."""
    return 20 * max(up, down) // up + 1


def stream_resample_final(P: int, up: int, down: int) -> int:
    """n_final(P) = max(0, ceil((P * up - half) / down)): the outputs that are final after P input samples."""
    return max(0, -((10 * max(up, down) - P * up) // down))


def _stream_resample_hist(hist) -> tuple:
    """The guards on a resampler's history [2 parities, B, H] -> (B, H)."""
    check_dev_f32(hist, "hist")
    if hist.dtype != torch.float32 or hist.dim() != 3 or hist.shape[0] != 2 or not hist.is_contiguous():
        raise ValueError("stream_resample: hist must be a contiguous float32 tensor [2, B, H]")
    return int(hist.shape[1]), int(hist.shape[2])


def _stream_resample_x(x, B: int, n: int):
    """The new samples as the kernels read them: fp32 rows of n samples at any pitch -> (tensor or None, pitch)."""
    if n == 0:
        return None, 0
    check_dev_f32(x, "x")
    if x.dim() != 2 or x.shape[0] != B or x.shape[1] != n:
        raise ValueError(f"stream_resample: x must be [{B}, {n}], got {tuple(x.shape)}")
    x = _ragged_rows(x)
    return x, x.stride(0)


def stream_resample(hist: torch.Tensor, parity: int, x: Optional[torch.Tensor], n_new: int, P0: int, flush: bool, n0: int, m: int,
                    up: int, down: int, taps_mode: str = "auto") -> torch.Tensor:
    """idv_stream_resample: the B streams of ``hist`` [2, B, H] at position P0 take x [B, n_new] (None for n_new = 0) -> y [B, m], the
    outputs n0 .. n0 + m - 1; ``flush``: the signals end at P0 + n_new.  Half ``parity`` of hist is read and, unless the call
    flushes or brings nothing, half 1 - parity written."""
    B, H = _stream_resample_hist(hist)
    x, ldx = _stream_resample_x(x, B, n_new)
    taps = resample_taps(up, down, hist.device)
    y = torch.empty(B, m, dtype=torch.float32, device=hist.device)
    call("idv_stream_resample", p(hist), i(H), i(parity), p(x), ll(ldx), i(n_new), ll(P0), i(1 if flush else 0), ll(n0), i(m), i(B),
         i(up), i(down), p(taps), i(SR_TAPS_MODES[taps_mode]), p(y) if m else p(None), ll(m), stream_ptr())
    return y


def stream_resample_rows(hist: torch.Tensor, x: Optional[torch.Tensor], n_x: int, rows, ldy: int, up: int, down: int,
                         taps_mode: str = "auto") -> torch.Tensor:
    """idv_stream_resample_rows: ``rows`` is the device pointer of a table [B][SR_ROW_FIELDS] that idv_stream_resample_rows_check
    has passed -> y [B, ldy], row b's outputs followed by zeros."""
    B, H = _stream_resample_hist(hist)
    x, ldx = _stream_resample_x(x, B, n_x)
    taps = resample_taps(up, down, hist.device)
    y = torch.empty(B, ldy, dtype=torch.float32, device=hist.device)
    call("idv_stream_resample_rows", p(hist), i(H), p(x), ll(ldx), i(n_x), rows, i(B), i(up), i(down), p(taps),
         i(SR_TAPS_MODES[taps_mode]), p(y) if ldy else p(None), ll(ldy), stream_ptr())
    return y


def stft_frames_pad(x: torch.Tensor, lengths: Lengths, n_fft: int, win: int, hop: int, T: int, pad_mode: str) -> Planar:
    """idv_stft_frames_ragged_pad: the frames [win][Jp] (a Planar of win // 2 "channels") of a padded batch, T columns per row."""
    fr = Planar.empty(1, win // 2, x.shape[0], T, T + 1, x.device)
    call("idv_stft_frames_ragged_pad", p(x), ll(x.stride(0)), p(lengths.dev), i(x.shape[0]), i(n_fft), i(win), i(hop), i(T),
         i(PAD_MODES[pad_mode]), fr.ptr(), i(T + 1), i(fr.Jp), stream_ptr())
    return fr


# ----------------------------------------------------------------------------- silence trimming
TRIM_MAX_LEN = ROWS_MAX_LEN
TRIM_MAX_BLOCKS = 64           # frame_length / hop_length


def check_trim_args(top_db, frame_length, hop_length) -> float:
    """The guards on the trimming parameters (host only, no device use) -> top_db as a float."""
    import math
    if isinstance(top_db, bool) or not isinstance(top_db, (int, float)) or not math.isfinite(top_db) or top_db <= 0:
        raise ValueError(f"trim: top_db = {top_db!r}: a positive finite number of decibels is expected")
    for name, v in (("frame_length", frame_length), ("hop_length", hop_length)):
        if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
            raise ValueError(f"trim: {name} = {v!r}: a positive integer is expected")
    if hop_length > TRIM_MAX_LEN or hop_length % 4 or frame_length % (2 * hop_length) or frame_length // hop_length > TRIM_MAX_BLOCKS:
        raise ValueError(f"trim: frame_length = {frame_length}, hop_length = {hop_length}: hop_length must be a multiple of 4 and "
                         f"frame_length a multiple of 2 * hop_length, at most {TRIM_MAX_BLOCKS} * hop_length")
    return float(top_db)


def trim_bounds(x: torch.Tensor, top_db: float, frame_length: int, hop_length: int, lengths: Optional[Lengths] = None, power: bool = False):
    """idv_trim_bounds: x [B, L] -> int32 bounds [B, 2] on the device (start, end of the non-silent span of every row); with ``power``
    also the float64 frame powers [B, 1 + L // hop_length].  Nothing at or past lengths[b] is read."""
    B, Lx = x.shape
    if Lx < 1 or Lx > TRIM_MAX_LEN:
        raise ValueError(f"trim: rows of {Lx} samples; 1 .. 2^27 are supported")
    if B < 1 or B > ROWS_MAX_ROWS:
        raise ValueError(f"trim: a batch of {B} rows; 1 .. {ROWS_MAX_ROWS} are supported")
    check_dev_f32(x, "x")
    x = _ragged_rows(x)
    nbytes = int(_ll_fn("idv_trim_work_bytes")(i(B), i(Lx), i(hop_length)))
    if nbytes < 0:
        raise ValueError(f"trim: a batch of {B} rows of {Lx} samples at hop {hop_length} is not supported")
    work = _scratch(nbytes, x.device, "trim", torch.uint8)
    bounds = torch.empty(B, 2, dtype=torch.int32, device=x.device)
    P = torch.empty(B, 1 + Lx // hop_length, dtype=torch.float64, device=x.device) if power else None
    call("idv_trim_bounds", p(x), ll(x.stride(0)), p(None if lengths is None else lengths.dev), i(B), i(Lx), i(frame_length),
         i(hop_length), d(top_db), p(work), ll(work.numel()), p(bounds), p(P), ll(0 if P is None else P.stride(0)), stream_ptr())
    return (bounds, P) if power else bounds


def trim_gather(x: torch.Tensor, bounds: torch.Tensor, Lout: int) -> torch.Tensor:
    """idv_trim_gather: y [B, Lout] with y[b, :end_b - start_b] = x[b, start_b:end_b] and zeros behind; ``bounds`` int32 [B, 2] on the
    device, as :func:`trim_bounds` returns them."""
    B = x.shape[0]
    check_dev_f32(x, "x")
    x = _ragged_rows(x)
    y = torch.empty(B, Lout, dtype=torch.float32, device=x.device)
    if Lout > 0:
        call("idv_trim_gather", p(x), ll(x.stride(0)), p(bounds), i(B), i(Lout), p(y), ll(y.stride(0)), stream_ptr())
    return y


# ----------------------------------------------------------------------------- mixture synthesis
MIX_MAX_LEN = ROWS_MAX_LEN
MIX_WIN_FIELDS = 6             # IDV_MIX_WIN_FIELDS: max|c|, sum c^2, max|v|, sum v^2, max|y0|, sum y0^2 per window
MIX_ROW_FIELDS = 16            # IDV_MIX_ROW_FIELDS, the IDV_MIX_* indices of include/idccrn_hip.h:
MIX_FIELD = {"max_c": 0, "sum_c2": 1, "max_v": 2, "sum_v2": 3, "act_c2": 4, "act_v2": 5, "active": 6, "a": 7, "b": 8, "sum_y2": 9,
             "max_y": 10, "g_clean": 11, "g_noise": 12, "level_db": 13, "clipped": 14, "len": 15}


class MixRows(NamedTuple):
    """Where the kernels of csrc/mix.hip find their B rows: ``clean`` / ``noise`` are fp32 device tensors, either a padded batch
    ([B, L] / [B, Ln], ``*_off`` None) or a flat pool with ``*_off`` the int64 device table of every row's first sample; ``table`` is
    the int32 device tensor [3, B] of (lens, noise_lens, phase)."""
    clean: torch.Tensor
    clean_off: Optional[torch.Tensor]
    noise: torch.Tensor
    noise_off: Optional[torch.Tensor]
    table: torch.Tensor
    B: int
    L: int
    Ln: int

    def args(self):
        ldc = 0 if self.clean_off is not None else self.clean.stride(0)
        ldn = 0 if self.noise_off is not None else self.noise.stride(0)
        return (p(self.clean), p(self.clean_off), ll(ldc), p(self.noise), p(self.noise_off), ll(ldn), p(self.table[0]), p(self.table[1]),
                p(self.table[2]), i(self.B), i(self.L), i(self.Ln))


def mix_gains(rows: MixRows, par: torch.Tensor, segmental: bool, target_db: float, clip: float, win: int, thresh_db: float):
    """idv_mix_gains: ``par`` float64 [B, 2] = (snr_db, level_db) on the device -> (the float64 row records [B, MIX_ROW_FIELDS],
    the float64 window sums [B, ceil(L / win), MIX_WIN_FIELDS]).  The window sums are a view of the work buffer of this device and
    stream, which :func:`asm_activity` shares: the next call of either overwrites them."""
    check_dev_f32(rows.clean, "clean")
    check_dev_f32(rows.noise, "noise", rows.clean.device)
    nbytes = int(_ll_fn("idv_mix_work_bytes")(i(rows.B), i(rows.L), i(win)))
    if nbytes < 0:
        raise ValueError(f"mix: a batch of {rows.B} rows of {rows.L} samples in windows of {win} is not supported")
    work = _scratch(nbytes, rows.clean.device, "mix", torch.uint8)
    rec = torch.empty(rows.B, MIX_ROW_FIELDS, dtype=torch.float64, device=rows.clean.device)
    call("idv_mix_gains", *rows.args(), p(par), i(1 if segmental else 0), d(target_db), d(clip), i(win), d(thresh_db), p(work),
         ll(work.numel()), p(rec), stream_ptr())
    return rec, work[:nbytes].view(torch.float64).view(rows.B, -1, MIX_WIN_FIELDS)


def mix_write(rows: MixRows, rec: torch.Tensor):
    """idv_mix_write: -> (noisy, clean_out, noise_out), each fp32 [B, L] with zeros from a row's length on."""
    out = torch.empty(3, rows.B, rows.L, dtype=torch.float32, device=rows.clean.device)
    call("idv_mix_write", *rows.args(), p(rec), p(out[0]), p(out[1]), p(out[2]), ll(rows.L), stream_ptr())
    return out[0], out[1], out[2]


# ----------------------------------------------------------------------------- reverberation
REVERB_MAX_TAPS = 1 << 16      # taps per impulse response
REVERB_MAX_HIST = 65535        # samples in front of a row that its convolution may reach


def reverb_apply(x: torch.Tensor, x_off: Optional[torch.Tensor], h: torch.Tensor, h_off: Optional[torch.Tensor], table: torch.Tensor,
                 B: int, L: int, Kmax: int) -> torch.Tensor:
    """idv_reverb: every row convolved with its own impulse response -> fp32 [B, L], zeros from a row's length on.  ``x`` / ``h`` are
    fp32 device tensors, either a padded batch ([B, L] / [B, Kmax], ``*_off`` None) or a flat pool with ``*_off`` the int64 device
    table of every row's first sample; ``table`` is the int32 device tensor [3, B] of (lens, taps, hist)."""
    check_dev_f32(x, "x")
    check_dev_f32(h, "rir", x.device)
    y = torch.empty(B, L, dtype=torch.float32, device=x.device)
    ldx = 0 if x_off is not None else x.stride(0)
    ldh = 0 if h_off is not None else h.stride(0)
    call("idv_reverb", p(x), p(x_off), ll(ldx), p(h), p(h_off), ll(ldh), p(table[0]), p(table[1]), p(table[2]), i(B), i(L), i(Kmax),
         p(y), ll(L), stream_ptr())
    return y


# ----------------------------------------------------------------------------- image-source impulse responses
ISM_FIELDS = 17                # IDV_ISM_FIELDS, the IDV_ISM_* indices of include/idccrn_hip.h:
ISM_FIELD = {"lx": 0, "ly": 1, "lz": 2, "sx": 3, "sy": 4, "sz": 5, "rx": 6, "ry": 7, "rz": 8, "beta": 9, "fs": 15, "c": 16}
ISM_TILE = 64                  # samples of a tile: the work buffer holds one image count per tile


def ism_rir(geom: torch.Tensor, taps: torch.Tensor, max_order: Optional[torch.Tensor], B: int, Kmax: int,
            out: Optional[torch.Tensor] = None):
    """idv_ism_rir: ``geom`` float64 [B, ISM_FIELDS], ``taps`` (and ``max_order`` or None) int32 [B] on the device -> (fp32 [B, Kmax],
    row b its taps[b] samples and zeros behind them; int64 [B, ceil(Kmax / 64), 2]: per tile the images summed into it and those it
    owns, whose sum over a row is the row's image count).  ``out``: a
    float32 device tensor [B, >= Kmax] of any row pitch to write into; what lies past column Kmax stays.  The counts are a view of the
    work buffer of this device and stream: the next call overwrites them."""
    if not isinstance(geom, torch.Tensor) or not geom.is_cuda:
        raise L.IdvError("ism_rir: geom must be a CUDA (ROCm) tensor; the HIP hot path has no CPU fallback")
    nbytes = int(_ll_fn("idv_ism_work_bytes")(i(B), i(Kmax)))
    if nbytes < 0:
        raise ValueError(f"ism_rir: {B} rooms of {Kmax} taps are not supported")
    work = _scratch(nbytes // 8, geom.device, "ism", torch.int64)
    h = torch.empty(B, Kmax, dtype=torch.float32, device=geom.device) if out is None else out
    check_dev_f32(h, "out", geom.device)
    call("idv_ism_rir", p(geom), p(taps), p(max_order), i(B), i(Kmax), p(h), ll(h.stride(0)), p(work), ll(work.numel() * 8), stream_ptr())
    return h, work[:nbytes // 8].view(B, -1, 2)


def ism_peaks(h: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    """idv_ism_peaks: the index of max|h[b]| over the first taps[b] samples of every row, the first on ties -> int32 [B] on the device."""
    check_dev_f32(h, "h")
    peaks = torch.empty(h.shape[0], dtype=torch.int32, device=h.device)
    call("idv_ism_peaks", p(h), ll(h.stride(0)), p(taps), i(h.shape[0]), p(peaks), stream_ptr())
    return peaks


# ----------------------------------------------------------------------------- clip assembly
ASM_MAX_PIECES = 64            # IDV_ASM_MAX_PIECES: pieces per candidate row
ASM_MAX_TRIES = 16             # IDV_ASM_MAX_TRIES: candidates per row
ASM_MAX_ROWS = ROWS_MAX_ROWS   # candidate rows (B tries) of one call
ASM_WIN_FIELDS = 2             # IDV_ASM_WIN_FIELDS: max|x|, sum x^2 per window


class AsmTables(NamedTuple):
    """Where the kernels of csrc/assemble.hip find their candidate rows: ``pool`` is the flat fp32 device buffer the pieces point
    into, ``src`` (int64) / ``len`` / ``dst`` (int32) the device piece arrays, ``first`` / ``count`` (int32) index them per candidate
    row r = b tries + t."""
    pool: torch.Tensor
    src: torch.Tensor
    len: torch.Tensor
    dst: torch.Tensor
    first: torch.Tensor
    count: torch.Tensor
    B: int
    tries: int
    samples: int

    def args(self):
        return (p(self.pool), ll(self.pool.numel()), p(self.src), p(self.len), p(self.dst), p(self.first), p(self.count),
                i(self.src.numel()))


def asm_tables(pool: torch.Tensor, src, lens, dst, first, count, B: int, tries: int, samples: int) -> AsmTables:
    """The python lists of a candidate table -> :class:`AsmTables`, uploaded in ONE copy: the int64 offsets in front, the four int32
    arrays behind them in the same buffer."""
    P, R = len(src), len(first)
    small = np.zeros(2 * ((2 * P + 2 * R + 1) // 2), dtype=np.int32)
    small[:P], small[P:2 * P], small[2 * P:2 * P + R], small[2 * P + R:2 * P + 2 * R] = lens, dst, first, count
    host = np.concatenate([np.asarray(src, dtype=np.int64), small.view(np.int64)])
    dev = torch.from_numpy(host).to(pool.device, non_blocking=False)
    s32 = dev[P:].view(torch.int32)
    return AsmTables(pool, dev[:P], s32[:P], s32[P:2 * P], s32[2 * P:2 * P + R], s32[2 * P + R:2 * P + 2 * R], B, tries, samples)


def asm_activity(tab: AsmTables, rowlen: Optional[torch.Tensor], win: int, target_db: float, energy_thresh: float, min_activity: float):
    """idv_asm_activity -> dict of device tensors: ``rowstat`` float64 [R, 2] (max|x|, sum x^2), ``active`` / ``windows`` int32 [R],
    ``activity`` float64 [R], ``chosen`` / ``accepted`` int32 [B], ``window_stats`` float64 [R, ceil(samples / win), 2]: a view of the
    work buffer of this device and stream, which :func:`mix_gains` shares: the next call of either overwrites it."""
    check_dev_f32(tab.pool, "pool")
    R, dev = tab.B * tab.tries, tab.pool.device
    nbytes = int(_ll_fn("idv_asm_work_bytes")(i(R), i(tab.samples), i(win)))
    if nbytes < 0:
        raise ValueError(f"assemble: {R} candidate rows of {tab.samples} samples in windows of {win} are not supported")
    work = _scratch(nbytes, dev, "mix", torch.uint8)
    rowstat = torch.empty(R, 2, dtype=torch.float64, device=dev)
    act = torch.empty(R, dtype=torch.float64, device=dev)
    ints = torch.empty(2 * R + 2 * tab.B, dtype=torch.int32, device=dev)
    active, windows, chosen, accepted = ints[:R], ints[R:2 * R], ints[2 * R:2 * R + tab.B], ints[2 * R + tab.B:]
    call("idv_asm_activity", *tab.args(), p(rowlen), i(tab.B), i(tab.tries), i(tab.samples), i(win), d(target_db), d(energy_thresh),
         d(min_activity), p(work), ll(work.numel()), p(rowstat), p(active), p(windows), p(act), p(chosen), p(accepted), stream_ptr())
    return {"rowstat": rowstat, "active": active, "windows": windows, "activity": act, "chosen": chosen, "accepted": accepted,
            "window_stats": work[:nbytes].view(torch.float64).view(R, -1, ASM_WIN_FIELDS)}


def asm_write(tab: AsmTables, chosen: torch.Tensor) -> torch.Tensor:
    """idv_asm_write: -> fp32 [B, samples], row b the candidate ``chosen[b]`` (int32 on the device) of its ``tries``."""
    out = torch.empty(tab.B, tab.samples, dtype=torch.float32, device=tab.pool.device)
    call("idv_asm_write", *tab.args(), p(chosen), i(tab.B), i(tab.tries), i(tab.samples), p(out), ll(tab.samples), stream_ptr())
    return out


def mask_apply(mask: Planar, X: Planar, x_div: int = 1):
    """-> (pred planar, pred complex64 [B, F, T])."""
    B, F, T = mask.B, mask.F, mask.T
    pred = Planar.empty(1, F, B, T, mask.Tp, mask.buf.device)
    pc = torch.empty(B, F, T, 2, dtype=torch.float32, device=mask.buf.device)
    call("idv_mask_apply", mask.ptr(), X.ptr(), i(x_div), i(X.Jp), pred.ptr(), p(pc), i(F), i(B), i(T), i(mask.Tp),
         i(mask.Jp), stream_ptr())
    return pred, torch.view_as_complex(pc)


def msd(a: Planar, ca0: int, b: Planar, cb0: int, C: int) -> torch.Tensor:
    """One term of residual_loss (nsvae_loss.py:363-446): mean over [B, C, F, T, 2] of (a[:, ca0:ca0+C] - b[:, cb0:cb0+C])^2."""
    work = torch.empty(3, dtype=torch.float64, device=a.buf.device)
    out = torch.empty(1, dtype=torch.float32, device=a.buf.device)
    call("idv_msd", a.ptr(), i(a.C), i(ca0), i(a.Jp), b.ptr(), i(b.C), i(cb0), i(b.Jp), i(C), i(a.F), i(a.B), i(a.Tp), i(a.T),
         p(work), p(out), stream_ptr())
    return out[0]


def planar_to_complex(act: Planar) -> torch.Tensor:
    pc = torch.empty(act.B, act.F, act.T, 2, dtype=torch.float32, device=act.buf.device)
    call("idv_planar_to_complex", act.ptr(), p(pc), i(act.F), i(act.B), i(act.T), i(act.Tp), i(act.Jp), stream_ptr())
    return torch.view_as_complex(pc)


def cbn_train(act: Planar, stats: torch.Tensor, bn, slope, first_call: bool, momentum: float = 0.9):
    """Finish a train-mode conv block: stats (filled by cconv2d(stats=...)) -> batch moments, running
    buffers (in place, on the module's own buffers), then y = PReLU(Z x + s) in place on `act`."""
    C = act.C
    dev = act.buf.device
    moments = torch.empty(5, C, dtype=torch.float32, device=dev)
    fold = torch.empty(C, 6, dtype=torch.float32, device=dev)
    count = float(act.B) * act.F * act.T
    if BN_SYNC is not None:
        count = count * BN_SYNC(stats)
    call("idv_cbn_finalize", p(stats), d(count), p(bn.gamma_rr), p(bn.gamma_ri), p(bn.gamma_ii), p(bn.beta_r), p(bn.beta_i),
         i(C), i(1 if first_call else 0), f(momentum), p(bn.running_mean_real), p(bn.running_mean_imag), p(bn.Vrr), p(bn.Vri),
         p(bn.Vii), p(moments), p(fold), stream_ptr())
    call("idv_cbn_apply_prelu", act.ptr(), p(fold), p(slope), i(C), i(act.F), i(act.B), i(act.Tp), i(act.Jp), i(act.T),
         stream_ptr())
    return moments


def reparam(lat: Planar, off, zdim: int, eps_r, eps_i, ns: int) -> Planar:
    """reparameterization on a planar latent; off = (miu, log_sigma, delta) channel offsets."""
    B, T = lat.B, lat.T
    z = Planar.empty(zdim, 1, B * ns, T, lat.Tp, lat.buf.device)
    call("idv_reparam", lat.ptr(), i(lat.C), i(off[0]), i(off[1]), i(off[2]), i(zdim), p(eps_r.contiguous()),
         p(eps_i.contiguous()), i(ns), i(B), i(T), i(lat.Tp), i(lat.Jp), z.ptr(), i(z.Jp), stream_ptr())
    return z


# ----------------------------------------------------------------------------- losses
def check_dev_f32(t: torch.Tensor, name: str, device=None):
    """The kernels dereference raw pointers: a CPU tensor (e.g. straight out of a DataLoader) must fail here, not on the GPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.IdvError(f"{name}: expected a CUDA (ROCm) tensor, got {type(t).__name__} on "
                         f"{getattr(t, 'device', '?')}; the HIP hot path has no CPU fallback")
    if device is not None and t.device != torch.device(device):
        raise L.IdvError(f"{name}: on {t.device}, expected {device}")


def sisnr(source: torch.Tensor, est: torch.Tensor, src_div: int = 1) -> torch.Tensor:
    B, Ln = est.shape
    check_dev_f32(source, "source", est.device)
    if source.dtype != torch.float32 or est.dtype != torch.float32 or source.shape[-1] < Ln:
        raise L.IdvError("sisnr: float32 tensors with source length >= estimate length expected")
    assert source.stride(-1) == 1 and est.stride(-1) == 1
    work = torch.empty(3 * B, dtype=torch.float64, device=est.device)
    out = torch.empty(1, dtype=torch.float32, device=est.device)
    call("idv_sisnr", p(source), i(source.stride(0)), i(src_div), p(est), i(est.stride(0)), i(B), i(Ln), p(work), p(out),
         stream_ptr())
    return out[0]


def recon_loss(pred_c: torch.Tensor, ori: torch.Tensor, ori_div: int = 1):
    """pred_c: complex64 [B,F,T] (contiguous); ori: [B/ori_div, F, T, 2] real, any strides -> (cpx, mag)."""
    pr = torch.view_as_real(pred_c)
    assert pr.is_contiguous()
    check_dev_f32(ori, "ori_cpx_stft", pr.device)
    if ori.dtype != torch.float32:
        raise L.IdvError("recon_loss: float32 STFT expected")
    B, F, T, _ = pr.shape
    if tuple(ori.shape[1:]) != (F, T, 2):
        raise L.IdvError(f"recon_loss: STFT shape {tuple(ori.shape)} does not match the prediction {tuple(pr.shape)}")
    work = torch.empty(3, dtype=torch.float64, device=pr.device)
    out = torch.empty(2, dtype=torch.float32, device=pr.device)
    sb, sf, st, sr = ori.stride()
    call("idv_recon_loss", p(pr), p(ori), ll(sb), ll(sf), ll(st), ll(sr), i(ori_div), i(B), i(F), i(T), p(work), p(out),
         stream_ptr())
    return out[0], out[1]


def ckl(q1: Planar, off1, q2: Optional[Planar], off2, zdim: int, eps: float) -> torch.Tensor:
    work = torch.empty(3, dtype=torch.float64, device=q1.buf.device)
    out = torch.empty(1, dtype=torch.float32, device=q1.buf.device)
    o2 = off2 if q2 is not None else (0, 0, 0)
    call("idv_ckl", q1.ptr(), i(q1.C), i(q1.Jp), i(off1[0]), i(off1[1]), i(off1[2]),
         q2.ptr() if q2 is not None else p(None), i(q2.C if q2 is not None else 0), i(q2.Jp if q2 is not None else 0),
         i(o2[0]), i(o2[1]), i(o2[2]), i(zdim), f(eps), i(q1.B), i(q1.T), i(q1.Tp), p(work), p(out), stream_ptr())
    return out[0]


def mi_estimate(lat: Planar, off, z: Planar, zdim: int, ns: int, eps: float):
    """Minibatch mutual information (pretrain_pvaes_loss.py:129-159) -> (scalar, work); `work` holds d MI / d log q for mi_bwd."""
    lib = L.lib()
    if (z.C, z.B, z.T, z.Tp) != (zdim, lat.B * ns, lat.T, lat.Tp):
        raise ValueError(f"mutual_information: samples {(z.C, z.B, z.T)} do not belong to a posterior {(zdim, lat.B, lat.T)} x {ns}")
    work = torch.empty(int(lib.idv_mi_work_floats(i(lat.B), i(ns), i(lat.T), i(zdim))), dtype=torch.float32, device=lat.buf.device)
    acc = torch.empty(1, dtype=torch.float64, device=lat.buf.device)
    out = torch.empty(1, dtype=torch.float32, device=lat.buf.device)
    call("idv_mi_fwd", lat.ptr(), i(lat.C), i(lat.Jp), i(off[0]), i(off[1]), i(off[2]), z.ptr(), i(z.Jp), i(zdim), i(ns), i(lat.B),
         i(lat.T), i(lat.Tp), f(eps), p(work), p(acc), p(out), stream_ptr())
    return out[0], work


def mi_bwd(lat: Planar, off, z: Planar, zdim: int, ns: int, eps: float, work, gout, dlat: Optional[Planar], dz: Optional[Planar]):
    call("idv_mi_bwd", lat.ptr(), i(lat.C), i(lat.Jp), i(off[0]), i(off[1]), i(off[2]), z.ptr(), i(z.Jp), i(zdim), i(ns), i(lat.B),
         i(lat.T), i(lat.Tp), f(eps), p(work), p(gout), dlat.ptr() if dlat is not None else p(None),
         dz.ptr() if dz is not None else p(None), stream_ptr())


def miu_dist(q1: Planar, off1: int, q2: Planar, off2: int, zdim: int) -> torch.Tensor:
    work = torch.empty(3 * 2 * zdim, dtype=torch.float64, device=q1.buf.device)
    out = torch.empty(1, dtype=torch.float32, device=q1.buf.device)
    call("idv_miu_dist", q1.ptr(), i(q1.C), i(q1.Jp), i(off1), q2.ptr(), i(q2.C), i(q2.Jp), i(off2), i(zdim), i(q1.B), i(q1.T),
         i(q1.Tp), p(work), p(out), stream_ptr())
    return out[0]


# latent-space report (csrc/latent.hip; latent.py): q, q1, q2 are F == 1 planar latents, off the channel offsets (miu, log_sigma, delta),
# frames an int32 device tensor [B] or None, T the frames per row of the reference-shaped tensor.
def latent_row_stats(q: Planar, off, zdim: int, frames, B: int, T: int) -> torch.Tensor:
    out = torch.empty(B, 13, dtype=torch.float64, device=q.buf.device)
    work = torch.empty(B * zdim * 10, dtype=torch.float64, device=q.buf.device)
    call("idv_latent_row_stats", q.ptr(), i(q.C), i(q.Jp), i(q.Tp), i(off[0]), i(off[1]), i(off[2]), i(zdim), p(frames), i(B), i(T),
         p(work), p(out), stream_ptr())
    return out


def latent_pair_dist(q1: Planar, off1, q2: Planar, off2, zdim: int, frames, B: int, T: int) -> torch.Tensor:
    out = torch.empty(B, 3, dtype=torch.float64, device=q1.buf.device)
    work = torch.empty(B * zdim * 3, dtype=torch.float64, device=q1.buf.device)
    call("idv_latent_pair_dist", q1.ptr(), i(q1.C), i(q1.Jp), i(q1.Tp), i(off1[0]), i(off1[1]), i(off1[2]), q2.ptr(), i(q2.C), i(q2.Jp),
         i(q2.Tp), i(off2[0]), i(off2[1]), i(off2[2]), i(zdim), p(frames), i(B), i(T), p(work), p(out), stream_ptr())
    return out


def miu_moments_chunk() -> int:
    return int(L.lib().idv_miu_moments_chunk())


def miu_moments_update(q: Planar, off: int, zdim: int, frames, B: int, T: int, state: torch.Tensor):
    nbytes = int(_ll_fn("idv_miu_moments_work_bytes")(i(zdim), i(B), i(T)))
    if nbytes < 0:
        raise ValueError(f"miu moments: a batch of {B} rows of {T} frames at zdim = {zdim} is not supported")
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=state.device)
    call("idv_miu_moments_update", q.ptr(), i(q.C), i(q.Jp), i(q.Tp), i(off), i(zdim), p(frames), i(B), i(T), p(state), p(work),
         ll(nbytes), stream_ptr())


def miu_moments_merge(state: torch.Tensor, other: torch.Tensor, zdim: int):
    call("idv_miu_moments_merge", p(state), p(other), i(zdim), stream_ptr())


def latent_set_moments(x: torch.Tensor) -> torch.Tensor:
    """x [N, zdim, 2] contiguous fp32 -> double [2, 2 zdim]: the mean and the population variance of every column."""
    N, D = x.shape[0], x.shape[1] * 2
    mom = torch.empty(2, D, dtype=torch.float64, device=x.device)
    call("idv_latent_set_moments", p(x), i(N), i(D), p(mom), stream_ptr())
    return mom


def latent_silhouette(x1: torch.Tensor, x2: torch.Tensor, mom1: torch.Tensor, mom2: torch.Tensor) -> torch.Tensor:
    N1, N2, D = x1.shape[0], x2.shape[0], x1.shape[1] * 2
    work = torch.empty(N1 + N2, dtype=torch.float64, device=x1.device)
    out = torch.empty(6, dtype=torch.float64, device=x1.device)
    call("idv_latent_silhouette", p(x1), i(N1), p(x2), i(N2), i(D), p(mom1), p(mom2), p(work), p(out), stream_ptr())
    return out


def cbn_stats(act: Planar) -> torch.Tensor:
    """Moment sums [C][5] (double) of a planar activation, for a stand-alone train-mode batch norm."""
    stats = torch.zeros(act.C, 5, dtype=torch.float64, device=act.buf.device)
    call("idv_cbn_stats", act.ptr(), i(act.C), i(act.F), i(act.B), i(act.Tp), i(act.Jp), i(act.T), p(stats), stream_ptr())
    return stats


def cbn_apply(act: Planar, fold: torch.Tensor, slope=None):
    call("idv_cbn_apply_prelu", act.ptr(), p(fold), p(slope), i(act.C), i(act.F), i(act.B), i(act.Tp), i(act.Jp), i(act.T),
         stream_ptr())
    return act


# ----------------------------------------------------------------------------- backward (gradient) operators
# Thin wrappers over the idv_*_bwd entries; autograd.py strings them into torch.autograd.Function classes.


def _ll_fn(name):
    """A size query of the library by name; _lib.lib() has set its `long long` return type from the header's prototype."""
    return getattr(L.lib(), name)


def like(x: Planar, C: Optional[int] = None, F: Optional[int] = None, zero=False) -> Planar:
    return Planar.empty(x.C if C is None else C, x.F if F is None else F, x.B, x.T, x.Tp, x.buf.device, zero=zero)


def rewrap(buf: torch.Tensor, x: Planar, C: Optional[int] = None, F: Optional[int] = None) -> Planar:
    """A Planar with x's geometry over another flat buffer (e.g. an incoming gradient)."""
    return Planar(buf, x.C if C is None else C, x.F if F is None else F, x.B, x.T, x.Tp, x.Jp)


def pack_cconv_adjoint(w_re, w_im, cout: int, cin_total: int, cin_used: int, transposed: bool):
    """Fragments of the adjoint operator (data gradient), see idv_pack_cconv_adjoint; arguments describe the adjoint."""
    cck = L.lib().idv_cconv_cck(cin_used)
    ccp = (2 * cin_used + cck - 1) // cck * cck
    mt = mtiles_alloc(2 * cout)
    wfrag = torch.empty(mt * ccp * 5 * 64, dtype=torch.float32, device=w_re.device)
    bias = torch.empty(mt * 32, dtype=torch.float32, device=w_re.device)
    call("idv_pack_cconv_adjoint", p(w_re), p(w_im), i(cout), i(cin_total), i(cin_used), i(1 if transposed else 0), p(wfrag),
         p(bias), stream_ptr())
    return wfrag, bias


def pack_cconv_bf16_adjoint(w_re, w_im, cout: int, cin_total: int, cin_used: int, transposed: bool):
    """Split-bf16 fragments of the adjoint operator (bf16x3 training), see idv_pack_cconv_bf16_adjoint."""
    wfrag = torch.empty(int(L.lib().idv_cconv_bf16_wfrag_bytes(i(cout), i(cin_used))), dtype=torch.uint8, device=w_re.device)
    call("idv_pack_cconv_bf16_adjoint", p(w_re), p(w_im), i(cout), i(cin_total), i(cin_used), i(1 if transposed else 0),
         p(wfrag), stream_ptr())
    return wfrag


_ZBIAS = {}


def zero_bias(cout: int, device):
    key = (mtiles_alloc(2 * cout), str(device))
    if key not in _ZBIAS:
        _ZBIAS[key] = torch.zeros(key[0] * 32, dtype=torch.float32, device=device)
        torch.cuda.current_stream(device).synchronize()       # filled once; later users may sit on other streams
    return _ZBIAS[key]


def cconv_dgrad(dy: Planar, wfrag, bias, cout_adj: int, fwd_transposed: bool, causal: bool, wfrag_bf16=None, gauss=None) -> Planar:
    """Data gradient of a causal_complex_conv2d / causal_ComplexConvTranspose2d: the adjoint operator on idv_cconv2d_fwd
    (transposed conv reading (dy[t+1], dy[t]) / conv reading (dy[t], dy[t+1]); all T frames kept: column T+1 is the next
    utterance's zero guard column).  wfrag_bf16: run it on the split-bf16 kernel instead (bf16x3 training mode)."""
    adj_transposed = not fwd_transposed
    # causal blocks: time taps reversed (tshift 0), T frames in, T frames out.  Non-causal blocks (padding (2, 0)): the adjoint of
    # the conv (T -> T - 1 frames) is the transposed conv's own tap order (dx[t] = W0' dy[t] + W1' dy[t-1], tshift -1) on T frames;
    # the adjoint of the transposed conv (T -> T + 1) is the non-causal conv's (dx[t] = W0' dy[t] + W1' dy[t+1], tshift 0) on T frames
    Fout, t_out, tshift_adj = _conv_geometry(dy.F, dy.T, adj_transposed, causal, adjoint=True)
    if t_out + 1 > dy.Tp:
        raise RuntimeError("cconv_dgrad: the input of the block had more frames than the buffer's columns per utterance")
    out = Planar.empty(cout_adj, Fout, dy.B, t_out, dy.Tp, dy.buf.device)
    timer = _launch_timer()
    if wfrag_bf16 is not None:
        call("idv_cconv2d_bf16x3_fwd", dy.ptr(), i(dy.C), p(None), i(0), i(0), i(1), p(wfrag_bf16), p(bias), p(None), out.ptr(), p(None),
             p(None), i(0), i(1 if adj_transposed else 0), i(tshift_adj), i(cout_adj), i(dy.F), i(dy.B), i(dy.Tp), i(dy.Jp), i(t_out),
             stream_ptr())
        cfg = _bf16_cfg(adj_transposed, cout_adj, dy.F) if timer is not None else None
    else:
        # no skip, addend, slope or moment sums, and never the pack's fold: the adjoint of the contraction alone
        cfg = _cconv2d_fp32(dy, out, wfrag, bias, gauss, cout_adj, transposed=adj_transposed, tshift=tshift_adj, t_out=t_out, has_fold=0,
                            stats_rep=0, slope=None, skip=None, skip_div=1, stats=None, addend=None, addend_div=1)
    if timer is not None:
        _launch_logged(timer, cfg, _conv_macs(dy.C, cout_adj, dy, adj_transposed, Fout))
    return out


WGRAD_BF16_CFG = -96     # ... of wgrad_bf16_kernel + its unpack (bf16x3 training mode)
WGRAD_BF16 = os.environ.get("IDV_WGRAD_BF16", "1") != "0"
WGRAD_GAUSS_CFG = -95    # ... of the three-product fp32 weight gradient (wgrad_combine + wgrad_kernel x 3 products + unpack)
WGRAD_CFG = -97          # LAUNCH_LOG id of the conv weight-gradient kernel (wgrad_kernel<5, 2, 1, 1, 4, 1, 16, 2> + its unpack)


def cconv_wgrad(x: Planar, ci_off: int, dy: Planar, cout: int, cin_total: int, transposed: bool, causal: bool, dw_re, dw_im):
    tshift = -1 if (causal or transposed) else 0
    cs, cl = (x.C, cout) if transposed else (cout, x.C)
    # bf16x3 training mode: the wide layers (>= 32 planes on both sides) on the split-bf16 MFMA kernel; the one-channel
    # ends (a handful of planes against a 128 x 32 plane tile) stay on the exact-fp32 kernel
    bf16 = PRECISION == "bf16x3" and WGRAD_BF16 and 2 * cs >= 32 and 2 * cl >= 32
    # exact fp32 with three real contractions per complex channel pair (Gauss, csrc/wgrad.hip) where both sides are wide enough
    gauss = not bf16 and bool(L.lib().idv_cconv_wgrad_gauss_supported(i(cs), i(cl)))
    if gauss:
        n = int(_ll_fn("idv_cconv_wgrad_gauss_work_floats")(i(x.C), i(cout), i(1 if transposed else 0), i(x.F), i(x.B), i(x.Tp),
                                                            i(x.Jp), i(dy.Jp)))
    else:
        n = int(_ll_fn("idv_cconv_wgrad_bf16_work_floats" if bf16 else "idv_cconv_wgrad_work_floats")(i(cs), i(cl), i(x.B), i(x.Tp)))
    work = _scratch(n, x.buf.device)
    timer = _launch_timer()
    call("idv_cconv2d_bwd_weight_bf16x3" if bf16 else ("idv_cconv2d_bwd_weight_gauss" if gauss else "idv_cconv2d_bwd_weight"),
         x.ptr(), i(x.C), i(ci_off), dy.ptr(), i(cout), i(cin_total), i(1 if transposed else 0),
         i(tshift), i(x.F), i(x.B), i(x.Tp), i(x.Jp), i(dy.Jp), p(work), ll(work.numel()), p(dw_re), p(dw_im), stream_ptr())
    if timer is not None:
        _launch_logged(timer, WGRAD_BF16_CFG if bf16 else (WGRAD_GAUSS_CFG if gauss else WGRAD_CFG),
                       _conv_macs(x.C, cout, x, transposed, dy.F))


def cconv_bias_grad(dy: Planar):
    stats = cbn_stats(dy)
    db_re = torch.empty(dy.C, dtype=torch.float32, device=dy.buf.device)
    db_im = torch.empty_like(db_re)
    call("idv_cconv2d_bwd_bias", p(stats), i(dy.C), p(db_re), p(db_im), stream_ptr())
    return db_re, db_im


def train_image_ok(C: int) -> bool:
    """bf16x3 training: is an activation with C channels worth a split image (the image conv kernels take it as a source)?"""
    return PRECISION == "bf16x3" and IMAGE_TRAIN and C % 8 == 0 and 2 * C >= 64


def cbn_apply_to(y: Planar, fold, slope, want_image: bool = False):
    """-> z (Planar), or (z, Image of z) with want_image (one pass writes both)."""
    out = like(y)
    if want_image:
        img = Image.empty(y.C, y.F, y.B, y.T, y.Tp, y.buf.device)
        call("idv_cbn_apply_prelu_to_img", y.ptr(), p(fold), p(slope), i(y.C), i(y.F), i(y.B), i(y.Tp), i(y.Jp), i(y.T), out.ptr(),
             img.ptr(), ll(img.lo_off), stream_ptr())
        return out, img
    call("idv_cbn_apply_prelu_to", y.ptr(), p(fold), p(slope), i(y.C), i(y.F), i(y.B), i(y.Tp), i(y.Jp), i(y.T), out.ptr(),
         stream_ptr())
    return out


# Data-parallel training hook (parallel.py): when set, called on the per-channel moment sums of every train-mode
# ComplexBatchNormal (forward: [C][5] doubles, backward: [C][8] doubles) to all-reduce them over the ranks; returns
# the world size so the element count becomes the global one.
BN_SYNC = None


def cbn_bwd(dz: Planar, y: Planar, fold, moments, bn, slope, count: float, want_image: bool = False):
    """-> (dy, d gamma_rr, d gamma_ri, d gamma_ii, d beta_r, d beta_i, dslope[1]); want_image: dy is (Planar, Image)."""
    C, dev = y.C, y.buf.device
    sums = torch.empty(C, 8, dtype=torch.float64, device=dev)
    call("idv_cbn_bwd_reduce", dz.ptr(), y.ptr(), p(fold), p(slope), i(C), i(y.F), i(y.B), i(y.Tp), i(y.Jp), i(y.T), p(sums),
         stream_ptr())
    world = 1
    if BN_SYNC is not None:
        world = BN_SYNC(sums)
        count = count * world
    coef = torch.empty(C, 12, dtype=torch.float32, device=dev)
    g = [torch.empty(C, dtype=torch.float32, device=dev) for _ in range(5)]
    dslope = torch.zeros(1, dtype=torch.float32, device=dev)
    call("idv_cbn_bwd_finalize", p(sums), d(count), p(moments), p(bn[0]), p(bn[1]), p(bn[2]), i(C), p(coef), p(g[0]), p(g[1]),
         p(g[2]), p(g[3]), p(g[4]), p(dslope if slope is not None else None), f(1.0 / world), stream_ptr())
    dy = like(y)
    if want_image:
        img = Image.empty(y.C, y.F, y.B, y.T, y.Tp, dev)
        call("idv_cbn_bwd_apply_img", dz.ptr(), y.ptr(), p(fold), p(coef), p(slope), i(C), i(y.F), i(y.B), i(y.Tp), i(y.Jp), i(y.T),
             dy.ptr(), img.ptr(), ll(img.lo_off), stream_ptr())
        return ((dy, img), *g, dslope)
    call("idv_cbn_bwd_apply", dz.ptr(), y.ptr(), p(fold), p(coef), p(slope), i(C), i(y.F), i(y.B), i(y.Tp), i(y.Jp), i(y.T),
         dy.ptr(), stream_ptr())
    return (dy, *g, dslope)


def cbn_finalize(stats, count: float, bn_mod, first_call: bool, momentum: float, update_running: bool = True):
    """stats -> (moments [5, C], fold [C, 6]); running buffers of bn_mod updated in place."""
    C = bn_mod.C
    dev = stats.device
    if BN_SYNC is not None:
        count = count * BN_SYNC(stats)
    moments = torch.empty(5, C, dtype=torch.float32, device=dev)
    fold = torch.empty(C, 6, dtype=torch.float32, device=dev)
    rb = (bn_mod.running_mean_real, bn_mod.running_mean_imag, bn_mod.Vrr, bn_mod.Vri, bn_mod.Vii) if update_running else (None,) * 5
    call("idv_cbn_finalize", p(stats), d(count), p(bn_mod.gamma_rr), p(bn_mod.gamma_ri), p(bn_mod.gamma_ii), p(bn_mod.beta_r),
         p(bn_mod.beta_i), i(C), i(1 if first_call else 0), f(momentum), p(rb[0]), p(rb[1]), p(rb[2]), p(rb[3]), p(rb[4]),
         p(moments), p(fold), stream_ptr())
    return moments, fold


def pw_wgrad(dout_ptr, M: int, Jp_d: int, x_ptr, K: int, Jp_x: int, J: int, dw: torch.Tensor, *, shift=0, rowmap=0, H=0,
             accumulate=False):
    n = int(_ll_fn("idv_pw_wgrad_work_floats")(i(M), i(K), i(J)))
    work = _scratch(n, dw.device)
    # bf16x3 training mode: the split-bf16 kernel for the big contractions (LSTM projections); tiny ones stay fp32
    bf16 = PRECISION == "bf16x3" and WGRAD_BF16 and M >= 64 and K >= 64
    call("idv_pw_bwd_weight_bf16x3" if bf16 else "idv_pw_bwd_weight", dout_ptr, i(M), i(Jp_d), x_ptr, i(K), i(Jp_x), i(J), i(shift), p(work), ll(work.numel()), p(dw),
         i(dw.stride(0)), i(rowmap), i(H), i(1 if accumulate else 0), stream_ptr())


def planar_rowsum(x_ptr, M: int, Jp: int, J: int, out: torch.Tensor, accumulate=False):
    call("idv_planar_rowsum", x_ptr, i(M), i(Jp), i(J), i(1 if accumulate else 0), p(out), stream_ptr())


def mask_apply_bwd(mask: Planar, X: Planar, x_div: int, dpred: Optional[Planar], dpred_c, want_dx: bool = False):
    dm = like(mask)
    dX = like(X) if want_dx else None
    call("idv_mask_apply_bwd", mask.ptr(), X.ptr(), i(x_div), i(X.Jp), dpred.ptr() if dpred is not None else p(None),
         p(dpred_c), i(mask.F), i(mask.B), i(mask.T), i(mask.Tp), i(mask.Jp), dm.ptr(), dX.ptr() if dX is not None else p(None),
         stream_ptr())
    return dm, dX


def complex_to_planar(xc: torch.Tensor, Tp: Optional[int] = None) -> Planar:
    """interleaved float [B, F, T, 2] -> planar [2][1][F][Jp]"""
    B, F, T, _ = xc.shape
    out = Planar.empty(1, F, B, T, Tp or T + 1, xc.device)
    call("idv_complex_to_planar", p(xc.contiguous()), out.ptr(), i(F), i(B), i(T), i(out.Tp), i(out.Jp), stream_ptr())
    return out


def istft_bwd(dy: torch.Tensor, spec: Planar, plan: "DftPlan") -> Planar:
    """d loss / d spec of ops.istft."""
    B, T = spec.B, spec.T
    dfr = Planar.empty(1, plan.win // 2, B, T, spec.Tp, dy.device)
    call("idv_istft_ola_bwd", p(dy.contiguous()), p(plan.env_inv), i(B), i(plan.n_fft), i(plan.win), i(plan.hop), i(T),
         i(spec.Tp), i(dfr.Jp), dfr.ptr(), stream_ptr())
    out = like(spec)
    wT = plan.inv_T()
    pw_gemm(dfr.ptr(), plan.win, wT[0], wT[1], 2 * plan.F, B, spec.Tp, dfr.Jp, T, out.ptr())
    return out


def stft_bwd(dX: Planar, plan: "DftPlan", Lx: int) -> torch.Tensor:
    """d loss / d signal of ops.stft."""
    B, T = dX.B, dX.T
    dfr = Planar.empty(1, plan.win // 2, B, T, dX.Tp, dX.buf.device)
    wT = plan.fwd_T()
    pw_gemm(dX.ptr(), 2 * plan.F, wT[0], wT[1], plan.win, B, dX.Tp, dX.Jp, T, dfr.ptr())
    dx = torch.empty(B, Lx, dtype=torch.float32, device=dX.buf.device)
    call("idv_stft_frames_bwd", dfr.ptr(), i(B), i(Lx), i(plan.n_fft), i(plan.win), i(plan.hop), i(T), i(dX.Tp), i(dfr.Jp),
         p(dx), stream_ptr())
    return dx


def reparam_bwd(lat: Planar, off, zdim: int, eps_r, eps_i, ns: int, dz: Planar, dlat: Planar):
    call("idv_reparam_bwd", lat.ptr(), i(lat.C), i(off[0]), i(off[1]), i(off[2]), i(zdim), p(eps_r), p(eps_i), i(ns), i(lat.B),
         i(lat.T), i(lat.Tp), i(lat.Jp), dz.ptr(), i(dz.Jp), dlat.ptr(), stream_ptr())


# ----------------------------------------------------------------------------- distinguisher (csrc/dis.hip)
RLSTM1_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1")


def _rlstm1_check(x: Planar, params):
    """Shape checks of the hidden-size-1 nn.LSTM on a planar activation -> the eight tensors, contiguous fp32 on x's device."""
    K = 2 * x.C * x.F
    if len(params) != 8:
        raise L.IdvError("rlstm1: the eight nn.LSTM(K, 1, 2) tensors are expected")
    want = [(4, K), (4, 1), (4,), (4,), (4, 1), (4, 1), (4,), (4,)]
    out = []
    for n, t, s in zip(RLSTM1_NAMES, params, want):
        check_dev_f32(t, n, x.buf.device)
        if t.dtype != torch.float32 or tuple(t.shape) != s:
            raise L.IdvError(f"rlstm1: {n} is {t.dtype} {tuple(t.shape)}, expected float32 {s} (input features 2*C*F = {K})")
        out.append(t.detach().contiguous())
    if x.Tp < x.T + 1 or x.Jp < x.B * x.Tp or x.Jp % 4:
        raise L.IdvError("rlstm1: not a planar activation")
    return out


def rlstm1_fwd(x: Planar, params, want_save: bool):
    """nn.LSTM(2*C*F, 1, 2) over the frames of x -> (y [B, T, 1], save or None)."""
    w = _rlstm1_check(x, params)
    dev = x.buf.device
    K = 2 * x.C * x.F
    save = torch.empty(int(_ll_fn("idv_rlstm1_save_doubles")(i(x.B), i(x.T))), dtype=torch.float64, device=dev) if want_save else None
    scratch = torch.empty(int(_ll_fn("idv_rlstm1_fwd_scratch_doubles")(i(K), i(x.Jp))), dtype=torch.float64, device=dev)
    y = torch.empty(x.B, x.T, 1, dtype=torch.float32, device=dev)
    call("idv_rlstm1_fwd", x.ptr(), i(x.C), i(x.F), i(x.B), i(x.T), i(x.Tp), i(x.Jp), *[p(t) for t in w], p(save), p(scratch), p(y),
         stream_ptr())
    return y, save


def rlstm1_bwd(x: Planar, params, save: torch.Tensor, dy: torch.Tensor, want_dx: bool, want_dw: bool):
    """-> (dx Planar or None, dW_ih0 [4, K] or None, dsmall[28]: dW_hh0, db_ih0, db_hh0, dW_ih1, dW_hh1, db_ih1, db_hh1)."""
    w = _rlstm1_check(x, params)
    dev = x.buf.device
    K = 2 * x.C * x.F
    check_dev_f32(dy, "dy", dev)
    if dy.dtype != torch.float32 or dy.numel() != x.B * x.T or not dy.is_contiguous():
        raise L.IdvError(f"rlstm1_bwd: dy must be contiguous float32 [B, T, 1] = [{x.B}, {x.T}, 1]")
    if save is None or save.dtype != torch.float64 or save.numel() != 12 * x.B * x.T:
        raise L.IdvError("rlstm1_bwd: save is not what rlstm1_fwd(..., want_save=True) returned for this shape")
    scratch = torch.empty(int(_ll_fn("idv_rlstm1_bwd_scratch_doubles")(i(K), i(x.B), i(x.Jp))), dtype=torch.float64, device=dev)
    dx = like(x) if want_dx else None
    dw = torch.empty(4, K, dtype=torch.float32, device=dev) if want_dw else None
    small = torch.empty(28, dtype=torch.float32, device=dev)
    call("idv_rlstm1_bwd", x.ptr(), i(x.C), i(x.F), i(x.B), i(x.T), i(x.Tp), i(x.Jp), p(dy), p(w[0]), p(w[1]), p(w[4]), p(w[5]),
         p(save), p(scratch), dx.ptr() if dx is not None else p(None), p(dw), p(small), stream_ptr())
    return dx, dw, small


def _lsgan_pair(a, b):
    check_dev_f32(a, "a")
    if a.dtype != torch.float32 or not a.is_contiguous() or a.numel() == 0:
        raise L.IdvError("lsgan: contiguous non-empty float32 distinguisher outputs expected")
    if b is not None:
        check_dev_f32(b, "b", a.device)
        if b.dtype != torch.float32 or not b.is_contiguous() or b.shape != a.shape:
            raise L.IdvError(f"lsgan: the two distinguisher outputs differ: {tuple(a.shape)} vs {tuple(b.shape)}")


def lsgan(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mean((a - 1)^2 + b^2), or mean((a - 1)^2) without b."""
    _lsgan_pair(a, b)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    call("idv_lsgan", p(a), p(b), ll(a.numel()), p(out), stream_ptr())
    return out[0]


def lsgan_bwd(a: torch.Tensor, b: Optional[torch.Tensor], gout: torch.Tensor, want_a: bool = True, want_b: bool = True):
    _lsgan_pair(a, b)
    da = torch.empty_like(a) if want_a else None
    db = torch.empty_like(b) if (b is not None and want_b) else None
    if da is None and db is None:
        return None, None
    call("idv_lsgan_bwd", p(a), p(b), ll(a.numel()), p(gout.reshape(1).contiguous().float()), p(da), p(db), stream_ptr())
    return da, db
