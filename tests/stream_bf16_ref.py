"""Float64 model of one streaming conv block in split-bf16 (bf16x3) arithmetic (csrc/stream_conv_bf16.hip, ``conv="bf16x3"``).  A plain
module: it calls nothing of the package under test and runs on CPU tensors.

The complex conv is bilinear in (w, x), so the value the engine defines is the sum of three float64 convs of the definition of
tests/pw_ref.py (``split``): (w_lo, x_hi) + (w_hi, x_lo) + (w_hi, x_hi), with the raw real and imaginary weights and every input
column (the history column included) split.  Bias, the eval batch norm and PReLU follow in float64.  ``exact=True`` keeps the
unsplit operands instead (the product w x itself): the block of the oracle in float64."""
import torch

from oracle import idccrn_oracle as O
from pw_ref import split


def _conv(kind, x5, w_re, w_im, np_, idx):
    """The complex conv / transposed conv of block ``idx`` without bias, causal, float64."""
    z = torch.zeros(w_re.shape[1 if kind == "dec" else 0], dtype=torch.float64)
    if kind == "enc":
        return O.complex_conv2d(x5, w_re, z, w_im, z, np_["encoder_strides"][idx], np_["encoder_paddings"][idx], True)
    return O.complex_conv_transpose2d(x5, w_re, z, w_im, z, np_["decoder_strides"][idx], np_["decoder_paddings"][idx], True)


def split_block(kind, idx, x5, sd, np_, exact=False):
    """``kind`` "enc" / "dec", x5 [B, Cin, Fin, T, 2] (fp32 values) and the state dict of the model -> float64
    [B, Cout, Fout, T, 2]: what ``O.encoder_block`` / ``O.decoder_block`` (eval, causal) return, with the products of the conv in
    bf16x3 arithmetic (``exact``: in plain float64)."""
    pre = f"std_DCCRN.{'encoders' if kind == 'enc' else 'decoders'}.{idx}."
    cv = pre + ("conv.conv_" if kind == "enc" else "transconv.tconv_")
    w_re, w_im = sd[cv + "re.weight"].float(), sd[cv + "im.weight"].float()
    if exact:
        y = _conv(kind, x5.double(), w_re.double(), w_im.double(), np_, idx)
    else:
        (xh, xl), (rh, rl), (ih, il) = split(x5), split(w_re), split(w_im)
        y = _conv(kind, xh, rl, il, np_, idx) + _conv(kind, xl, rh, ih, np_, idx) + _conv(kind, xh, rh, ih, np_, idx)
    b_re, b_im = sd[cv + "re.bias"].double(), sd[cv + "im.bias"].double()
    y = y + torch.stack((b_re - b_im, b_re + b_im), dim=-1).reshape(1, -1, 1, 1, 2)
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(pre)}
    return O.prelu(O._cbn(y, sd64, pre + "bn.", False, None), sd64[pre + "prelu.weight"])
