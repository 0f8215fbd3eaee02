"""Host side of the split-bf16 streaming conv engine (``conv="bf16x3"``; no GPU): the five C entries are declared, exported and
prototyped like their fp32 siblings at ABI version 9, the shape predicate and the pack size answer without a device, the
``conv=`` guard knows the engine, and the float64 model of tests/stream_bf16_ref.py is the oracle's block when the products are
kept exact."""
import importlib

import pytest
import torch

import stream_bf16_ref as R
from oracle import idccrn_oracle as O
from pw_ref import split_model

NEW = ["idv_stream_cconv_bf16_wfloats", "idv_stream_pack_cconv_bf16", "idv_stream_cconv_bf16_supported", "idv_stream_cconv_bf16",
       "idv_stream_cconv_bf16_rows"]

# (transposed, Cin, Cout) of the full-width (base 32) blocks with Cout >= 16 and Cin >= 4: enc1 .. enc5, dec0 .. dec4 with the skips
FULL_WIDTH = [(0, 32, 64), (0, 64, 128), (0, 128, 128), (0, 128, 256), (0, 256, 256),
              (1, 512, 256), (1, 512, 128), (1, 256, 128), (1, 256, 64), (1, 128, 32)]


def _lib():
    return importlib.import_module("i-dccrn-vae_amd._lib")


def test_entries_declared_and_exported_at_abi_9():
    L = _lib()
    declared, protos, lib = L.declared_symbols(), L.prototypes(), L.lib()
    for name in NEW:
        assert name in declared and name in protos and hasattr(lib, name), name
    assert L.declared_abi_version() == 9 and int(lib.idv_abi_version()) == 9
    assert protos["idv_stream_cconv_bf16"] == protos["idv_stream_cconv"]
    assert protos["idv_stream_cconv_bf16_rows"] == protos["idv_stream_cconv_rows"]
    assert protos["idv_stream_pack_cconv_bf16"] == protos["idv_stream_pack_cconv"]
    assert protos["idv_stream_cconv_bf16_wfloats"] == ("long long", ["int", "int"])
    assert protos["idv_stream_cconv_bf16_supported"] == protos["idv_stream_cconv_mfma_supported"]


def test_supported_shapes():
    lib = _lib().lib()
    sup, fp32 = lib.idv_stream_cconv_bf16_supported, lib.idv_stream_cconv_mfma_supported
    for tr, cin, cout in FULL_WIDTH:
        for direction in (0, 1):
            assert sup(direction, cin, cout) == 1, (direction, cin, cout)
    for shape in [(1, 64, 1), (0, 1, 4), (0, 8, 12), (1, 1, 15), (0, 512, 15)]:           # 0 wherever the fp32 MFMA engine says 0
        assert sup(*shape) == 0 and fp32(*shape) == 0, shape
    for shape in [(0, 1, 32), (0, 3, 16), (1, 2, 64)]:                                    # thin inputs stay on the fp32 engines
        assert sup(*shape) == 0 and fp32(*shape) == 1, shape
    assert sup(0, 4, 16) == 1 and sup(1, 5, 17) == 1
    for shape in [(0, 0, 32), (0, 32, 0), (1, -1, 32), (1, 32, -16), (0, 0, 0)]:
        assert sup(*shape) <= 0, shape


def test_pack_size():
    wf = _lib().lib().idv_stream_cconv_bf16_wfloats
    for cin, cout in [(4, 32), (512, 256), (24, 48), (12, 24), (128, 16), (7, 33)]:
        n = wf(cin, cout)
        # both tiles, hi and lo, two time taps, (re, im) as two bf16 per word: 4 words per (channel, kf, row), channels in fours
        assert n == 4 * 5 * 4 * ((cin + 3) // 4) * 2 * 32 * ((cout + 31) // 32), (cin, cout, n)
        assert n % 4 == 0
    assert wf(0, 32) <= 0 and wf(32, 0) <= 0


def test_check_conv():
    S = importlib.import_module("i-dccrn-vae_amd.streaming")
    assert S.CONV_ENGINES == ("valu", "mfma", "bf16x3")
    assert S.check_conv("bf16x3") == "bf16x3" and S.check_conv("valu") == "valu" and S.check_conv("mfma") == "mfma"
    for bad in ("auto", None, "", "BF16X3", "bf16", 3):
        with pytest.raises(ValueError, match="bf16x3"):
            S.check_conv(bad)


def _cpu_state_dict(base, seed):
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    np_ = O.net_params(True, base)
    m = pm.DCCRN_(512, 100, np_, True, "cpu", 400, [0, 1, 2, 3, 4, 5], "mask", False, None, None)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k not in ("data_mean", "data_std")}, seed)
    return sd, np_


@pytest.mark.parametrize("kind,idx", [("enc", 2), ("dec", 1)])
def test_reference_with_exact_products_is_the_oracle_block(kind, idx):
    """One conv shape and one transposed shape (two sources' worth of channels): to 1e-12 in float64; the three-term model stands
    about 1e-5 from it and not closer than the dropped lo lo term."""
    sd, np_ = _cpu_state_dict(4, 14)
    pre = f"std_DCCRN.{'encoders' if kind == 'enc' else 'decoders'}.{idx}."
    w = sd[pre + ("conv.conv_re.weight" if kind == "enc" else "transconv.tconv_re.weight")]
    cin = w.shape[1] if kind == "enc" else w.shape[0]
    fin = 65 if kind == "enc" else 9
    x5 = torch.randn(3, cin, fin, 5, 2, generator=torch.Generator().manual_seed(7))
    sd64 = {k: v.double() for k, v in sd.items()}
    block = O.encoder_block if kind == "enc" else O.decoder_block
    want = block(x5.double(), sd64, pre, np_, idx, True, False)
    got = R.split_block(kind, idx, x5, sd, np_, exact=True)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).norm() / want.norm()) < 1e-12
    model = R.split_block(kind, idx, x5, sd, np_)
    e = float((model - want).norm() / want.norm())
    assert 1e-8 < e < 1e-4, e


def test_split_model_is_exact_on_small_integers():
    """10-bit integers times weights in -3 .. 3 (and the mirror set): the lo part carries what the hi part drops, the lo lo term is
    zero and every sum stays below 2^24: the split model is the plain product."""
    g = torch.Generator().manual_seed(3)
    K = 4096
    w = torch.randint(-3, 4, (8, K), generator=g).float()
    x = torch.randint(-1023, 1024, (K, 16), generator=g).float()
    assert float((w.abs() @ x.abs()).max()) < 2 ** 24
    assert torch.equal(split_model(w, x), w.double() @ x.double())
    assert torch.equal(split_model(x.t().contiguous(), w.t().contiguous()), x.t().double() @ w.t().double())
