"""Host side of the fp32-MFMA streaming conv engine (no GPU): the five C entries are declared and exported at ABI version 9, the
shape predicate and the pack size answer without a device, and the ``conv=`` guard of the streamers."""
import importlib

import pytest

NEW = ["idv_stream_cconv_mfma_wfloats", "idv_stream_pack_cconv_mfma", "idv_stream_cconv_mfma_supported", "idv_stream_cconv_mfma",
       "idv_stream_cconv_mfma_rows"]

# (transposed, Cin, Cout) of the eleven full-width (base 32) blocks with Cout >= 16: enc0 .. enc5, dec0 .. dec4 with the skips
FULL_WIDTH = [(0, 1, 32), (0, 32, 64), (0, 64, 128), (0, 128, 128), (0, 128, 256), (0, 256, 256),
              (1, 512, 256), (1, 512, 128), (1, 256, 128), (1, 256, 64), (1, 128, 32)]


def _lib():
    return importlib.import_module("i-dccrn-vae_amd._lib")


def test_entries_declared_and_exported_at_abi_9():
    L = _lib()
    declared, protos, lib = L.declared_symbols(), L.prototypes(), L.lib()
    for name in NEW:
        assert name in declared and name in protos and hasattr(lib, name), name
    assert L.declared_abi_version() == 9 and int(lib.idv_abi_version()) == 9
    assert protos["idv_stream_cconv_mfma"] == protos["idv_stream_cconv"]
    assert protos["idv_stream_cconv_mfma_rows"] == protos["idv_stream_cconv_rows"]
    assert protos["idv_stream_pack_cconv_mfma"] == protos["idv_stream_pack_cconv"]
    assert protos["idv_stream_cconv_mfma_wfloats"] == ("long long", ["int", "int"])


def test_supported_shapes():
    sup = _lib().lib().idv_stream_cconv_mfma_supported
    for tr, cin, cout in FULL_WIDTH:
        for direction in (0, 1):
            assert sup(direction, cin, cout) == 1, (direction, cin, cout)
    for shape in [(1, 64, 1), (0, 1, 4), (0, 8, 12)]:
        assert sup(*shape) == 0, shape
    assert sup(0, 1, 16) == 1 and sup(1, 1, 15) == 0
    for shape in [(0, 0, 32), (0, 32, 0), (1, -1, 32), (1, 32, -16), (0, 0, 0)]:
        assert sup(*shape) <= 0, shape


def test_pack_size():
    wf = _lib().lib().idv_stream_cconv_mfma_wfloats
    for cin, cout in [(1, 32), (512, 256), (24, 48), (12, 24), (128, 16), (7, 33)]:
        n = wf(cin, cout)
        assert n > 0 and n >= 4 * 5 * cin * 32 * ((cout + 31) // 32), (cin, cout, n)
    assert wf(0, 32) <= 0 and wf(32, 0) <= 0


def test_check_conv():
    S = importlib.import_module("i-dccrn-vae_amd.streaming")
    assert S.check_conv("valu") == "valu" and S.check_conv("mfma") == "mfma"
    for bad in ("auto", None, "", "MFMA", 1):
        with pytest.raises(ValueError, match="conv"):
            S.check_conv(bad)
