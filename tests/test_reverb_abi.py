"""CPU tests of the C ABI of reverberation (csrc/reverb.hip): the additive entry and every refusal before any GPU
work; loads the library, needs no GPU."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIB = importlib.import_module("i-dccrn-vae_amd._lib")
OPS = importlib.import_module("i-dccrn-vae_amd.ops")


def test_entry_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    assert "idv_reverb" in declared and "idv_reverb" in protos and hasattr(lib, "idv_reverb")
    assert protos["idv_reverb"] == ("int", ["ptr", "ptr", "long long", "ptr", "ptr", "long long", "ptr", "ptr", "ptr", "int", "int", "int",
                                            "ptr", "long long", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # an additive entry
    assert OPS.REVERB_MAX_TAPS == 1 << 16


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    good = dict(x=8, x_off=None, ldx=4096, h=8, h_off=None, ldh=1024, lens=None, taps=8, hist=None, B=2, L=4096, Kmax=1024, y=8, ldy=4096)
    order = list(good)

    def run(**kw):
        a = dict(good, **kw)
        return lib.idv_reverb(*[a[k] for k in order], None)

    bad = [dict(x=None), dict(h=None), dict(taps=None), dict(y=None),
           dict(B=0), dict(B=-3), dict(B=65536),
           dict(L=0), dict(L=-1), dict(L=(1 << 27) + 1, ldx=1 << 28, ldy=1 << 28),
           dict(Kmax=0), dict(Kmax=-1), dict(Kmax=(1 << 16) + 1, ldh=1 << 17),
           dict(ldx=4095), dict(ldx=0), dict(ldh=1023), dict(ldh=0), dict(ldy=4095), dict(ldy=0),
           dict(x=6), dict(x=9), dict(h=10), dict(y=2), dict(x_off=4, ldx=0), dict(x_off=12), dict(h_off=4, ldh=0), dict(h_off=20),
           dict(lens=6), dict(taps=10), dict(taps=9), dict(hist=7),
           # a pool (offset tables) needs no pitch, but is refused for everything else all the same
           dict(x_off=8, h_off=8, ldx=0, ldh=0, B=0), dict(x_off=8, h_off=8, ldx=0, ldh=0, ldy=100), dict(x_off=8, h_off=8, ldx=0, ldh=0, y=None)]
    for kw in bad:
        assert run(**kw) == -1, kw
