"""CPU tests of the C ABI of the image-source entries (csrc/ism.hip): the additive entries, the field indices and
every refusal before any GPU work; loads the library, needs no GPU."""
import importlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIB = importlib.import_module("i-dccrn-vae_amd._lib")
OPS = importlib.import_module("i-dccrn-vae_amd.ops")


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_ism_work_bytes", "idv_ism_rir", "idv_ism_peaks"):
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_ism_work_bytes"] == ("long long", ["int", "int"])
    assert protos["idv_ism_rir"] == ("int", ["ptr", "ptr", "ptr", "int", "int", "ptr", "long long", "ptr", "long long", "ptr"])
    assert protos["idv_ism_peaks"] == ("int", ["ptr", "long long", "ptr", "int", "ptr", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries


def test_field_indices_match_the_header():
    with open(LIB.HEADER_PATH) as f:
        defs = {k: int(v) for k, v in re.findall(r"#define\s+IDV_ISM_([A-Z]+)\s+(\d+)", f.read())}
    assert defs.pop("FIELDS") == OPS.ISM_FIELDS == 17
    assert defs == {k.upper(): v for k, v in OPS.ISM_FIELD.items()}
    used = sorted(v for k, v in OPS.ISM_FIELD.items() if k != "beta") + list(range(OPS.ISM_FIELD["beta"], OPS.ISM_FIELD["beta"] + 6))
    assert sorted(used) == list(range(OPS.ISM_FIELDS))                         # every field once, the six betas in a row


def test_work_bytes_values_and_refusals():
    fn = LIB.lib().idv_ism_work_bytes
    assert OPS.ISM_TILE == 64
    for B, K in ((1, 1), (1, 64), (1, 65), (5, 4000), (65535, 65536), (3, 63)):
        assert fn(B, K) == 16 * B * ((K + 63) // 64), (B, K)
    for B, K in ((0, 100), (-1, 100), (65536, 100), (1, 0), (1, -5), (1, 65537)):
        assert fn(B, K) == -1, (B, K)


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    good = dict(geom=8, taps=4, max_order=None, B=2, Kmax=1000, h=4, ldh=1000, work=8, work_bytes=16 * 2 * 16)
    order = list(good)

    def run(**kw):
        a = dict(good, **kw)
        return lib.idv_ism_rir(*[a[k] for k in order], None)

    bad = [dict(geom=None), dict(taps=None), dict(h=None), dict(work=None),
           dict(B=0), dict(B=-2), dict(B=65536, work_bytes=1 << 40),
           dict(Kmax=0), dict(Kmax=-1), dict(Kmax=65537, ldh=1 << 17, work_bytes=1 << 40),
           dict(ldh=999), dict(ldh=0), dict(ldh=-1000),
           dict(work_bytes=16 * 2 * 16 - 1), dict(work_bytes=0), dict(work_bytes=-1),
           dict(geom=4), dict(geom=12), dict(work=4), dict(work=20), dict(taps=6), dict(taps=9), dict(max_order=2), dict(max_order=7),
           dict(h=2), dict(h=5)]
    for kw in bad:
        assert run(**kw) == -1, kw

    pgood = dict(h=4, ldh=1000, taps=4, B=3, peaks=4)
    porder = list(pgood)

    def prun(**kw):
        a = dict(pgood, **kw)
        return lib.idv_ism_peaks(*[a[k] for k in porder], None)

    for kw in [dict(h=None), dict(taps=None), dict(peaks=None), dict(B=0), dict(B=-1), dict(B=65536), dict(ldh=0), dict(ldh=-4),
               dict(h=6), dict(taps=5), dict(peaks=10)]:
        assert prun(**kw) == -1, kw
