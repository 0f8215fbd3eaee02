"""CPU tests of the C ABI of the gradient-norm / clipping kernels (csrc/bucket.hip): the additive entries, the
record's field offsets, the number of partials and every refusal before any GPU work; loads the library, needs no GPU."""
import importlib
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIB = importlib.import_module("i-dccrn-vae_amd._lib")
OPTIM = importlib.import_module("i-dccrn-vae_amd.optim")

ADAM = ["ptr", "ptr", "ptr", "ptr", "ptr", "int", "long long", "float", "double", "double", "float", "float", "float", "float", "float"]


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_bucket_sqnorm_partials", "idv_bucket_sqnorm", "idv_bucket_clip_finalize", "idv_bucket_adam_clipped", "idv_bucket_scale"):
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_bucket_sqnorm_partials"] == ("int", ["long long"])
    assert protos["idv_bucket_sqnorm"] == ("int", ["ptr", "ptr", "ptr", "int", "long long", "float", "ptr", "long long", "ptr"])
    assert protos["idv_bucket_clip_finalize"] == ("int", ["ptr", "int", "double", "int", "ptr", "ptr"])
    assert protos["idv_bucket_adam"] == ("int", ADAM + ["ptr"])                       # unchanged
    assert protos["idv_bucket_adam_clipped"] == ("int", ADAM + ["ptr", "int", "long long", "ptr"])
    assert protos["idv_bucket_scale"] == ("int", ["ptr", "int", "long long", "ptr", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9              # additive entries


def test_field_offsets_match_the_header():
    with open(LIB.HEADER_PATH) as f:
        defs = dict(re.findall(r"#define\s+IDV_CLIP_([A-Z0-9_]+)\s+(\d+)", f.read()))
    assert int(defs.pop("RECORD_BYTES")) == OPTIM.CLIP_RECORD_BYTES == 32
    assert {k.lower(): int(v) for k, v in defs.items()} == OPTIM.CLIP_FIELD
    # two doubles, a float, an int, an int64: packed, each aligned to its size
    assert OPTIM.CLIP_FIELD == {"sumsq": 0, "norm": 8, "coef": 16, "finite": 20, "skipped": 24}


def test_partials():
    """One partial per 4096 floats of the PADDED length (tables of 1, 4096, 4097 and 25 M elements pad to 4, 4096, 4100, 25 M)."""
    np_ = LIB.lib().idv_bucket_sqnorm_partials
    assert np_(4) == 1 and np_(4096) == 1 and np_(4100) == 2 and np_(25_000_000) == 6104 and np_(8192) == 2 and np_(8196) == 3
    for total in (0, -4, 1, 4097, 6, (1 << 41) + 4096):     # not positive, not padded to 4, more workgroups than a grid has
        assert np_(total) == -1, total
    assert OPTIM.sqnorm_partials(4100) == 2


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()

    def sqnorm(**kw):
        a = dict(ptable=16, gtable=16, gflat=None, n=3, total=64, scale=1.0, partials=16, first=0)
        a.update(kw)
        return lib.idv_bucket_sqnorm(a["ptable"], a["gtable"], a["gflat"], a["n"], a["total"], a["scale"], a["partials"], a["first"], None)

    for kw in (dict(ptable=None), dict(gtable=None), dict(gflat=16), dict(gtable=None, gflat=8), dict(gtable=None, gflat=20), dict(n=0),
               dict(n=-1), dict(total=0), dict(total=-4), dict(total=62), dict(total=(1 << 41) + 4096), dict(partials=None), dict(partials=4),
               dict(partials=12), dict(first=-1)):
        assert sqnorm(**kw) == -1, kw

    def finalize(**kw):
        a = dict(partials=16, count=5, max_norm=1.0, guard=1, record=32)
        a.update(kw)
        return lib.idv_bucket_clip_finalize(a["partials"], a["count"], a["max_norm"], a["guard"], a["record"], None)

    for kw in (dict(partials=None), dict(partials=4), dict(count=0), dict(count=-2), dict(max_norm=math.nan), dict(record=None), dict(record=4),
               dict(record=36)):
        assert finalize(**kw) == -1, kw

    def adam(**kw):
        a = dict(ptable=16, gtable=16, gflat=None, m=16, v=32, n=3, total=64, bc1=0.1, bc2s=0.03, record=32, guard=1, t=1)
        a.update(kw)
        return lib.idv_bucket_adam_clipped(a["ptable"], a["gtable"], a["gflat"], a["m"], a["v"], a["n"], a["total"], 1e-3, 0.9, 0.999, 1e-8, 0.0,
                                           a["bc1"], a["bc2s"], 1.0, a["record"], a["guard"], a["t"], None)

    for kw in (dict(ptable=None), dict(gtable=None), dict(gflat=16), dict(gtable=None, gflat=8), dict(m=None), dict(m=8), dict(v=None), dict(v=24),
               dict(n=0), dict(total=0), dict(total=62), dict(bc1=0.0), dict(bc2s=math.nan), dict(record=None), dict(record=4), dict(t=0),
               dict(t=-3)):
        assert adam(**kw) == -1, kw

    def scale(**kw):
        a = dict(table=16, n=3, total=64, record=32)
        a.update(kw)
        return lib.idv_bucket_scale(a["table"], a["n"], a["total"], a["record"], None)

    for kw in (dict(table=None), dict(n=0), dict(total=0), dict(total=-8), dict(total=66), dict(record=None), dict(record=12)):
        assert scale(**kw) == -1, kw
