"""CPU tests of the C ABI of mixture synthesis (csrc/mix.hip): the additive entries, the work size and every refusal
before any GPU work; loads the library, needs no GPU."""
import importlib
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIB = importlib.import_module("i-dccrn-vae_amd._lib")
OPS = importlib.import_module("i-dccrn-vae_amd.ops")

ROWS = ["ptr", "ptr", "long long", "ptr", "ptr", "long long", "ptr", "ptr", "ptr", "int", "int", "int"]


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_mix_work_bytes", "idv_mix_gains", "idv_mix_write"):
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_mix_work_bytes"] == ("long long", ["int", "int", "int"])
    assert protos["idv_mix_gains"] == ("int", ROWS + ["ptr", "int", "double", "double", "int", "double", "ptr", "long long", "ptr", "ptr"])
    assert protos["idv_mix_write"] == ("int", ROWS + ["ptr", "ptr", "ptr", "ptr", "long long", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries


def test_field_indices_match_the_header():
    with open(LIB.HEADER_PATH) as f:
        defs = dict(re.findall(r"#define\s+IDV_MIX_([A-Z0-9_]+)\s+(\d+)", f.read()))
    assert int(defs.pop("WIN_FIELDS")) == OPS.MIX_WIN_FIELDS and int(defs.pop("ROW_FIELDS")) == OPS.MIX_ROW_FIELDS
    assert {k.lower(): int(v) for k, v in defs.items()} == OPS.MIX_FIELD
    assert sorted(OPS.MIX_FIELD.values()) == list(range(OPS.MIX_ROW_FIELDS))


def test_work_bytes():
    wb = LIB.lib().idv_mix_work_bytes
    # six doubles per window and row, the last window of a row may be short
    assert wb(1, 1, 1600) == 48 and wb(1, 1600, 1600) == 48 and wb(1, 1601, 1600) == 96 and wb(3, 16385, 1600) == 3 * 11 * 48
    assert wb(64, 64000, 1600) == 64 * 40 * 48 and wb(1, 1 << 27, 4) == (1 << 25) * 48 and wb(65535, 100, 64) == 65535 * 2 * 48
    for B, L, win in ((0, 100, 1600), (-1, 100, 1600), (65536, 100, 1600), (1, 0, 1600), (1, -5, 1600), (1, (1 << 27) + 1, 1600), (1, 100, 0),
                      (1, 100, -1600), (1, 100, 1602), (1, 100, 2), (1, 100, (1 << 27) + 4), (1, 100, 1 << 30)):
        assert wb(B, L, win) == -1, (B, L, win)


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    rows = dict(clean=8, clean_off=None, ldc=4096, noise=8, noise_off=None, ldn=2048, lens=None, noise_lens=None, phase=None, B=2, L=4096,
                Ln=2048)
    order = list(rows)

    def gains(**kw):
        a = dict(rows, par=8, segmental=0, target_db=-25.0, clip=0.99, win=1600, thresh_db=-50.0, work=8, work_bytes=1 << 40, rows=8)
        a.update(kw)
        return lib.idv_mix_gains(*[a[k] for k in order], a["par"], a["segmental"], a["target_db"], a["clip"], a["win"], a["thresh_db"],
                                 a["work"], a["work_bytes"], a["rows"], None)

    def write(**kw):
        a = dict(rows, rows=8, noisy=8, clean_out=8, noise_out=8, ldy=4096)
        a.update(kw)
        return lib.idv_mix_write(*[a[k] for k in order], a["rows"], a["noisy"], a["clean_out"], a["noise_out"], a["ldy"], None)

    bad_rows = [dict(clean=None), dict(noise=None), dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(L=(1 << 27) + 1),
                dict(Ln=0), dict(Ln=(1 << 27) + 1), dict(ldc=4095), dict(ldn=2047), dict(clean=6), dict(noise=10), dict(clean_off=4),
                dict(noise_off=12)]
    for kw in bad_rows:
        assert gains(**kw) == -1 and write(**kw) == -1, kw
    for kw in (dict(par=None), dict(work=None), dict(rows=None), dict(par=4), dict(work=4), dict(rows=12), dict(segmental=2), dict(segmental=-1),
               dict(target_db=math.inf), dict(target_db=math.nan), dict(thresh_db=-math.inf), dict(clip=math.nan), dict(clip=0.0),
               dict(clip=-0.99), dict(clip=math.inf), dict(win=0), dict(win=-1600), dict(win=1602), dict(win=2), dict(win=1 << 30),
               dict(work_bytes=2 * 3 * 48 - 1), dict(work_bytes=0)):
        assert gains(**kw) == -1, kw
    for kw in (dict(rows=None), dict(rows=4), dict(noisy=None), dict(clean_out=None), dict(noise_out=None), dict(ldy=4095), dict(noisy=6),
               dict(clean_out=2), dict(noise_out=9)):
        assert write(**kw) == -1, kw
    # a pool (offset tables) needs no pitch
    assert gains(clean_off=8, noise_off=8, ldc=0, ldn=0, B=0) == -1
