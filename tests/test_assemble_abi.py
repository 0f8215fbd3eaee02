"""CPU tests of the C ABI of clip assembly (csrc/assemble.hip): the additive entries against the exports and the call
sites, and every refusal before any GPU work; loads the library, needs no GPU."""
import importlib
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIB = importlib.import_module("i-dccrn-vae_amd._lib")
OPS = importlib.import_module("i-dccrn-vae_amd.ops")
ASM = importlib.import_module("i-dccrn-vae_amd.dataset.assemble")

TABLES = ["ptr", "long long", "ptr", "ptr", "ptr", "ptr", "ptr", "int"]          # pool, pool_n, src, len, dst, first, count, npieces
PROTOS = {
    "idv_asm_work_bytes": ("long long", ["int", "int", "int"]),
    "idv_asm_activity": ("int", TABLES + ["ptr", "int", "int", "int", "int", "double", "double", "double", "ptr", "long long", "ptr", "ptr",
                                          "ptr", "ptr", "ptr", "ptr", "ptr"]),
    "idv_asm_write": ("int", TABLES + ["ptr", "int", "int", "int", "ptr", "long long", "ptr"]),
}


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name, want in PROTOS.items():
        assert name in declared and hasattr(lib, name), name
        assert protos[name] == want, name
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries
    with open(LIB.HEADER_PATH) as f:
        h = f.read()
    for name, val in (("IDV_ASM_MAX_PIECES", OPS.ASM_MAX_PIECES), ("IDV_ASM_MAX_TRIES", OPS.ASM_MAX_TRIES),
                      ("IDV_ASM_WIN_FIELDS", OPS.ASM_WIN_FIELDS)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", h).group(1)) == val, name
    assert (OPS.ASM_MAX_PIECES, OPS.ASM_MAX_TRIES, OPS.ASM_MAX_ROWS) == (64, 16, 65535) == (ASM.MAX_PIECES, ASM.MAX_TRIES, ASM.MAX_ROWS)


def test_call_sites_pass_what_the_prototypes_take():
    """Every call of an idv_asm_* entry in ops.py passes as many arguments as its prototype has parameters (AsmTables.args() stands
    for the eight of the tables)."""
    import torch
    src = inspect.getsource(OPS)
    z64, z32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    tab = OPS.AsmTables(torch.zeros(4), z64, z32, z32, z32, z32, 1, 1, 4)
    assert len(tab.args()) == len(TABLES)
    for name in ("idv_asm_activity", "idv_asm_write"):
        m = re.search(r'call\("' + name + r'",(.*?)stream_ptr\(\)\)', src, re.S)
        assert m, name
        passed = [a.strip() for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
        assert passed[0] == "*tab.args()", name
        # the tables, the other arguments, the stream
        assert len(TABLES) + (len(passed) - 1) + 1 == len(PROTOS[name][1]), (name, passed)
    m = re.search(r'_ll_fn\("idv_asm_work_bytes"\)\((.*?)\)\)\n', src)
    assert m and len(m.group(1).split(",")) == 3


def test_work_bytes():
    lib = LIB.lib()
    assert lib.idv_asm_work_bytes(1, 1, 800) == 16 and lib.idv_asm_work_bytes(3, 801, 800) == 3 * 2 * 16
    assert lib.idv_asm_work_bytes(65535, 64000, 800) == 65535 * 80 * 16
    for bad in ((0, 100, 800), (65536, 100, 800), (1, 0, 800), (1, (1 << 27) + 1, 800), (1, 100, 0), (1, 100, 802), (1, 100, 2),
                (1, 100, (1 << 27) + 4), (-1, 100, 800)):
        assert lib.idv_asm_work_bytes(*bad) == -1, bad


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    tables = dict(pool=8, pool_n=1000, src=8, len=8, dst=8, first=8, count=8, npieces=10)
    act = dict(tables, rowlen=None, B=2, tries=4, samples=1600, win=800, target_db=-25.0, energy_thresh=0.13, min_activity=0.6, work=8,
               work_bytes=8 * 2 * 16, rowstat=8, active=8, windows=8, activity=8, chosen=8, accepted=8)
    wr = dict(tables, chosen=8, B=2, tries=4, samples=1600, out=8, ldo=1600)

    def run(fn, good, **kw):
        a = dict(good, **kw)
        return fn(*[a[k] for k in good], None)

    bad_tables = [dict(pool=None), dict(src=None), dict(len=None), dict(dst=None), dict(first=None), dict(count=None), dict(pool=6), dict(src=4),
                  dict(len=2), dict(dst=6), dict(first=9), dict(count=10), dict(pool_n=0), dict(pool_n=-5), dict(npieces=0),
                  dict(npieces=(1 << 30) + 1), dict(B=0), dict(B=-1), dict(tries=0), dict(tries=17), dict(B=16384, tries=4), dict(samples=0),
                  dict(samples=-1), dict(samples=(1 << 27) + 1)]
    for kw in bad_tables + [dict(win=0), dict(win=2), dict(win=802), dict(win=-800), dict(work=None), dict(work=4), dict(work_bytes=8 * 2 * 16 - 1),
                            dict(rowstat=None), dict(active=None), dict(windows=None), dict(activity=None), dict(chosen=None), dict(accepted=None),
                            dict(rowstat=4), dict(activity=12), dict(active=2), dict(windows=6), dict(chosen=5), dict(accepted=7), dict(rowlen=6),
                            dict(target_db=float("nan")), dict(energy_thresh=float("inf")), dict(min_activity=float("nan"))]:
        assert run(lib.idv_asm_activity, act, **kw) == -1, kw
    for kw in bad_tables + [dict(chosen=None), dict(out=None), dict(chosen=6), dict(out=2), dict(ldo=1599), dict(ldo=0)]:
        assert run(lib.idv_asm_write, wr, **kw) == -1, kw
