"""CPU tests of the switch of the paired time-Winograd kernels (two co tiles per workgroup): the additive C entries are declared in
the header and exported by the library, and the switch is host state that needs no GPU."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OPS = importlib.import_module("i-dccrn-vae_amd.ops")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")

NEW_ENTRIES = ("idv_tw_pair", "idv_tw_pair_launches")


def test_header_declares_and_library_exports_the_pair_entries():
    names = LIB.declared_symbols()
    protos = LIB.prototypes()
    lib = LIB.lib()
    for n in NEW_ENTRIES:
        assert n in names and n in protos, n
        assert hasattr(lib, n), n
    assert LIB.declared_abi_version() == 9 and lib.idv_abi_version() == 9          # additive entries: the version stays
    assert protos["idv_tw_pair"] == ("int", ["int"])
    assert protos["idv_tw_pair_launches"] == ("long long", ["int"])
    with open(LIB.HEADER_PATH) as f:
        src = f.read()
    for macro, val in (("IDV_TW_PAIR_T_EVEN", 1), ("IDV_TW_PAIR_T_ODD", 2), ("IDV_TW_PAIR_CONV", 4), ("IDV_TW_PAIR_ALL", 7)):
        assert f"#define {macro} {val}" in src, macro


def test_pair_switch_is_host_state():
    lib = LIB.lib()
    own = lib.idv_tw_pair(-1)
    assert 0 <= own <= 7
    try:
        assert lib.idv_tw_pair(0) == own and lib.idv_tw_pair(-1) == 0
        assert lib.idv_tw_pair(5) == 0 and lib.idv_tw_pair(-1) == 5
        assert lib.idv_tw_pair(0x7fffffff) == 5 and lib.idv_tw_pair(-1) == 7       # bits that select nothing are dropped
        keep = OPS.TW_PAIR, OPS._tw_pair_pushed, OPS._tw_pair_lib
        try:
            OPS._tw_pair_pushed, OPS._tw_pair_lib = None, own
            OPS.TW_PAIR = 2
            OPS._sync_tw_pair()
            assert lib.idv_tw_pair(-1) == 2
            OPS.TW_PAIR = None
            OPS._sync_tw_pair()
            assert lib.idv_tw_pair(-1) == own
        finally:
            OPS.TW_PAIR, OPS._tw_pair_pushed, OPS._tw_pair_lib = keep
    finally:
        lib.idv_tw_pair(own)
    assert lib.idv_tw_pair_launches(0) >= 0 and lib.idv_tw_pair_launches(1) >= 0 and lib.idv_tw_pair_launches(0) == 0
