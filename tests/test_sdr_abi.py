"""CPU tests of the C ABI of the BSS-eval SDR (csrc/sdr.hip): the additive entries, the work size and every refusal
before any GPU work; loads the library, needs no GPU."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIB = importlib.import_module("i-dccrn-vae_amd._lib")


def work_bytes(B, L, K):
    """The formula of the header: per row the lag sums of T1 tiles of 256 sample blocks, the filter, a status word and the two
    energies of T3 tiles of 4096 outputs, all doubles."""
    t1 = -(-((L + 14) // 16 + 1) // 256)
    t3 = -(-(L + K - 1) // 4096)
    return 8 * B * (2 * K * t1 + K + 1 + 2 * t3)


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_sdr_work_bytes", "idv_sdr"):
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_sdr_work_bytes"] == ("long long", ["int", "int", "int"])
    assert protos["idv_sdr"] == ("int", ["ptr", "long long", "ptr", "long long", "ptr", "int", "int", "int", "ptr", "long long", "ptr", "ptr",
                                         "ptr", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries


def test_work_bytes():
    wb = LIB.lib().idv_sdr_work_bytes
    assert wb(1, 1, 16) == 8 * (32 + 16 + 1 + 2) and wb(1, 1, 512) == 8 * (1024 + 512 + 1 + 2)
    # (L + 14) / 16 + 1 sample blocks, the one more for the lags that reach back: 4081 is the last length of one tile of 256
    assert wb(1, 4081, 512) == 8 * (1024 + 512 + 1 + 4) and wb(1, 4082, 512) == 8 * (2048 + 512 + 1 + 4)
    # 4096 outputs per energy tile: L + K - 1 = 4096 is the last length of one
    assert wb(1, 4033, 64) == 8 * (128 + 64 + 1 + 2) and wb(1, 4034, 64) == 8 * (128 + 64 + 1 + 4)
    for B, L, K in ((1, 16385, 512), (3, 160000, 512), (64, 160000, 512), (65535, 100, 16), (1, 1 << 27, 512), (7, 4001, 64), (2, 300, 496)):
        assert wb(B, L, K) == work_bytes(B, L, K), (B, L, K)
    assert wb(64, 160000, 512) == 64 * 8 * (1024 * 40 + 513 + 2 * 40)
    for B, L, K in ((0, 100, 512), (-1, 100, 512), (65536, 100, 512), (1, 0, 512), (1, -5, 512), (1, (1 << 27) + 1, 512), (1, 100, 0),
                    (1, 100, 8), (1, 100, 24), (1, 100, 520), (1, 100, 528), (1, 100, 1024), (1, 100, -16), (1, 100, 500)):
        assert wb(B, L, K) == -1, (B, L, K)


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    good = dict(ref=16, ref_ld=4096, est=16, est_ld=4100, lens=None, B=2, Lmax=4096, K=512, work=32, work_bytes=work_bytes(2, 4096, 512) - 1,
                out=16, details=None, filt=None)
    order = list(good)

    def sdr(**kw):
        a = dict(good)
        a.update(kw)
        return lib.idv_sdr(*[a[k] for k in order], None)

    # the one bad argument of `good` itself is the work size, one byte short: with it mended only the cases below refuse
    assert sdr() == -1
    full = work_bytes(2, 4096, 512)
    for kw in (dict(ref=None), dict(est=None), dict(work=None), dict(out=None), dict(B=0), dict(B=-2), dict(B=65536), dict(Lmax=0),
               dict(Lmax=-1), dict(Lmax=(1 << 27) + 1), dict(K=0), dict(K=8), dict(K=24), dict(K=520), dict(K=1024), dict(K=-512),
               dict(ref_ld=4095), dict(est_ld=4095), dict(ref_ld=0), dict(est_ld=-4096), dict(work=40), dict(work=36), dict(details=12),
               dict(filt=20), dict(ref=18), dict(est=6), dict(out=10), dict(lens=2), dict(work_bytes=0), dict(work_bytes=-1),
               dict(work_bytes=work_bytes(1, 4096, 512)), dict(B=3), dict(Lmax=4096, ref_ld=1 << 40, K=528)):
        a = dict(work_bytes=full)
        a.update(kw)
        assert sdr(**a) == -1, kw
