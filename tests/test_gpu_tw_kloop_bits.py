"""The K loops of the time-Winograd kernels (csrc/cgemm_tw.hip, csrc/cgemm_tw2.hip) may change how they form addresses and in which
order they issue instructions, never what they compute: the operands, their k order per accumulator and every floating-point
expression are fixed, so every output bit is.  Checked here as SHA-256 digests of whole output planes against the digests of the
build BEFORE the K-loop address work ("K loops: addresses and transforms out of the MFMAs' way"), measured on that
build (profiles/tw_kloop_alu/digests.txt):

  dec1   transposed form, 256 + 256 -> 128 channels, Fin = 9, B = 2, T = 641 (tests/tools/tw_edge_probe.py digest): paired kernels, both
         row phases, edge workgroups, two sources;
  enc4   conv form, 128 -> 256 channels, Fin = 17, B = 2, T = 641 (tests/tools/tw2_edge_probe.py digest): paired kernels, edge workgroups;
  dec32  transposed form, 16 + 16 -> 32 channels, Fin = 5, B = 3, T = 42 (J = 129: three column blocks, the last with one column): ONE
         co tile, so the one-co-tile kernels (NCT = 1) of both row phases.

The inputs come from a seeded CPU generator.  `last` is the row the edge workgroups compute, `rest` all other rows."""
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

# (last row, all other rows) of the parent build
PARENT = {
    "dec1": ("9c887475679de930", "b94f48463e29d521"),
    "enc4": ("d3fb6ba8ad7f5c8d", "a9517be3542cf441"),
    "dec32": ("577c1d0ce8391218", "98a05faab98413cd"),
}


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def _transposed(ops, c0, c1, cout, fin, B, T, g, dev="cuda"):
    x = torch.randn(B, c0, fin, T, 2, generator=g)
    sk = torch.randn(B, c1, fin, T, 2, generator=g)
    shape = (c0 + c1, cout, 5, 2)
    wr, wi = torch.randn(shape, generator=g) * 0.05, torch.randn(shape, generator=g) * 0.05
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    pk = ops.pack_cconv_gauss(wr.to(dev), wi.to(dev), br.to(dev), bi.to(dev), None, transposed=True)
    xp, skp = ops.Planar.from_tensor5(x.to(dev), T + 1), ops.Planar.from_tensor5(sk.to(dev), T + 1)
    slope = torch.tensor([0.25], device=dev)
    return ops.cconv2d(xp, None, None, cout, transposed=True, slope=slope, skip=skp, gauss=pk)


def _conv(ops, cin, cout, fin, B, T, g, dev="cuda"):
    x = torch.randn(B, cin, fin, T, 2, generator=g)
    wr, wi = torch.randn(cout, cin, 5, 2, generator=g) * 0.05, torch.randn(cout, cin, 5, 2, generator=g) * 0.05
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    pk = ops.pack_cconv_gauss(wr.to(dev), wi.to(dev), br.to(dev), bi.to(dev), None, transposed=False)
    xp = ops.Planar.from_tensor5(x.to(dev), T + 1)
    slope = torch.tensor([0.25], device=dev)
    return ops.cconv2d(xp, None, None, cout, transposed=False, slope=slope, gauss=pk)


def digests(ops):
    """{case: (digest of the last row, digest of all other rows)} with every time-Winograd route on; the switches are restored."""
    keep = ops.WINO, ops.TW, ops.TW_CONV, ops.LAUNCH_LOG
    out = {}
    try:
        ops.WINO = ops.TW = ops.TW_CONV = True
        for name, want, run in (
            ("dec1", (ops.TW_CFG, ops.TW_CFG + 1), lambda g: _transposed(ops, 256, 256, 128, 9, 2, 641, g)),
            ("enc4", (ops.TW_CFG + 2, ops.TW_CFG + 3), lambda g: _conv(ops, 128, 256, 17, 2, 641, g)),
            ("dec32", (ops.TW_CFG, ops.TW_CFG + 1), lambda g: _transposed(ops, 16, 16, 32, 5, 3, 42, g)),
        ):
            ops.LAUNCH_LOG = []
            ops.tw_pair_launches(reset=True)
            y = run(torch.Generator().manual_seed(1234))
            torch.cuda.synchronize()
            assert [c for c, *_ in ops.LAUNCH_LOG if c in want], f"{name}: time-Winograd kernel not launched"
            if name == "dec32":
                assert ops.tw_pair_launches() == 0, "one co tile: the one-co-tile kernels"
            else:
                assert ops.tw_pair_launches() > 0, f"{name}: the paired kernels"
            pl = y.planes().cpu()                                   # [2, Cout, Fout, B, Tp]
            out[name] = (_sha(pl[:, :, -1]), _sha(pl[:, :, :-1]))
    finally:
        ops.WINO, ops.TW, ops.TW_CONV, ops.LAUNCH_LOG = keep
    return out


@pytest.fixture(scope="module")
def found(amd):
    return digests(amd.ops)


@pytest.mark.parametrize("case", sorted(PARENT))
def test_every_output_bit_is_the_parent_builds(found, case):
    print(case, "this build", found[case], "parent build", PARENT[case])
    assert found[case] == PARENT[case]
