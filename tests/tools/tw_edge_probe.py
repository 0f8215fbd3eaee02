"""Edge workgroups of the time-Winograd transposed conv (csrc/cgemm_tw.hip), two checks to run on a parent build and on this build
(IDV_LIB_PATH selects the library):

  digest   one real layer shape (dec1: 256 + 256 -> 128 channels, Fin = 9, B = 2, seeded inputs): a SHA-256 of the last even output row
           out[2 (Fin - 1)] and one of all other rows.  Between the two builds only the first may differ.  With --save FILE the planes
           are stored, with --against FILE the largest differences to a stored run are printed per group of rows.
  layers   time per call of dec0 .. dec4 at B utterances of 4 s (both row phases; the split per kernel is the profiler's).

    python tests/tools/tw_edge_probe.py digest [--save FILE | --against FILE]
    python tests/tools/tw_edge_probe.py layers [B] [repeats]                      (GPU box)"""
import hashlib
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
amd = importlib.import_module("i-dccrn-vae_amd")
ops = amd.ops
dev = "cuda"
ops.WINO = ops.TW = True


def layer(c0, c1, cout, fin, B, T, g):
    x = torch.randn(B, c0, fin, T, 2, generator=g)
    sk = torch.randn(B, c1, fin, T, 2, generator=g)
    shape = (c0 + c1, cout, 5, 2)
    wr, wi = torch.randn(shape, generator=g) * 0.05, torch.randn(shape, generator=g) * 0.05
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    pk = ops.pack_cconv_gauss(wr.to(dev), wi.to(dev), br.to(dev), bi.to(dev), None, transposed=True)
    xp, skp = ops.Planar.from_tensor5(x.to(dev), T + 1), ops.Planar.from_tensor5(sk.to(dev), T + 1)
    slope = torch.tensor([0.25], device=dev)
    return lambda: ops.cconv2d(xp, None, None, cout, transposed=True, slope=slope, skip=skp, gauss=pk)


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def digest(argv):
    g = torch.Generator().manual_seed(1234)
    ops.LAUNCH_LOG = []
    y = layer(256, 256, 128, 9, 2, 641, g)()
    torch.cuda.synchronize()
    assert [c for c, *_ in ops.LAUNCH_LOG if c in (ops.TW_CFG, ops.TW_CFG + 1)], "time-Winograd kernel not launched"
    pl = y.planes().cpu()                                       # [2, Cout, Fout, B, Tp]
    assert pl.shape[2] == 17
    last, rest = pl[:, :, -1], pl[:, :, :-1]
    print(f"library {ops.L.LIB_PATH}")
    print(f"last even row (row {pl.shape[2] - 1}): sha256 {sha(last)}   all other rows: sha256 {sha(rest)}")
    if "--save" in argv:
        torch.save(pl, argv[argv.index("--save") + 1])
    if "--against" in argv:
        ref = torch.load(argv[argv.index("--against") + 1])
        rlast, rrest = ref[:, :, -1], ref[:, :, :-1]
        d_last, d_rest = float((last - rlast).abs().max()), float((rest - rrest).abs().max())
        rel = float((last.double() - rlast.double()).norm() / rlast.double().norm())
        print(f"against the stored run: last even row max |diff| {d_last:.3e} (relative l2 {rel:.2e}, largest value "
              f"{float(rlast.abs().max()):.3f}); all other rows max |diff| {d_rest:.3e}")
        return 0 if d_rest == 0.0 else 1
    return 0


def layers(argv):
    B = int(argv[0]) if argv else 64
    rep = int(argv[1]) if len(argv) > 1 else 5
    DEC = [(256, 256, 256, 5), (256, 256, 128, 9), (128, 128, 128, 17), (128, 128, 64, 33), (64, 64, 32, 65)]
    g = torch.Generator().manual_seed(0)
    line, tot = [], 0.0
    for k, (c0, c1, cout, fin) in enumerate(DEC):
        x = ops.Planar.empty(c0, fin, B, 641, 642, dev, zero=True)
        x.tensor5().normal_()
        sk = ops.Planar.empty(c1, fin, B, 641, 642, dev, zero=True)
        sk.tensor5().normal_()
        shape = (c0 + c1, cout, 5, 2)
        wr, wi = torch.randn(shape, generator=g).to(dev) * 0.05, torch.randn(shape, generator=g).to(dev) * 0.05
        br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
        pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=True)
        slope = torch.tensor([0.25], device=dev)
        call = lambda: ops.cconv2d(x, None, None, cout, transposed=True, slope=slope, skip=sk, gauss=pk)
        for _ in range(2):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rep):
            call()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / rep
        tot += t
        line.append(f"dec{k} {t:6.3f}")
        del x, sk
    print(f"[time-Winograd, B = {B}, ms per call] " + " | ".join(line) + f" | total {tot:.2f}")
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "digest"
    sys.exit({"digest": digest, "layers": layers}[mode](sys.argv[2:]))
