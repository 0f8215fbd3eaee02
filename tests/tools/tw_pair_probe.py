"""Per-layer timing of the time-Winograd convs with two co tiles per workgroup (ops.TW_PAIR) beside the one-co-tile kernels, at the
DCCRN-CL evaluation shapes: dec0 .. dec3 (csrc/cgemm_tw.hip; pair masks 0, 1 = even-row phase, 2 = odd-row phase, 3 = both) and
enc2 .. enc5 (csrc/cgemm_tw2.hip; masks 0, 4).  Prints the time per layer and mask and the largest output difference to mask 0,
which must be 0.     python tests/tools/tw_pair_probe.py [B] [repeats]      (GPU box)"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
amd = importlib.import_module("i-dccrn-vae_amd")
ops = amd.ops

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T = 641
dev = "cuda"
g = torch.Generator().manual_seed(0)
slope = torch.tensor([0.25], device=dev)
ops.WINO = ops.TW = ops.TW_CONV = True


def measure(name, masks, call):
    """call() -> Planar; per mask the mean time of REP launches after two warm-up launches, and the difference to the first mask."""
    times, ref, worst = [], None, 0.0
    for mask in masks:
        ops.TW_PAIR = mask
        for _ in range(2):
            y = call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REP):
            y = call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / REP)
        if ref is None:
            ref = y.planes().clone()
        else:
            worst = max(worst, float((y.planes() - ref).abs().max()))
    print(f"{name}: " + "  ".join(f"mask {m}: {t:6.3f} ms" for m, t in zip(masks, times)) + f"  max |diff to mask {masks[0]}| = {worst:.1e}")
    return times, worst


DEC = [(256, 256, 256), (256, 256, 128), (128, 128, 128), (128, 128, 64)]     # (from below, skip, out)
FE = [5, 9, 17, 33]
tot, bad = [0.0] * 4, 0.0
for k, (c0, c1, cout) in enumerate(DEC):
    x = ops.Planar.empty(c0, FE[k], B, T, T + 1, dev, zero=True)
    x.tensor5().normal_()
    sk = ops.Planar.empty(c1, FE[k], B, T, T + 1, dev, zero=True)
    sk.tensor5().normal_()
    shape = (c0 + c1, cout, 5, 2)
    wr, wi = torch.randn(shape, generator=g).to(dev) * 0.05, torch.randn(shape, generator=g).to(dev) * 0.05
    br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=True)
    t, w = measure(f"dec{k} {c0}+{c1} -> {cout}, F = {FE[k]}", (0, 1, 2, 3),
                   lambda: ops.cconv2d(x, None, None, cout, transposed=True, slope=slope, skip=sk, gauss=pk))
    tot = [a + b for a, b in zip(tot, t)]
    bad = max(bad, w)
print("dec0-3 total: " + "  ".join(f"mask {m}: {t:6.2f} ms" for m, t in zip((0, 1, 2, 3), tot)))

ENC = [(64, 128), (128, 128), (128, 256), (256, 256)]
FI = [65, 33, 17, 9]
tot = [0.0] * 2
for k, (cin, cout) in enumerate(ENC):
    x = ops.Planar.empty(cin, FI[k], B, T, T + 1, dev, zero=True)
    x.tensor5().normal_()
    wr, wi = torch.randn((cout, cin, 5, 2), generator=g).to(dev) * 0.05, torch.randn((cout, cin, 5, 2), generator=g).to(dev) * 0.05
    br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
    pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=False)
    t, w = measure(f"enc{k + 2} {cin} -> {cout}, F = {FI[k]}", (0, 4),
                   lambda: ops.cconv2d(x, None, None, cout, transposed=False, slope=slope, gauss=pk))
    tot = [a + b for a, b in zip(tot, t)]
    bad = max(bad, w)
print("enc2-5 total: " + "  ".join(f"mask {m}: {t:6.2f} ms" for m, t in zip((0, 4), tot)))
print(f"largest output difference: {bad:.1e}" + ("" if bad == 0.0 else "  <-- NOT bit-identical"))
sys.exit(0 if bad == 0.0 else 1)
