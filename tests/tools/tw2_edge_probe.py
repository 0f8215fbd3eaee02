"""Edge workgroups of the time-Winograd conv form (csrc/cgemm_tw2.hip), two checks to run on a parent build and on this build
(IDV_LIB_PATH selects the library):

  digest   one real layer shape (enc4: 128 -> 256 channels, Fin = 17, B = 2, seeded inputs): a SHA-256 of the last output row
           out[Fout - 1] and one of all other rows.  Between the two builds only the first may differ.  With --save FILE the planes
           are stored, with --against FILE the largest differences to a stored run are printed per group of rows.
  layers   time per call of enc2 .. enc5 at B utterances of 4 s, next to the change predicted from the workgroup counts
           (the kernel's time follows its workgroup count).

    python tests/tools/tw2_edge_probe.py digest [--save FILE | --against FILE]
    python tests/tools/tw2_edge_probe.py layers [B] [repeats]                      (GPU box)"""
import hashlib
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
amd = importlib.import_module("i-dccrn-vae_amd")
ops = amd.ops
dev = "cuda"
ops.WINO = ops.TW = ops.TW_CONV = True

# enc2 .. enc5: cin, cout, Fin, and the time of the layer before edge workgroups with the change predicted from the workgroup counts
ENC = [(64, 128, 65, 4.40, -0.13), (128, 128, 33, 4.27, -0.24), (128, 256, 17, 4.70, -0.47), (256, 256, 9, 5.45, -0.91)]


def _tw2_ran():
    return bool([c for c, *_ in ops.LAUNCH_LOG if c in (ops.TW_CFG + 2, ops.TW_CFG + 3)])


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def digest(argv):
    g = torch.Generator().manual_seed(1234)
    cin, cout, fin, B, T = 128, 256, 17, 2, 641
    x = torch.randn(B, cin, fin, T, 2, generator=g)
    wr, wi = torch.randn(cout, cin, 5, 2, generator=g) * 0.05, torch.randn(cout, cin, 5, 2, generator=g) * 0.05
    br, bi = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
    pk = ops.pack_cconv_gauss(wr.to(dev), wi.to(dev), br.to(dev), bi.to(dev), None, transposed=False)
    xp = ops.Planar.from_tensor5(x.to(dev), T + 1)
    slope = torch.tensor([0.25], device=dev)
    ops.LAUNCH_LOG = []
    y = ops.cconv2d(xp, None, None, cout, transposed=False, slope=slope, gauss=pk)
    torch.cuda.synchronize()
    assert _tw2_ran(), "time-Winograd conv kernel not launched"
    pl = y.planes().cpu()                                       # [2, Cout, Fout, B, Tp]
    assert pl.shape[2] == 9
    last, rest = pl[:, :, -1], pl[:, :, :-1]
    print(f"library {ops.L.LIB_PATH}")
    print(f"last row (row {pl.shape[2] - 1}): sha256 {sha(last)}   all other rows: sha256 {sha(rest)}")
    if "--save" in argv:
        torch.save(pl, argv[argv.index("--save") + 1])
    if "--against" in argv:
        ref = torch.load(argv[argv.index("--against") + 1])
        rlast, rrest = ref[:, :, -1], ref[:, :, :-1]
        d_last, d_rest = float((last - rlast).abs().max()), float((rest - rrest).abs().max())
        rel = float((last.double() - rlast.double()).norm() / rlast.double().norm())
        print(f"against the stored run: last row max |diff| {d_last:.3e} (relative l2 {rel:.2e}, largest value "
              f"{float(rlast.abs().max()):.3f}); all other rows max |diff| {d_rest:.3e}")
        return 0 if d_rest == 0.0 else 1
    return 0


def layers(argv):
    B = int(argv[0]) if argv else 64
    rep = int(argv[1]) if len(argv) > 1 else 5
    g = torch.Generator().manual_seed(0)
    rows, tot = [], 0.0
    for k, (cin, cout, fin, before, pred) in enumerate(ENC):
        x = ops.Planar.empty(cin, fin, B, 641, 642, dev, zero=True)
        x.tensor5().normal_()
        shape = (cout, cin, 5, 2)
        wr, wi = torch.randn(shape, generator=g).to(dev) * 0.05, torch.randn(shape, generator=g).to(dev) * 0.05
        br, bi = torch.randn(cout, generator=g).to(dev), torch.randn(cout, generator=g).to(dev)
        pk = ops.pack_cconv_gauss(wr, wi, br, bi, None, transposed=False)
        slope = torch.tensor([0.25], device=dev)
        call = lambda: ops.cconv2d(x, None, None, cout, transposed=False, slope=slope, gauss=pk)
        ops.LAUNCH_LOG = []
        for _ in range(2):
            call()
        assert _tw2_ran(), "time-Winograd conv kernel not launched"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rep):
            call()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / rep
        tot += t
        rows.append((f"enc{k + 2}", cin, cout, fin, t, before, pred))
        del x
    print(f"library {ops.L.LIB_PATH}")
    print(f"[time-Winograd conv form, B = {B}, ms per call]")
    print("| layer | channels | Fin | this run | before edge workgroups (DESIGN.md 3.1e) | predicted change |")
    print("|---|---|---|---|---|---|")
    for name, cin, cout, fin, t, before, pred in rows:
        print(f"| {name} | {cin} -> {cout} | {fin} | {t:6.3f} | {before:.2f} | {pred:+.2f} |")
    print(f"| total | | | {tot:6.3f} | {sum(r[5] for r in rows):.2f} | {sum(r[6] for r in rows):+.2f} |")
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "digest"
    sys.exit({"digest": digest, "layers": layers}[mode](sys.argv[2:]))
