"""usage (GPU box): python tests/tools/lstm_proj_probe.py [B] [T] -- the two constants of csrc/lstm_proj_split.hpp and the
A/B of the layer-0 projection inside the cooperative launch, event-timed at the bottleneck's shape (H = 128, K = 1280):

    idv_pw_gemm, M = 8H, one input part       -> us per 256-row x 64-column tile per CU
    idv_clstm_fwd3, flags 2 (G given)         -> us per step of lstm_stack2_f32_kernel (the combine kernel's few us included)
    idv_clstm_fwd3, flags 16 / 0              -> hoisted against fused projection, and forced opening-phase sizes
"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
amd = importlib.import_module("i-dccrn-vae_amd")
ops = amd.ops
lib = ops.L.lib()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T = int(sys.argv[2]) if len(sys.argv) > 2 else 641
H, K, DEV = 128, 1280, "cuda"
g = torch.Generator().manual_seed(3)
sd = {}
for part in ("re", "im"):
    for l, kin in ((0, K), (1, H)):
        sd[f"lstm_{part}.weight_ih_l{l}"] = (torch.randn(4 * H, kin, generator=g) / kin ** 0.5).to(DEV)
        sd[f"lstm_{part}.weight_hh_l{l}"] = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(DEV)
        sd[f"lstm_{part}.bias_ih_l{l}"] = (torch.randn(4 * H, generator=g) * 0.1).to(DEV)
        sd[f"lstm_{part}.bias_hh_l{l}"] = (torch.randn(4 * H, generator=g) * 0.1).to(DEV)
p0, p1 = ops.pack_lstm(sd.__getitem__, H, K, 0, DEV), ops.pack_lstm(sd.__getitem__, H, H, 1, DEV)
x = ops.Planar.from_tensor5((torch.randn(B, K, 1, T, 2, generator=g) * 0.5).to(DEV))
out = ops.Planar.empty(H, 1, B, T, x.Tp, DEV)
work = torch.zeros(int(lib.idv_clstm_work_floats(H, B, T, x.Jp)), dtype=torch.float32, device=DEV)
i, p = ops.i, ops.p


def timed(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def pw():
    ops.call("idv_pw_gemm", x.ptr(), i(K), p(p0.wih), p(p0.bih), p(None), p(work), i(8 * H), i(B), i(x.Tp), i(x.Jp), i(T), i(1),
             i(8 * H), ops.stream_ptr())


def fwd(flags, c0=-1):
    def run():
        ops.call("idv_clstm_fwd3", x.ptr(), i(K), p(p0.wih), p(p0.bih), p(p0.whh), p(p1.wih), p(p1.bih), p(p1.whh), p(p1.wih_hh),
                 i(H), i(B), i(T), i(x.Tp), i(x.Jp), p(work), out.ptr(), i(flags), p(None), i(c0), ops.stream_ptr())

    def run2():                              # a library from before idv_clstm_fwd3
        ops.call("idv_clstm_fwd2", x.ptr(), i(K), p(p0.wih), p(p0.bih), p(p0.whh), p(p1.wih), p(p1.bih), p(p1.whh), p(p1.wih_hh),
                 i(H), i(B), i(T), i(x.Tp), i(x.Jp), p(work), out.ptr(), i(flags & ~16), p(None), ops.stream_ptr())
    return run if hasattr(lib, "idv_clstm_fwd3") else run2


cus = torch.cuda.get_device_properties(0).multi_processor_count
ngrp = (B * x.Tp + 63) // 64
lo, med = timed(pw)
rounds = -(-(ngrp * 4) // cus)
print(f"B={B} T={T} Tp={x.Tp}: idv_pw_gemm M={8 * H} K={K}: min {lo:.3f} median {med:.3f} ms; {ngrp * 4} workgroups on {cus} CUs = "
      f"{rounds} rounds -> {med * 1e3 / rounds:.1f} us per tile per CU")
lo, med = timed(fwd(2))
print(f"recurrence only (flags 2): min {lo:.3f} median {med:.3f} ms -> {med * 1e3 / T:.3f} us per step")
lo, med = timed(fwd(16))
print(f"hoisted projection (flags 16): min {lo:.3f} median {med:.3f} ms")
if hasattr(lib, "idv_clstm_fwd3"):
    nch = (T + 15) // 16
    for c0 in [-1] + sorted({0, nch // 4, nch // 3, (2 * nch) // 5, nch // 2, (3 * nch) // 5, (3 * nch) // 4, nch}):
        lo, med = timed(fwd(0, c0))
        print(f"fused projection, opening chunks {c0:3d}: min {lo:.3f} median {med:.3f} ms")
assert lib.idv_coop_last_status(1) == 0
