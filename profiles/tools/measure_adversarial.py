"""Time of the adversarial decoder fine-tune step (adversarial.AdversarialFineTune, csrc/dis.hip) against the plain two-phase
fine-tune step, and of each new kernel.

    python profiles/tools/measure_adversarial.py [--batch 32] [--ns 2] [--len 64000] [--iters 6] [--warmup 2]
                                                 [--out profiles/adversarial/measure.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o adv -- python profiles/tools/measure_adversarial.py --mode kernels
    python profiles/tools/measure_adversarial.py --merge-trace DIR/.../adv_kernel_trace.csv [--out ...]

  step (default): full width (base 32, zdim 128, K = 2560), synthetic weights, 0.1 N(0, 1) signals, fp32, d_step = 2.
      adversarial:    mean device time of one ``step`` over ``--iters`` iterations (an even number: half of them update the
                      distinguisher) after ``--warmup`` untimed ones, HIP events around the timed window; the means of the
                      iterations with and without a distinguisher update are reported too.
      twophase:       the decoder fine-tune step with SI-SNR alone (frozen noisy encoder, decoder forward, backward, Adam), same run.
      ratio:          adversarial / twophase.
      skip_dis_grads_in_g: the adversarial mean with the switch off, and the difference.
  kernels: the distinguisher's LSTM forward + backward and the two LSGAN losses with their gradients at the workload's shape
      (C = 256, F = 5, B = batch * ns, T = 1 + len / 100), a few times, and nothing else: to be run under a kernel trace of its own.
  --merge-trace: reads that trace, writes the mean time per new kernel into the output file under "kernels", and for the two
      passes over the activation the bytes they move (2 C F Jp floats read by the projection; read and written by the
      back-projection) over their time.
Fails without a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
NEW_KERNELS = ("rl_proj_kernel", "rl_gsum_kernel", "rl_scan_kernel", "rl_bptt_kernel", "rl_small_kernel", "rl_back_kernel",
               "rl_dw_kernel", "lsgan_kernel", "lsgan_bwd_kernel")


def build(base, zdim, ns):
    from oracle import idccrn_oracle as O
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    synth = importlib.import_module("i-dccrn-vae_amd.utils.synth")
    np_ = O.net_params(True, base)

    def load(m, seed):
        m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed), strict=True)
        return m.cuda()
    ye = load(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2), 6)
    de = load(pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP, False), 7)
    D = load(pm.distinguisher(np_, True, "cuda", zdim, NFFT, HOP, WIN), 8)
    for q in ye.parameters():
        q.requires_grad = False
    return ye, de, D


def timed(fn, iters, warmup):
    """Mean device milliseconds of fn(i) over `iters` calls after `warmup` untimed ones, and the per-call times."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn(warmup + i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]
    return sum(per) / iters, per


def mode_step(a):
    adv = importlib.import_module("i-dccrn-vae_amd.adversarial")
    optim = importlib.import_module("i-dccrn-vae_amd.optim")
    nl = importlib.import_module("i-dccrn-vae_amd.model.nsvae_loss")
    if a.iters % 2 or a.warmup % 2:
        raise SystemExit("--iters and --warmup must be even (d_step = 2: every other iteration updates the distinguisher)")
    g = torch.Generator().manual_seed(0)
    clean = (0.1 * torch.randn(a.batch, a.len, generator=g)).cuda()
    noisy = clean + (0.1 * torch.randn(a.batch, a.len, generator=g)).cuda()
    res = {"shape": {"batch": a.batch, "ns": a.ns, "len": a.len, "base": a.base, "zdim": a.zdim, "d_step": 2, "iters": a.iters,
                     "warmup": a.warmup}, "device": torch.cuda.get_device_name(0)}
    for key, skip in (("adversarial", True), ("adversarial_no_skip", False)):
        ye, de, D = build(a.base, a.zdim, a.ns)
        step = adv.AdversarialFineTune(ye, de, D, optim.Adam(de.parameters(), lr=1e-3, weight_decay=1e-3),
                                       optim.Adam(D.parameters(), lr=8e-5, weight_decay=1e-3), d_step=2, skip_dis_grads_in_g=skip)
        mean, per = timed(lambda i: step.step(noisy, clean), a.iters, a.warmup)
        res[key] = {"ms_per_step": mean, "ms_with_d_update": sum(per[0::2]) / len(per[0::2]),
                    "ms_without_d_update": sum(per[1::2]) / len(per[1::2])}
        del step, ye, de, D
        torch.cuda.empty_cache()
    ye, de, D = build(a.base, a.zdim, a.ns)
    opt = optim.Adam(de.parameters(), lr=1e-3, weight_decay=1e-3)
    tl = nl.two_phase_loss([0, 0, 1], 1.0, a.zdim, 1)

    def twophase(i):
        with torch.no_grad():
            r = ye(noisy, train=False)
        with torch.enable_grad():
            rec, prd = de(r[11], r[0], r[8], r[9], r[10], train=True, pad='sig')
            loss = tl.si_snr(clean, rec)
            opt.zero_grad()
            loss.backward()
        opt.step()
    mean, _ = timed(twophase, a.iters, a.warmup)
    res["twophase"] = {"ms_per_step": mean}
    res["ratio"] = res["adversarial"]["ms_per_step"] / mean
    res["skip_dis_grads_in_g_saves_ms"] = res["adversarial_no_skip"]["ms_per_step"] - res["adversarial"]["ms_per_step"]
    return res


def mode_kernels(a):
    ops = importlib.import_module("i-dccrn-vae_amd.ops")
    AG = importlib.import_module("i-dccrn-vae_amd.autograd")
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    C, F, B, T = 8 * a.base, 5, a.batch * a.ns, 1 + a.len // HOP
    mod = pm._RealLSTM1(input_size=2 * C * F, hidden_size=1, num_layers=2).cuda()
    x = ops.Planar.empty(C, F, B, T, T + 1, "cuda", zero=True)
    x.tensor5().normal_(0.0, (2 * C * F) ** -0.5)
    x.buf.requires_grad_(True)
    for _ in range(a.iters):
        with torch.enable_grad():
            y = AG.rlstm1(mod, x)
            loss = AG.lsgan(y, y.detach()) + AG.lsgan(y)
            loss.backward()
    torch.cuda.synchronize()
    return {"kernel_shape": {"C": C, "F": F, "B": B, "T": T, "Jp": x.Jp}}


def merge_trace(a, res):
    rows = list(csv.DictReader(open(a.merge_trace)))
    out = {}
    for name in NEW_KERNELS:
        pat = re.compile(r"(?:^|::|\s)" + name + r"(?:<|\(|\.|$)")
        t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if pat.search(r["Kernel_Name"])]
        if t:
            t = t[len(t) // 3:]                                   # the first calls carry the code-object load
            out[name] = {"us_mean": sum(t) / len(t), "us_min": min(t), "calls": len(t)}
    C, F, B, T = 8 * a.base, 5, a.batch * a.ns, 1 + a.len // HOP
    Jp = (B * (T + 1) + 3) // 4 * 4
    act = 2 * C * F * Jp * 4
    if "rl_proj_kernel" in out:
        out["rl_proj_kernel"]["GBps"] = act / out["rl_proj_kernel"]["us_mean"] / 1e3
    if "rl_back_kernel" in out:
        out["rl_back_kernel"]["GBps"] = 2 * act / out["rl_back_kernel"]["us_mean"] / 1e3
    res["kernels"] = out
    res["kernel_shape"] = {"C": C, "F": F, "B": B, "T": T, "Jp": Jp, "activation_bytes": act}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "kernels"), default="step")
    ap.add_argument("--merge-trace", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ns", type=int, default=2)
    ap.add_argument("--len", type=int, default=64000)
    ap.add_argument("--base", type=int, default=32)
    ap.add_argument("--zdim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "adversarial", "measure.json"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.merge_trace:
        res = merge_trace(a, res)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("measure_adversarial.py measures on the GPU; there is nothing to report without one")
        if a.mode == "kernels":
            print(json.dumps(mode_kernels(a)))
            return
        res.update(mode_step(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
