#!/usr/bin/env python3
"""Generate the fixtures of the adversarial decoder fine-tune by RUNNING THE REAL REFERENCE
(model/pvae_module.py distinguisher, model/nsvae_loss.py adversarial_second_phase_loss, the step of
i_dccrn_vae/nsvae_dccrn/train_second_phase_adversarial.py:290-320 and its validation pass :351-370).

Run in the build container only (the reference never travels):
``PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adv.py [op] [mini] [full]``

Data only: inputs, expected outputs, gradients.  Weights are rebuilt on both sides from oracle.synth_tensor.  Every gradient is
stored twice: from the reference in float32 (``g:`` / ``n:`` = summarised gradient / full L2 norm, as make_golden.py's grad_record)
and from the same reference run with ``.double()`` modules and inputs (``g64:`` / ``n64:``), so that the distance of the float32
reference from the float64 truth is known per tensor; the GPU tests derive their tolerances from it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (puts the repository root and the reference on sys.path; helpers rnd / save / load_synth ...)

O, R_pm, R_nl = G.O, G.R_pm, G.R_nl
NFFT, HOP, WIN = G.NFFT, G.HOP, G.WIN
SKIP = [0, 1, 2, 3, 4, 5]
DLR, LR, WD = 8e-5, 1e-3, 1e-3
ADAM_KEYS = ("conv_re.weight", "gamma_ri", "prelu.weight", "weight_hh_l1", "weight_ih_l0", "linear_read.weight", "tconv_im.weight")


def as_dtype(module, dtype):
    """The reference module in `dtype`: parameters, buffers, and the Hann windows its STFT / ISTFT keep as plain attributes."""
    module.to(dtype)
    for m in module.modules():
        if isinstance(getattr(m, "window", None), torch.Tensor):
            m.window = torch.hann_window(m.win_length, dtype=dtype)
    return module


def grad_store(out, tag, prefix, module, limit, cap):
    for k, p_ in module.named_parameters():
        if p_.grad is not None:
            out[f"g{tag}:{prefix}{k}"] = G.summarize(p_.grad, limit, cap).float()     # float64 run: stored rounded once to float32
            out[f"n{tag}:{prefix}{k}"] = p_.grad.double().norm()


def adam_store(out, prefix, module, limit, cap):
    for k, p_ in module.named_parameters():
        if p_.grad is not None and k.endswith(ADAM_KEYS):
            out[f"a:{prefix}{k}"] = G.summarize(p_, limit, cap)


class draws:
    """torch.randn_like replaced by the recorded draws for the duration of an encoder call (make_golden.py's way)."""

    def __init__(self, eps, dtype):
        self.eps, self.dtype = [e.to(dtype) for e in eps], dtype

    def __enter__(self):
        self.orig = torch.randn_like
        torch.randn_like = lambda t, *a, **k: self.eps.pop(0)

    def __exit__(self, *a):
        torch.randn_like = self.orig


# ----------------------------------------------------------------------------- the distinguisher on its own
def gen_op_dis(base=4, B=3, L=700, seed=101):
    print(f"== distinguisher: base={base} B={B} L={L}")
    np_ = O.net_params(True, base)
    x, x2 = G.rnd(seed + 100, B, L, scale=0.1), G.rnd(seed + 101, B, L, scale=0.1)
    out = dict(x=x, x2=x2, seed=seed, base=base)
    for tag, dtype in (("", torch.float32), ("64", torch.float64)):
        with torch.enable_grad():
            D = R_pm.distinguisher(np_, True, "cpu", 16, NFFT, HOP, WIN)
            G.load_synth(D, seed)
            as_dtype(D, dtype)
            D.train()
            xin = x.detach().to(dtype).clone().requires_grad_(True)
            seen = {}
            hook = D.lstms[0].register_forward_pre_hook(lambda m, a: (a[0].retain_grad(), seen.__setitem__("x", a[0])) and None)
            y = D(xin, train=True)
            hook.remove()
            loss = 0.5 * torch.mean((y - 1).pow(2))            # the distinguisher path of generator_loss, alone
            loss.backward()
        out[f"y{tag}"], out[f"loss{tag}"], out[f"gx{tag}"] = y.detach().float(), loss.detach().double(), xin.grad.float()
        grad_store(out, tag, "", D, 1 << 30, 1 << 30)
        if tag == "64":
            # the LSTM on its own, in float64 as it ran: its [T, B, K] input, the gradient arriving there, its output, its gradients
            out["lstm_in64"], out["lstm_gin64"], out["lstm_y64"] = seen["x"].detach(), seen["x"].grad, y.detach()
            for k, p_ in D.lstms[0].named_parameters():
                out["lstm_g64:" + k] = p_.grad
        if tag == "":
            with torch.no_grad():
                y2 = D(x2, train=True)                          # the second train-mode call OVERWRITES the running buffers
            out["y2"] = y2
            for k, v in D.state_dict().items():
                if ".bn." in k and k.endswith(("running_mean_real", "running_mean_imag", "Vrr", "Vri", "Vii")):
                    out["bn:" + k] = v
            out["init_flag"] = np.asarray([int(m.init_flag) for m in D.modules() if hasattr(m, "init_flag")])
            sd = D.state_dict()
            out["sd_keys"] = np.asarray(list(sd.keys()))
            out["sd_shapes"] = np.asarray([",".join(str(n) for n in v.shape) for v in sd.values()])
            print(f"  T = {y.shape[1]}, K = {sd['lstms.0.weight_ih_l0'].shape[1]}, state_dict entries: {len(sd)}")
    G.save("op_dis_mini", **out)


# ----------------------------------------------------------------------------- the whole step
def run_steps(out, tag, dtype, base, zdim, B, L, ns, seed, iters, limit, cap, adam, first):
    np_ = O.net_params(True, base)
    T = 1 + L // HOP
    with torch.enable_grad():
        ye = R_pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cpu", zdim, NFFT, HOP, WIN, ns, 2)
        de = R_pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cpu", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP, False)
        D = R_pm.distinguisher(np_, True, "cpu", zdim, NFFT, HOP, WIN)
        G.load_synth(ye, seed + 6), G.load_synth(de, seed + 7), G.load_synth(D, seed + 8)
        for m in (ye, de, D):
            as_dtype(m, dtype)
        for p_ in ye.parameters():
            p_.requires_grad = False
        model_loss = R_nl.adversarial_second_phase_loss(1)
        opt_de = torch.optim.Adam(de.parameters(), lr=LR, weight_decay=WD)
        opt_dis = torch.optim.Adam(D.parameters(), lr=DLR, weight_decay=WD)

        def batch(it):
            clean, noise = G.rnd(seed + 110 + 10 * it, B, L, scale=0.1), G.rnd(seed + 111 + 10 * it, B, L, scale=0.1)
            eps = [G.rnd(seed + 340 + 10 * it + i, B, ns, T, zdim) for i in range(4)]
            if first:
                out.update({f"clean{it}": clean, f"noise{it}": noise}, **{f"eps{it}_{i}": e for i, e in enumerate(eps)})
            return clean.to(dtype), noise.to(dtype), eps

        def generate(clean, noise, eps, train):
            with draws(eps, dtype):
                r = ye(clean + noise, train=False)
            z, sky, C, F, stft_y = r[0], r[8], r[9], r[10], r[11]
            rec, _ = de(stft_y, z, sky, C, F, train=train, pad='sig')
            cb = clean.unsqueeze(1).repeat(1, ns, 1).view(B * ns, L)
            return rec, cb

        # validation pass of the script, before any update (the distinguisher with train=True: it only overwrites its buffers)
        clean, noise, eps = batch(0)
        with torch.no_grad():
            ye.eval(), de.eval(), D.eval()
            rec, cb = generate(clean, noise, list(eps), False)
            dt, dest = D(cb, train=True), D(rec, train=True)
            dist_loss = model_loss.distinguisher_loss(dt, dest, None, None)
            gen_loss, loss_recon, loss_dis_gen = model_loss.generator_loss(cb, rec, dest, None, None, None)
        out[f"val_loss{tag}"] = torch.stack([gen_loss, loss_recon, loss_dis_gen, dist_loss]).double()

        ye.eval(), de.train(), D.train()
        for it in range(iters):
            clean, noise, eps = batch(it)
            rec, cb = generate(clean, noise, list(eps), True)
            if it % 2 == 0:                                               # d_step = 2
                dt, dest = D(cb, train=True), D(rec.detach(), train=True)
                dist_loss = model_loss.distinguisher_loss(dt, dest, None, None)
                opt_dis.zero_grad()
                dist_loss.backward()
                grad_store(out, tag, f"dis{it}.", D, limit, cap)
                opt_dis.step()
                if adam and first:
                    adam_store(out, f"dis{it}.", D, limit, cap)
            dg = D(rec, train=True)
            gen_loss, loss_recon, loss_dis_gen = model_loss.generator_loss(cb, rec, dg, None, None, None)
            opt_de.zero_grad()
            gen_loss.backward()
            grad_store(out, tag, f"dec{it}.", de, limit, cap)
            opt_de.step()
            if adam and first:
                adam_store(out, f"dec{it}.", de, limit, cap)
            out[f"loss{it}{tag}"] = torch.stack([gen_loss, loss_recon, loss_dis_gen, dist_loss]).detach().double()
            if it == 0:
                out[f"recon0{tag}"] = rec.detach().float()
                if tag == "64":
                    out["dis_true64"], out["dis_est64"], out["dis_gen64"] = dt.detach(), dest.detach(), dg.detach()
            print(f"  [{dtype}] it {it}: gen {float(gen_loss.detach()):.6f} sisnr {float(loss_recon.detach()):.6f} "
                  f"dis_gen {float(loss_dis_gen.detach()):.6f} dist {float(dist_loss.detach()):.6f}")


def gen_grad_adv(name, base, zdim, B, L, ns, seed, iters, limit=16384, cap=8192, adam=True):
    print(f"== adversarial step {name}: base={base} zdim={zdim} B={B} ns={ns} L={L} iterations={iters}")
    out = dict(seed=seed, base=base, zdim=zdim, ns=ns, iters=iters, sum_limit=limit, sum_cap=cap, d_step=2,
               lr=np.asarray([LR, DLR, WD]))
    run_steps(out, "", torch.float32, base, zdim, B, L, ns, seed, iters, limit, cap, adam, True)
    run_steps(out, "64", torch.float64, base, zdim, B, L, ns, seed, iters, limit, cap, adam, False)
    worst = (0.0, "")
    for k in list(out):
        if k.startswith("g:"):
            a, b = out[k].double(), out["g64" + k[1:]].double()
            worst = max(worst, (float((a - b).norm() / (b.norm() + 1e-30)), k))
    print("  worst float32-vs-float64 gradient distance of the reference:", worst)
    G.save(f"grad_adv_{name}", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["op", "mini", "full"]
    if "op" in which:
        gen_op_dis()
    if "mini" in which:
        gen_grad_adv("mini", 4, 32, 2, 1600, 2, 171, iters=2, limit=3072, cap=1536)
    if "full" in which:
        torch.set_num_threads(os.cpu_count())
        gen_grad_adv("full", 32, 128, 1, 1600, 2, 193, iters=1, limit=2048, cap=1024, adam=False)
