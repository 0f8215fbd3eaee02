"""CPU tests behind the latent and loss suite (tests/test_gpu_loss.py).

1. The float64 reference (tests/loss_ref.py) against the oracle's own functions (complex_kl, reparameterization, si_snr,
   multiple_recon_loss, sisdr_np, residual_loss, the miu distance of nsvae_loss) to 1e-12.
2. The conditions the GPU file relies on, for every entry of its case tables: on every drawn element the guard decision
   a >= sigma - 1e-3 is the same in float32 and float64 and lies at least 1e-2 sigma from its threshold; every kind switches the
   guard as it says; the noise keeps |e - s_t|^2 away from its clamp; every entry has a case past its grid cap.
3. The asserted bounds notice mistakes: each mutant of the reference moves at least one compared quantity of at least one case
   by more than the bound the GPU file asserts for it.
4. Every refusal of the entries is IDV_EINVAL with dummy pointers, before any GPU work (the library is loaded, no GPU needed)."""
import importlib

import pytest
import torch

import loss_ref as R
import test_gpu_loss as G
from oracle import idccrn_oracle as O

LIB = importlib.import_module("i-dccrn-vae_amd._lib")


def ri(a, b):
    """Two [zdim, B, T] -> the oracle's [B, T, zdim, 2]."""
    return torch.stack((a, b), dim=-1).permute(1, 2, 0, 3)


def oracle_latent(q):
    q = R.dbl(q)
    return ri(q["mr"], q["mi"]), ri(q["ls"], torch.zeros_like(q["ls"])), ri(q["dr"], q["di"])


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return bool(((a - b).abs() <= tol * b.abs().clamp_min(1e-300)).all())


# ----------------------------------------------------------------------------- 1. the reference against the oracle
@pytest.mark.parametrize("kind", R.KINDS)
def test_latent_reference_equals_the_oracle(kind):
    zdim, B, T, ns = 5, 3, 7, 3
    q1, q2 = R.gen_latent(kind, zdim, B, T, 1), R.gen_latent("guarded" if kind == "plain" else "plain", zdim, B, T, 2)
    eps_r, eps_i = R.gen_eps(zdim, B, T, ns, 3)
    m, l, d = oracle_latent(q1)
    want = O.reparameterization(m, l, d, ns, eps_r.double(), eps_i.double())            # [B * ns, T, zdim, 2]
    assert close(R.reparam(q1, eps_r, eps_i, ns), want.permute(3, 2, 0, 1))
    m2, l2, d2 = oracle_latent(q2)
    for eps in (1e-9, 1e-10):
        assert close(R.ckl(q1, q2, eps), O.complex_kl(m, m2, l, l2, d, d2, eps).mean())
        z = torch.zeros_like(m)
        assert close(R.ckl(q1, None, eps), O.complex_kl(m, z, l, z, d, z, eps).mean())
    value, sums = R.miu_dist(q1, q2)
    assert close(value, torch.sqrt(torch.sum(torch.mean((m - m2) ** 2, dim=(0, 1)))))
    assert close(sums.sum(), ((m - m2) ** 2).sum())


def test_waveform_reference_equals_the_oracle():
    src, est = R.gen_waves("normal", 6, 257, 3, 4)
    rows = R.source_rows(src, 6, 3).double()
    assert torch.equal(rows[0], rows[2]) and torch.equal(rows[3], src[1].double())
    assert close(R.si_snr(src, est, 3), O.si_snr(rows, est.double()))
    E, D, Q = R.dots(src, est, 3).unbind(1)
    assert close(E, (rows * rows).sum(1)) and close(D, (rows * est.double()).sum(1)) and close(Q, (est.double() ** 2).sum(1))
    # the numpy original takes the machine epsilon of its input's type: float64 in, 2^-52; float32 in (the kernel's 2^-23), it
    # also sums in float32
    want = [O.sisdr_np(est[b].double().numpy(), rows[b].numpy()).item() for b in range(6)]
    assert close(R.si_sdr(rows.float(), est, eps=2.0 ** -52), want)
    want = [O.sisdr_np(est[b].numpy(), rows[b].float().numpy()).item() for b in range(6)]
    assert close(R.si_sdr(rows.float(), est), want, 1e-5)
    lens = (-3, 0, 1, 200, 257, 300)
    cut = R.si_sdr(rows.float(), est, lens)
    for b, n in enumerate(lens):
        n = max(0, min(n, 257))
        assert close(cut[b], R.si_sdr(rows[b:b + 1, :n].float(), est[b:b + 1, :n])[0])


def test_spectrum_reference_equals_the_oracle():
    B, F, T, div = 4, 9, 5, 2
    pred, ori = R.gen("normal", (B, F, T, 2), 5), R.gen("normal", (B // div, F, T, 2), 6)
    cpx, mag, total = R.recon(pred, ori, div)
    rows = R.source_rows(ori, B, div).double()
    src, est = R.gen_waves("normal", B, 40, 1, 7)
    _, l_cpx, l_mag, _ = O.multiple_recon_loss(pred.double(), rows, src.double(), est.double(), (1.0, 1.0, 1.0))
    assert close(cpx, l_cpx) and close(mag, l_mag) and close(total, l_cpx * B * T)
    # one term of residual_loss: the clean encoder's skip against the first half of the noisy encoder's channels
    C = 3
    clean, noisy = R.gen("normal", (2, B, C, F, T), 8).double(), R.gen("normal", (2, B, 2 * C, F, T), 9).double()
    layout = lambda v: v.permute(0, 2, 3, 1, 4)                                  # [2, B, C, F, T] -> [2, C, F, B, T]
    five = lambda v: v.permute(1, 2, 3, 4, 0)                                    # -> the oracle's [B, C, F, T, 2]
    _, speech, _ = O.residual_loss([five(clean)], [None], [five(noisy)], [0], 1, True, "speech")
    mean, total = R.msd(layout(clean), layout(noisy), 0, 0, C)
    assert close(mean, speech) and close(total, speech * 2 * B * C * F * T)
    _, _, noise = O.residual_loss([five(clean)], [five(clean)], [five(noisy)], [0], 2, True, "both")
    assert close(R.msd(layout(clean), layout(noisy), 0, C, C)[0], noise)       # the noise term: the second half of the channels
    x = R.gen("normal", (6, 11), 10)
    assert close(R.mean_over_samples(x, 3), torch.mean(x.double().reshape(2, 3, 11), dim=1))


def test_gradients_are_those_of_the_values():
    """Central differences of the float64 values on a few coordinates (the gradients are autograd of the same functions)."""
    q1, q2 = R.gen_latent("mixed", 3, 2, 4, 11), R.gen_latent("plain", 3, 2, 4, 12)
    eps_r, eps_i = R.gen_eps(3, 2, 4, 2, 13)
    dz = R.gen("normal", (2, 3, 4, 4), 14).double()
    gr = R.reparam_bwd(q1, eps_r, eps_i, 2, dz)
    gk = R.ckl_bwd(q1, q2, 1e-9, 1.3)
    pick = dict(mr=("miu", 0), mi=("miu", 1), ls=("ls", 0), dr=("dl", 0), di=("dl", 1))
    h = 1e-6
    for part, (group, k) in pick.items():
        for idx in ((0, 0, 0), (2, 1, 3), (1, 1, 2)):
            def at(step, fn):
                q = R.dbl(q1)
                q[part] = q[part].clone()
                q[part][idx] += step
                return fn(q)
            f_r = lambda q: (R.reparam(q, eps_r, eps_i, 2) * dz).sum()
            f_k = lambda q: R.ckl(q, q2, 1e-9) * 1.3
            for f, g in ((f_r, gr), (f_k, gk)):
                fd = float(at(h, f) - at(-h, f)) / (2 * h)
                assert abs(fd - float(g[group][k][idx])) < 1e-6 * max(1.0, abs(fd)), (part, idx)


# ----------------------------------------------------------------------------- 2. the conditions of the GPU file's cases
def test_guard_decisions_are_safe_on_every_drawn_element():
    smallest = 1.0
    for name, c in R.LATENT_CASES.items():
        draws = [(k, G.latent(name, k)) for k in c["kinds"]] + [(k, G.latent(name, k, 1)) for k in R.Q2_KINDS if k]
        for kind, lat in draws:
            hit = torch.sqrt(lat["dr"].double() ** 2 + lat["di"].double() ** 2) >= torch.exp(lat["ls"].double()) - 1e-3
            if kind == "plain":
                assert not bool(hit.any())
            elif kind == "guarded":
                assert bool(hit.all())
            elif hit.numel() > 1:
                flat = hit.reshape(-1)
                assert not bool(flat[0::2].any()) and bool(flat[1::2].all())      # both branches inside one wave
            for e in (1e-6, c["eps"]):
                same, margin = R.guard_condition(lat, e)
                assert same and margin >= 1e-2, (name, kind, e, margin)
                smallest = min(smallest, margin)
    print(f"smallest |a - (sigma - 1e-3)| / sigma over all cases: {smallest:.3f}")


def test_case_tables_reach_what_they_are_for():
    G.test_every_entry_runs_past_its_grid_cap()
    cs = R.LATENT_CASES.values()
    assert {c["zdim"] for c in cs} >= {1, 5, 8} and {c["B"] for c in cs} >= {1, 3} and {c["T"] for c in cs} >= {1, 7}
    assert {c["ns"] for c in cs} == {1, 3} and {c["dTp"] for c in cs} == {1, 3} and {c["eps"] for c in cs} == {1e-9, 1e-10}
    for c in cs:
        (H1, o1, Tp, J, Jp1), (H2, o2, _, _, Jp2) = R.latent_layout(c), R.latent_layout(c, True)
        assert H1 != H2 and Jp1 != Jp2 and Jp2 > J and max(o1) + c["zdim"] <= H1 and max(o2) + c["zdim"] <= H2
    assert any(R.latent_layout(c)[4] > R.latent_layout(c)[3] for c in cs) and any(c["second"] for c in cs)
    assert {c[1] for c in R.WAVE_CASES.values()} == {1, 255, 257, 16385} and {c[0] for c in R.WAVE_CASES.values()} == {1, 6}
    assert {c[2] for c in R.WAVE_CASES.values()} == {1, 3} and all(c[3] > 0 and c[4] > 0 for c in R.WAVE_CASES.values())
    assert {c[5] for c in R.WAVE_CASES.values()} == {0, 1}
    ref_ld, est_ld, lens = R.RAGGED_CASE
    assert ref_ld != est_ld and set(lens) == {-3, 0, 1, min(ref_ld, est_ld), min(ref_ld, est_ld) + 5}
    assert {c[:3] for c in R.RECON_CASES.values()} == {(1, 1, 1), (4, 257, 9), (4, 257, 256)}
    assert {c[3] for c in R.RECON_CASES.values()} == {1, 2} and {c[4] for c in R.RECON_CASES.values()} == {"interleaved", "planar"}
    for Ca, Cb, ca0, cb0, C, F, B, T, Tp, pa, pb in R.MSD_CASES.values():
        assert Ca != Cb and ca0 > 0 and cb0 > 0 and pa != pb and T < Tp - 1 and ca0 + C <= Ca and cb0 + C <= Cb
    assert {c[0] for c in R.MEAN_CASES.values()} >= {1, 3, 4}


def test_the_noise_keeps_the_residual_off_its_clamp():
    for i, (name, (B, Ln, div, _, _, _)) in enumerate(R.WAVE_CASES.items()):
        if Ln == 1:
            continue                                               # one sample: the estimate is parallel to the source
        src, est = R.gen_waves("normal", B, Ln, div, 200 + i)
        E, D, Q = R.dots(src, est, div).unbind(1)
        en = Q - D * D / E
        assert float((en / Q).min()) > 1e-2, name


def test_exact_sums_stay_integers_below_2_53():
    for i, (name, (B, Ln, div, _, _, _)) in enumerate(R.WAVE_CASES.items()):
        w = R.dots(*R.gen_waves("exact", B, Ln, div, 200 + i), div)
        assert torch.equal(w, w.round()) and float(w.abs().max()) < 2 ** 53
    q1, q2 = R.gen_latent("exact", 5, 3, 7, 900), R.gen_latent("exact", 5, 3, 7, 901)
    sums = R.miu_dist(q1, q2)[1]
    assert torch.equal(sums, sums.round()) and float(sums.max()) > 0


# ----------------------------------------------------------------------------- 3. the bounds notice the mutants
def quantities(mut):
    """Every measured or derived comparison of the GPU file on its small cases, with the reference mutated -> a list of
    (what, errors against the unmutated reference, the bounds the GPU file asserts)."""
    out = []
    for name in R.SMALL:
        c = R.LATENT_CASES[name]
        zdim, B, T, ns, eps = c["zdim"], c["B"], c["T"], c["ns"], c["eps"]
        eps_r, eps_i = R.gen_eps(zdim, B, T, ns, 31 + list(R.LATENT_CASES).index(name))
        dz = R.gen("normal", (2, zdim, B * ns, T), 47)
        for kind in c["kinds"]:
            q1 = G.latent(name, kind)
            errs = R.worst_block(R.reparam(q1, eps_r, eps_i, ns, mut), R.reparam(q1, eps_r, eps_i, ns), R.Z_BLOCK)
            out.append((f"reparam {name} {kind}", errs, [G.bound("reparam", kind, G.TOL, k) for k in (0, 1)]))
            errs = R.latent_errors(R.reparam_bwd(q1, eps_r, eps_i, ns, dz, mut), R.reparam_bwd(q1, eps_r, eps_i, ns, dz))
            out.append((f"reparam_bwd {name} {kind}", errs, [G.bound("reparam_bwd", kind, G.GTOL, k) for k in (0, 1)]))
            for q2kind in R.Q2_KINDS:
                q2 = G.latent(name, q2kind, 1) if q2kind else None
                got, want = R.ckl(q1, q2, eps, mut), R.ckl(q1, q2, eps)
                out.append((f"ckl {name} {kind} {q2kind}", [G.rel(got, want)], [G.bound("ckl", f"{kind}/{q2kind}", G.TOL)]))
                errs = R.latent_errors(R.ckl_bwd(q1, q2, eps, 1.3, mut), R.ckl_bwd(q1, q2, eps, 1.3))
                out.append((f"ckl_bwd {name} {kind} {q2kind}", errs, [G.bound("ckl_bwd", f"{kind}/{q2kind}", G.GTOL, k) for k in (0, 1)]))
        q1, q2 = G.latent(name, "plain"), G.latent(name, "plain", 1)
        out.append((f"miu_dist {name}", [G.rel(R.miu_dist(q1, q2, mut)[0], R.miu_dist(q1, q2)[0])], [G.SUM_TOL]))
        errs = [R.worst_block(a, b, R.LATENT_BLOCK) for a, b in zip(R.miu_dist_bwd(q1, q2, 0.7, mut), R.miu_dist_bwd(q1, q2, 0.7))]
        out.append((f"miu_dist_bwd {name}", [max(e[k] for e in errs) for k in (0, 1)],
                    [G.bound("miu_dist_bwd", "plain", G.GTOL, k) for k in (0, 1)]))
    for i, (name, (B, Ln, div, _, _, _)) in enumerate(R.WAVE_CASES.items()):
        src, est = R.gen_waves("normal", B, Ln, div, 200 + i)
        out.append((f"sisnr {name}", [G.rel(R.si_snr(src, est, div, mut), R.si_snr(src, est, div))], [G.bound("sisnr", "normal", G.TOL)]))
        errs = R.worst_block(R.si_snr_bwd(src, est, div, 1.7, mut), R.si_snr_bwd(src, est, div, 1.7), R.WAVE_BLOCK)
        out.append((f"sisnr_bwd {name}", errs, [G.bound("sisnr_bwd", "normal", G.GTOL, k) for k in (0, 1)]))
    for i, (name, (B, F, T, div, _)) in enumerate(R.RECON_CASES.items()):
        if name == "r256":
            continue
        pred, ori = R.gen("normal", (B, F, T, 2), 400 + i), R.gen("normal", (B // div, F, T, 2), 401 + i)
        got, want = R.recon(pred, ori, div, mut), R.recon(pred, ori, div)
        out.append((f"recon cpx {name}", [G.rel(got[0], want[0])], [G.SUM_TOL]))
        out.append((f"recon mag {name}", [G.rel(got[1], want[1])], [G.bound("recon_mag", "normal", G.TOL)]))
        errs = R.worst_block(R.recon_bwd(pred, ori, div, 0.7, 1.3, mut), R.recon_bwd(pred, ori, div, 0.7, 1.3), R.SPEC_BLOCK)
        out.append((f"recon_bwd {name}", errs, [G.bound("recon_bwd", "normal", G.GTOL, k) for k in (0, 1)]))
    return out


# where each mutant has to show: a prefix of the comparison's name
MUTANT_SHOWS_IN = {
    "guard_scale": ("reparam ", "ckl "), "guard_sigma_path": ("reparam_bwd", "ckl_bwd"), "k_ir_dr": ("reparam ",),
    "mag_imag": ("recon mag", "recon_bwd"), "dsigma_no_sigma": ("reparam_bwd", "ckl_bwd"), "kl_logdet1_sign": ("ckl_bwd",),
    "src_div": ("sisnr ", "sisnr_bwd", "recon cpx"), "utterance": ("reparam ", "ckl ", "miu_dist ", "sisnr ", "recon cpx"),
}


def test_the_unmutated_reference_moves_nothing():
    assert all(e == 0 for _, errs, _ in quantities(None) for e in errs)


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_the_bounds_notice_the_mutant(mut):
    rows = quantities(mut)
    for prefix in MUTANT_SHOWS_IN[mut]:
        seen = [(what, errs, bounds) for what, errs, bounds in rows if what.startswith(prefix) and all(e > b for e, b in zip(errs, bounds))]
        most = max((max(errs) for what, errs, _ in rows if what.startswith(prefix)), default=0.0)
        print(f"{mut}: {len(seen)} comparisons of `{prefix.strip()}` notice it (largest movement {most:.2e})")
        assert seen, f"no comparison of `{prefix.strip()}` moves by more than its bound under the mutant {mut}"


# ----------------------------------------------------------------------------- 4. the refusals
def refusals(fn, good, bad):
    for kw in bad:
        a = dict(good, **kw)
        assert fn(*a.values(), None) == -1, kw


def pair(**kw):
    return dict(dict(q1=16, H1=24, Jp1=30, o1_miu=0, o1_ls=8, o1_dl=16, q2=16, H2=48, Jp2=32, o2_miu=24, o2_ls=32, o2_dl=40, zdim=8,
                     eps=1e-9, B=3, T=7, Tp=10), **kw)


BAD_PAIR = [dict(o1_miu=-1), dict(o1_ls=17), dict(o1_dl=24), dict(o2_miu=41), dict(o2_ls=-8), dict(o2_dl=48), dict(H1=23), dict(H2=47),
            dict(Tp=7), dict(Jp1=29), dict(Jp2=29), dict(zdim=0), dict(B=0), dict(T=0), dict(q1=None)]


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9          # the refusals are additive
    refusals(lib.idv_ckl, dict(pair(), work=16, out=16), BAD_PAIR + [dict(work=None), dict(out=None)])
    refusals(lib.idv_ckl_bwd, dict(pair(), gout=16, dq1=16), BAD_PAIR + [dict(gout=None), dict(dq1=None)])
    # q2 == NULL: its geometry is not looked at, q1's still is
    prior = dict(q2=None, H2=0, Jp2=0, o2_miu=0, o2_ls=0, o2_dl=0)
    refusals(lib.idv_ckl, dict(pair(**prior), work=16, out=16), [dict(o1_dl=17), dict(Tp=7), dict(Jp1=29)])
    refusals(lib.idv_ckl_bwd, dict(pair(**prior), gout=16, dq1=16), [dict(o1_dl=17), dict(Tp=7), dict(Jp1=29)])
    good = dict(q1=16, H1=24, Jp1=30, off1=0, q2=16, H2=48, Jp2=32, off2=24, zdim=8, B=3, T=7, Tp=10)
    bad = [dict(off1=-1), dict(off1=17), dict(off2=41), dict(off2=-1), dict(H1=7), dict(Tp=7), dict(Jp1=29), dict(Jp2=29), dict(zdim=0),
           dict(B=0), dict(T=0), dict(q1=None), dict(q2=None)]
    refusals(lib.idv_miu_dist, dict(good, work=16, out=16), bad + [dict(work=None), dict(out=None)])
    refusals(lib.idv_miu_dist_bwd, dict(good, gout=16, val=16, dq1=16, dq2=16), bad + [dict(gout=None), dict(val=None), dict(dq1=None, dq2=None)])
    good = dict(lat=16, Hl=24, off_miu=0, off_ls=8, off_dl=16, zdim=8, eps_r=16, eps_i=16, ns=2, B=3, T=7, Tp=10, Jp=30, z=16, Jpz=60)
    bad = [dict(off_miu=17), dict(off_ls=17), dict(off_dl=17), dict(Jpz=59), dict(zdim=0), dict(ns=0), dict(B=0), dict(T=0), dict(lat=None),
           dict(eps_r=None), dict(eps_i=None), dict(z=None)]
    refusals(lib.idv_reparam, good, bad)
    refusals(lib.idv_reparam_bwd, dict(good, dlat=16), bad + [dict(dlat=None)])      # z stands for dz
    wave = dict(src=16, src_ld=300, div=3, est=16, est_ld=257, B=6, L=257)
    bad = [dict(B=65536), dict(B=0), dict(L=0), dict(src_ld=256), dict(est_ld=256), dict(div=0), dict(src=None), dict(est=None)]
    refusals(lib.idv_sisnr, dict(wave, work=16, out=16), bad + [dict(work=None), dict(out=None)])
    refusals(lib.idv_sisnr_bwd, dict(wave, work=16, gout=16, dest=16), bad + [dict(work=None), dict(gout=None), dict(dest=None)])
    sdr = dict(ref=16, ref_ld=300, est=16, est_ld=257, B=6, L=257, work=16, out=16)
    refusals(lib.idv_sisdr, sdr, [dict(B=65536), dict(B=0), dict(L=0), dict(ref_ld=256), dict(est_ld=256), dict(ref=None), dict(out=None)])
    msd = dict(a=16, Ca=3, ca0=1, JpA=15, b=16, Cb=5, cb0=2, JpB=18, C=2, F=3, B=2, Tp=7, t_valid=4, work=16, out=16)
    refusals(lib.idv_msd, msd, [dict(C=128, Ca=200, Cb=200, F=256), dict(Ca=200, Cb=200, C=2, F=16384), dict(ca0=2), dict(cb0=4),
                                dict(JpA=13), dict(JpB=13), dict(t_valid=7), dict(t_valid=0), dict(a=None), dict(work=None)])
    assert lib.idv_msd(*dict(msd, C=1, F=32768).values(), None) == -1               # 2 C F = 65536, the first count refused
