"""Float64 reference of the latent and loss kernels -- idv_reparam (csrc/elementwise.hip), idv_ckl, idv_miu_dist, idv_sisnr,
idv_sisdr, idv_sisdr_ragged, idv_recon_loss, idv_msd, idv_mean_over_samples (csrc/reduce.hip) and their gradients idv_reparam_bwd,
idv_ckl_bwd, idv_miu_dist_bwd, idv_sisnr_bwd, idv_recon_loss_bwd (csrc/backward.hip) -- written from the formulas of
include/idccrn_hip.h and the reference lines the kernels cite.  Values are plain torch float64 on the fp32 inputs widened;
gradients are torch autograd of those same functions.  A plain module: it calls nothing of the package under test, runs on CPU
tensors and, given CUDA tensors, on the GPU.  It also holds the input generators, the per-block error measure, the mutants the
bounds have to notice, and the shapes the CPU and the GPU tests share.

A latent is a dict of five fp32 tensors [zdim, B, T]: mr, mi (mean), ls (log sigma), dr, di (delta).  In the planar layout its
channel groups sit at the offsets (o_miu, o_ls, o_dl) of the real plane set and, for mi and di, of the imaginary one.
tests/test_loss_ref_host.py checks this module on the CPU; tests/test_gpu_loss.py holds every entry to it."""
import math

import torch

from pw_ref import guard_mask, place_planar, read_planar  # noqa: F401  (re-exported for the tests)

PARTS = ("mr", "mi", "ls", "dr", "di")
# what a mutant changes (tests/test_loss_ref_host.py: every one must move a compared quantity by more than its bound)
MUTANTS = ("guard_scale", "guard_sigma_path", "k_ir_dr", "mag_imag", "dsigma_no_sigma", "kl_logdet1_sign", "src_div", "utterance")


def dbl(lat):
    return {k: v.double() for k, v in lat.items()}


# ----------------------------------------------------------------------------- the |delta| < sigma guard
def guard(sg, dr, di, e, mut=None):
    """pvae_module.py:1840-1845 (= pretrain_pvaes_loss.py:244-249, nsvae_loss.py:294-299): where a = sqrt(|delta|^2 + e) reaches
    sigma - 1e-3, delta is scaled to 0.99 sigma / (a + e)."""
    a = torch.sqrt(dr * dr + di * di + e)
    s = sg.detach() if mut == "guard_sigma_path" else sg
    scale = s * (1.0 if mut == "guard_scale" else 0.99) / (a + e)
    hit = a >= sg - 1e-3
    return torch.where(hit, dr * scale, dr), torch.where(hit, di * scale, di)


def guard_condition(lat, e):
    """-> (the decision a >= sigma - 1e-3 is the same in float32 and float64 on every element, the smallest
    |a - (sigma - 1e-3)| / sigma)."""
    ls, dr, di = lat["ls"], lat["dr"], lat["di"]
    a32 = torch.sqrt(dr * dr + di * di + torch.tensor(e, dtype=torch.float32))
    hit32 = a32 >= torch.exp(ls) - torch.tensor(1e-3, dtype=torch.float32)
    sg = torch.exp(ls.double())
    a = torch.sqrt(dr.double() ** 2 + di.double() ** 2 + e)
    return bool((hit32 == (a >= sg - 1e-3)).all()), float(((a - (sg - 1e-3)).abs() / sg).min())


# ----------------------------------------------------------------------------- values
def reparam(lat, eps_r, eps_i, ns, mut=None):
    """pvae_module.py:1832-1886 with the two draws given: eps_r, eps_i [B, ns, T, zdim] -> z float64 [2, zdim, B * ns, T]."""
    q, e = dbl(lat) if lat["ls"].dtype != torch.float64 else lat, 1e-6
    if mut == "utterance":
        eps_r, eps_i = eps_r.roll(1, 0), eps_i.roll(1, 0)
    sg = torch.exp(q["ls"])
    dr, di = guard(sg, q["dr"], q["di"], e, mut)
    a = torch.sqrt(dr * dr + di * di + e)
    den = torch.sqrt(2 * (sg + dr) + e)
    k_rr = (sg + dr) / (den + e)
    k_ir = (dr if mut == "k_ir_dr" else di) / (den + e)
    k_ii = torch.sqrt(sg * sg - a * a + e) / (den + e)
    er, ei = eps_r.double().permute(3, 0, 1, 2), eps_i.double().permute(3, 0, 1, 2)       # [zdim, B, ns, T]
    u = lambda v: v.unsqueeze(2)
    zr = u(q["mr"]) + u(k_rr) * er
    zi = u(q["mi"]) + u(k_ir) * er + u(k_ii) * ei
    zdim, B, _, T = er.shape
    return torch.stack((zr.reshape(zdim, B * ns, T), zi.reshape(zdim, B * ns, T)))


def ckl(q1, q2, eps, mut=None):
    """cal_kl_arbi_prior (pretrain_pvaes_loss.py:225-281) / cal_kl (nsvae_loss.py:275-328): mean over (b, t) of
    0.5 sum_h [coeff (trace + quad) + logdet2 - logdet1] - zdim;  q2 None: the standard prior (0, 0, 0)."""
    a = dbl(q1) if q1["ls"].dtype != torch.float64 else q1
    if q2 is None:
        z = torch.zeros_like(a["ls"])
        b = dict(mr=z, mi=z, ls=z, dr=z, di=z)
    else:
        b = dbl(q2)
    if mut == "utterance":
        a = dict(a, dr=a["dr"].roll(1, 1), di=a["di"].roll(1, 1))
    s1, s2 = torch.exp(a["ls"]), torch.exp(b["ls"])
    d1r, d1i = guard(s1, a["dr"], a["di"], eps, mut)
    d2r, d2i = guard(s2, b["dr"], b["di"], eps, mut)
    a1, a2 = d1r * d1r + d1i * d1i, d2r * d2r + d2i * d2i
    logdet1 = torch.log(0.25 * (s1 * s1 - a1) + eps)
    if mut == "kl_logdet1_sign":                                   # the value stays, the gradient through logdet1 flips
        logdet1 = 2 * logdet1.detach() - logdet1
    logdet2 = torch.log(0.25 * (s2 * s2 - a2) + eps)
    coeff = 2.0 / (s2 * s2 - a2 + eps)
    trace = s1 * s2 - d2r * d1r - d2i * d1i
    dr, di = b["mr"] - a["mr"], b["mi"] - a["mi"]
    quad = dr * dr * (s2 - d2r) - 2 * d2i * dr * di + di * di * (s2 + d2r)
    zdim, B, T = s1.shape
    return 0.5 * torch.sum(coeff * (trace + quad) + logdet2 - logdet1) / (B * T) - zdim


def miu_dist(q1, q2, mut=None):
    """miu_dis_loss (nsvae_loss.py:349-360) -> (sqrt(sum_{h, ri} mean_{b, t} (miu1 - miu2)^2), the sums [zdim, 2])."""
    a = dbl(q1) if q1["mr"].dtype != torch.float64 else q1
    b = dbl(q2) if q2["mr"].dtype != torch.float64 else q2
    if mut == "utterance":
        b = dict(b, mr=b["mr"].roll(1, 1), mi=b["mi"].roll(1, 1))
    sums = torch.stack((((a["mr"] - b["mr"]) ** 2).sum(dim=(1, 2)), ((a["mi"] - b["mi"]) ** 2).sum(dim=(1, 2))), dim=1)
    _, B, T = a["mr"].shape
    return torch.sqrt(sums.sum() / (B * T)), sums


def source_rows(src, B, src_div, mut=None):
    rows = torch.arange(B, device=src.device)
    return src[rows % src.shape[0] if mut == "src_div" else rows // src_div]


def dots(src, est, src_div=1, mut=None):
    """Per utterance (E, D, Q) = (<s, s>, <e, s>, <e, e>) -> float64 [B, 3]."""
    e = est.double()
    s = source_rows(src.double(), e.shape[0], src_div, mut)
    if mut == "utterance":
        s = s.roll(1, 0)
    return torch.stack(((s * s).sum(1), (e * s).sum(1), (e * e).sum(1)), dim=1)


def si_snr(src, est, src_div=1, mut=None, eps=1e-8):
    """sisnr_loss.py:7-19: -mean_b 10 log10(|s_t|^2 / (|e - s_t|^2 + eps) + eps), s_t = <e, s> s / (<s, s> + eps)."""
    e = est if est.dtype == torch.float64 else est.double()
    s = source_rows(src.double(), e.shape[0], src_div, mut)
    if mut == "utterance":
        s = s.roll(1, 0)
    s_t = (e * s).sum(1, keepdim=True) * s / ((s * s).sum(1, keepdim=True) + eps)
    e_n = e - s_t
    return -(10 * torch.log10((s_t * s_t).sum(1) / ((e_n * e_n).sum(1) + eps) + eps)).mean()


def si_sdr(ref, est, lens=None, eps=2.0 ** -23):
    """compute_sisdr (utils/eval_metrics.py:49-64) per utterance, eps = float32 machine epsilon -> float64 [B]; lens: only the
    first max(0, lens[b]) samples of row b count."""
    s, e = ref.double(), est.double()
    if lens is not None:
        n = min(s.shape[1], e.shape[1])
        keep = torch.arange(n, device=s.device)[None, :] < torch.as_tensor(lens, device=s.device)[:, None]
        zero = torch.zeros((), dtype=torch.float64, device=s.device)
        s, e = torch.where(keep, s[:, :n], zero), torch.where(keep, e[:, :n], zero)      # where, not *: what is cut may be NaN
    a = (eps + (s * e).sum(1, keepdim=True)) / ((s * s).sum(1, keepdim=True) + eps)
    return 10 * torch.log10((eps + ((a * s) ** 2).sum(1)) / (eps + ((e - a * s) ** 2).sum(1)))


def recon(pred, ori, ori_div=1, mut=None):
    """multiple_recon_loss (nsvae_loss.py:775-797): pred [B, F, T, 2], ori [B / ori_div, F, T, 2] -> (loss_cpx, loss_mag, the sum
    behind loss_cpx).  Each is a sum over F and a mean over (B, T); the original magnitude takes the real part twice (:783)."""
    p = pred if pred.dtype == torch.float64 else pred.double()
    o = source_rows(ori.double(), p.shape[0], ori_div, "src_div" if mut == "src_div" else None)
    if mut == "utterance":
        o = o.roll(1, 0)
    pr, pi, o_r, o_i = p[..., 0], p[..., 1], o[..., 0], o[..., 1]
    pmag = torch.sqrt(pr * pr + pi * pi + 1e-6)
    omag = torch.sqrt(o_r * o_r + (o_i * o_i if mut == "mag_imag" else o_r * o_r) + 1e-6)
    bt = p.shape[0] * p.shape[2]
    total = ((pr - o_r) ** 2 + (pi - o_i) ** 2).sum()
    return total / bt, ((pmag - omag) ** 2).sum() / bt, total


def msd(a, b, ca0, cb0, C):
    """One term of residual_loss (nsvae_loss.py:363-446): a [2, Ca, F, B, T], b [2, Cb, F, B, T] -> (mean, sum) of
    (a[:, ca0:ca0 + C] - b[:, cb0:cb0 + C])^2."""
    d = (a.double()[:, ca0:ca0 + C] - b.double()[:, cb0:cb0 + C]) ** 2
    return d.mean(), d.sum()


def mean_over_samples(x, ns):
    """test_se_cvaefinetune.py:309-311: x [B * ns, L] -> the mean over each utterance's ns rows, float64 [B, L]."""
    return x.double().reshape(-1, ns, x.shape[1]).mean(dim=1)


# ----------------------------------------------------------------------------- gradients: autograd of the functions above
def _leaves(lat):
    return {k: v.double().clone().requires_grad_(True) for k, v in lat.items()}


def _latent_grads(q, mut=None):
    """The .grad of the five leaves in the three channel groups: miu [2, ...], ls [1, ...], dl [2, ...]."""
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    if mut == "dsigma_no_sigma":                                   # d / d log sigma = sigma d / d sigma
        g["ls"] = g["ls"] / torch.exp(q["ls"].detach())
    return dict(miu=torch.stack((g["mr"], g["mi"])), ls=g["ls"][None], dl=torch.stack((g["dr"], g["di"])))


def reparam_bwd(lat, eps_r, eps_i, ns, dz, mut=None):
    """dz [2, zdim, B * ns, T] -> the gradient of sum(z * dz) in the three channel groups."""
    q = _leaves(lat)
    (reparam(q, eps_r, eps_i, ns, mut) * dz.double()).sum().backward()
    return _latent_grads(q, mut)


def ckl_bwd(q1, q2, eps, gout, mut=None):
    q = _leaves(q1)
    (ckl(q, q2, eps, mut) * gout).backward()
    return _latent_grads(q, mut)


def miu_dist_bwd(q1, q2, gout, mut=None):
    """-> (d / d miu1, d / d miu2), each [2, zdim, B, T]."""
    a, b = _leaves(q1), _leaves(q2)
    (miu_dist(a, b, mut)[0] * gout).backward()
    return torch.stack((a["mr"].grad, a["mi"].grad)), torch.stack((b["mr"].grad, b["mi"].grad))


def si_snr_bwd(src, est, src_div, gout, mut=None):
    e = est.double().clone().requires_grad_(True)
    (si_snr(src, e, src_div, mut) * gout).backward()
    return e.grad


def recon_bwd(pred, ori, ori_div, g_cpx, g_mag, mut=None):
    """g_cpx / g_mag None: that term sends no gradient."""
    p = pred.double().clone().requires_grad_(True)
    cpx, mag, _ = recon(p, ori, ori_div, mut)
    (cpx * (g_cpx or 0.0) + mag * (g_mag or 0.0)).backward()
    return p.grad


# ----------------------------------------------------------------------------- per-block error
def worst_block(got, want, dims):
    """Blocks: what is left of the shape after reducing over `dims`.  -> (the worst block's relative L2 error, the worst block's
    largest element error over its largest reference element).  A block whose reference is exactly zero must be exactly zero
    (else inf)."""
    g, w = got.double(), want.double()
    d = g - w
    l2, r2 = (d * d).sum(dim=dims), (w * w).sum(dim=dims)
    mx, rm = d.abs().amax(dim=dims), w.abs().amax(dim=dims)
    nz = r2 > 0
    if bool((l2[~nz] != 0).any()):
        return float("inf"), float("inf")
    if not bool(nz.any()):
        return 0.0, 0.0
    return float((l2[nz] / r2[nz]).max().sqrt()), float((mx[nz] / rm[nz]).max())


LATENT_BLOCK = (0, 1, 3)      # [parts, zdim, B, T]: a channel group of one utterance
Z_BLOCK = (1, 3)              # z [2, zdim, B * ns, T]: a part of one sampled utterance
WAVE_BLOCK = (1,)             # [B, L]: one row
SPEC_BLOCK = (2, 3)           # [B, F, T, 2]: one bin row of one utterance


def latent_errors(got, want):
    """Gradient dicts (miu, ls, dl) -> the worst (rel L2, max) over the channel group x utterance blocks."""
    errs = [worst_block(got[k], want[k], LATENT_BLOCK) for k in ("miu", "ls", "dl")]
    return max(e[0] for e in errs), max(e[1] for e in errs)


# ----------------------------------------------------------------------------- input generators (CPU draws, fixed seeds)
KINDS = ("plain", "guarded", "mixed")


def gen_latent(kind, zdim, B, T, seed):
    """plain: ls ~ 0.3 N(0, 1), delta = rho sigma e^{i phi} with rho in [0, 0.9] (guard off); guarded: rho in [1.05, 4] (guard
    on); mixed: the two alternating element by element; exact: integers in [-3, 3] everywhere (for the entries that read miu
    alone)."""
    g = torch.Generator().manual_seed(seed)
    shape = (zdim, B, T)
    if kind == "exact":
        return {k: torch.randint(-3, 4, shape, generator=g).float() for k in PARTS}
    ls = (0.3 * torch.randn(shape, generator=g, dtype=torch.float64)).float()
    u = torch.rand(shape, generator=g, dtype=torch.float64)
    lo, hi = 0.9 * u, 1.05 + 2.95 * u
    rho = {"plain": lo, "guarded": hi}.get(kind)
    if rho is None:
        rho = torch.where((torch.arange(zdim * B * T) % 2 == 0).reshape(shape), lo, hi)
    phi = 2 * math.pi * torch.rand(shape, generator=g, dtype=torch.float64)
    r = rho * torch.exp(ls.double())
    return dict(mr=torch.randn(shape, generator=g), mi=torch.randn(shape, generator=g), ls=ls,
                dr=(r * torch.cos(phi)).float(), di=(r * torch.sin(phi)).float())


def gen_eps(zdim, B, T, ns, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, ns, T, zdim, generator=g), torch.randn(B, ns, T, zdim, generator=g)


def gen(kind, shape, seed, scale=1.0):
    """exact: integers in [-3, 3]; normal: scale * N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        return torch.randint(-3, 4, shape, generator=g).float()
    return scale * torch.randn(shape, generator=g)


def gen_waves(kind, B, L, src_div, seed):
    """-> (src [B / src_div, L], est [B, L]); normal: est = src + 0.3 noise, which keeps |e - s_t|^2 away from its clamp."""
    src = gen(kind, (B // src_div, L), seed)
    if kind == "exact":
        return src, gen(kind, (B, L), seed + 1)
    return src, source_rows(src, B, src_div) + 0.3 * gen(kind, (B, L), seed + 1)


# ----------------------------------------------------------------------------- shapes shared by the CPU and the GPU tests
# Work-item counts past which an entry's grid stops growing and its stride loop runs (blocks x 256 threads, from the sources):
CAP_CKL = 1024 * 256          # idv_ckl: grid_for(B * zdim * T), cap 1024 (reduce.hip)
CAP_MIU = 16 * 256            # idv_miu_dist: grid_for(B * T, 16) per (h, ri) (reduce.hip)
CAP_ELEM = 8192 * 256         # idv_reparam (elementwise.hip) and every backward launch (backward.hip): cap 8192
CAP_WAVE = 64 * 256           # idv_sisnr / idv_sisdr / idv_sisdr_ragged / idv_sisnr_bwd: 64 blocks per row
CAP_RECON = 1024 * 256        # idv_recon_loss: grid_for(B * F * T), cap 1024; idv_recon_loss_bwd: cap 8192 (not reached)
CAP_MSD = 16 * 256            # idv_msd: 16 blocks per (part, c, f) row over the B * Tp columns
CAP_MEAN = 4096 * 256         # idv_mean_over_samples: grid_for(B * L, 4096)

# latent entries: zdim (= H, the group stride), B, T, ns, Tp - T, second (groups at (3H, 4H, 5H) of Hl = 6H, else (0, H, 2H) of
# Hl = 3H), pitch columns beyond J, eps of the KL, kinds
LATENT_CASES = {
    "one": dict(zdim=1, B=1, T=1, ns=1, dTp=1, second=False, pad=0, eps=1e-9, kinds=KINDS),
    "z5": dict(zdim=5, B=3, T=7, ns=3, dTp=3, second=True, pad=5, eps=1e-10, kinds=KINDS),
    "z8": dict(zdim=8, B=3, T=7, ns=1, dTp=1, second=False, pad=2, eps=1e-9, kinds=KINDS),
    "z8s": dict(zdim=8, B=1, T=7, ns=3, dTp=3, second=True, pad=4, eps=1e-10, kinds=KINDS),
    "kl_cap": dict(zdim=8, B=3, T=10923, ns=1, dTp=1, second=False, pad=3, eps=1e-9, kinds=("mixed",)),     # 262152 > CAP_CKL
    "miu_cap": dict(zdim=1, B=3, T=1366, ns=1, dTp=3, second=True, pad=1, eps=1e-10, kinds=("mixed",)),     # 4098 > CAP_MIU
    "elem_cap": dict(zdim=64, B=2, T=16385, ns=1, dTp=1, second=False, pad=4, eps=1e-9, kinds=("mixed",)),  # 2097280 > CAP_ELEM
}
Q2_KINDS = (None, "plain", "guarded")
# which cases an entry runs (every entry: all small ones and the case past its own cap)
SMALL = ("one", "z5", "z8", "z8s")
REPARAM_CASES = SMALL + ("elem_cap",)
CKL_CASES = SMALL + ("kl_cap", "elem_cap")
MIU_CASES = SMALL + ("miu_cap", "elem_cap")


def latent_layout(c, other=False):
    """-> (Hl, (o_miu, o_ls, o_dl), Tp, J, Jp) of a case's latent; other: the second latent of a pair entry, which takes the
    opposite channel layout and three more pitch columns (H1 != H2, Jp1 != Jp2)."""
    H, second = c["zdim"], c["second"] != other
    Tp = c["T"] + c["dTp"]
    J = c["B"] * Tp
    return (6 * H if second else 3 * H), ((3 * H, 4 * H, 5 * H) if second else (0, H, 2 * H)), Tp, J, J + c["pad"] + (3 if other else 0)


# idv_sisnr / idv_sisdr / idv_sisnr_bwd: B, L, src_div, src_ld - L, est_ld - L, floats off 16-byte alignment
WAVE_CASES = {
    "l1": (1, 1, 1, 3, 5, 1),
    "l255": (6, 255, 3, 2, 1, 0),
    "l257": (6, 257, 1, 7, 3, 1),
    "l16385": (6, 16385, 3, 1, 6, 0),                  # 16385 > CAP_WAVE
}
# idv_sisdr_ragged: ref_ld, est_ld, lens (Lmax = the shorter pitch)
RAGGED_CASE = (300, 257, (-3, 0, 1, 257, 262))
# idv_recon_loss / idv_recon_loss_bwd: B, F, T, ori_div, layout of ori
RECON_CASES = {
    "r1": (1, 1, 1, 1, "interleaved"),
    "r9p": (4, 257, 9, 2, "planar"),
    "r9i": (4, 257, 9, 1, "interleaved"),
    "r256": (4, 257, 256, 2, "planar"),                # 263168 > CAP_RECON
}
# idv_msd: Ca, Cb, ca0, cb0, C, F, B, T, Tp, JpA - J, JpB - J
MSD_CASES = {
    "small": (3, 5, 1, 2, 2, 3, 2, 4, 7, 1, 4),
    "wide": (2, 3, 1, 1, 1, 2, 3, 1366, 1370, 0, 5),   # B * Tp = 4110 > CAP_MSD
}
# idv_mean_over_samples: ns, B, L
MEAN_CASES = {"n1": (1, 2, 5), "n3": (3, 2, 257), "n2": (2, 3, 1000), "n4": (4, 2, 524289)}      # n4: 1048578 > CAP_MEAN


def cap_table():
    """(entry, work items of its case past the cap, the cap) -- asserted by both test files."""
    n = lambda name: LATENT_CASES[name]["B"] * LATENT_CASES[name]["zdim"] * LATENT_CASES[name]["T"]
    bt = lambda name: LATENT_CASES[name]["B"] * LATENT_CASES[name]["T"]
    r, m, v = RECON_CASES["r256"], MSD_CASES["wide"], MEAN_CASES["n4"]
    return [("idv_ckl", n("kl_cap"), CAP_CKL), ("idv_miu_dist", bt("miu_cap"), CAP_MIU), ("idv_reparam", n("elem_cap"), CAP_ELEM),
            ("idv_reparam_bwd", n("elem_cap"), CAP_ELEM), ("idv_ckl_bwd", n("elem_cap"), CAP_ELEM),
            ("idv_miu_dist_bwd", 2 * n("elem_cap"), CAP_ELEM), ("idv_sisnr / idv_sisdr / idv_sisnr_bwd", WAVE_CASES["l16385"][1], CAP_WAVE),
            ("idv_recon_loss", r[0] * r[1] * r[2], CAP_RECON), ("idv_msd", m[6] * m[8], CAP_MSD),
            ("idv_mean_over_samples", v[1] * v[2], CAP_MEAN)]
