"""float64 reference of the train-mode ComplexBatchNormal + PReLU kernels (csrc/elementwise.hip, backward.hip, pack.hip, wgrad.hip)
and the case tables that tests/test_cbn_ref_host.py (CPU) and tests/test_gpu_cbn.py (MI355X) share.  Plain torch on the CPU.

An activation is [2, C, F, B, T] (real / imaginary, channel, bin row, utterance, frame): the kept columns 1 <= tp <= T of the planar
layout act[ri][C][F][Jp].  Forward (model/complex_progress.py:131-209 of the reference, pvae_module.py:64-68):
    sums [C][5] = sum r, i, rr, ii, ri;  moments [5][C] = mean_r, mean_i, Vrr + eps, Vri, Vii + eps;
    W = whitening matrix of V, Z = Gamma W, s = beta - Z mu, fold [C][6] = Zrr, Zri, Zir, Zii, sr, si;  u = Z y + s, z = PReLU(u).
The constants are those of cbn_finalize_kernel: eps = 1e-5 on Vrr and Vii, inside delta, inside ta and added to sq tt; delta is
clamped at 1e-8.  The forward takes u >= 0 as the positive PReLU branch, the gradient u > 0 (torch's convention)."""
from typing import NamedTuple

import torch

EPS, CLAMP = 1e-5, 1e-8
F64 = torch.float64


# ----------------------------------------------------------------------------- forward
def moment_sums(y):
    """y [2, C, F, B, T] -> [C][5] sums of r, i, rr, ii, ri over the kept columns."""
    r, i = y[0].double(), y[1].double()
    return torch.stack([t.sum(dim=(1, 2, 3)) for t in (r, i, r * r, i * i, r * i)], dim=1)


def moments_of(sums, count):
    """[C][5] sums -> moments [5][C]."""
    mr, mi = sums[:, 0] / count, sums[:, 1] / count
    return torch.stack((mr, mi, sums[:, 2] / count - mr * mr + EPS, sums[:, 4] / count - mr * mi, sums[:, 3] / count - mi * mi + EPS))


def whiten(Vrr, Vri, Vii):
    """-> Wrr, Wri, Wii of the inverse square root of [[Vrr, Vri], [Vri, Vii]] as the reference computes it."""
    sq = torch.clamp(Vrr * Vii - Vri * Vri + EPS, min=CLAMP).sqrt()
    tt = (Vrr + Vii + 2.0 * sq + EPS).sqrt()
    inv = 1.0 / (sq * tt + EPS)
    return (Vii + sq) * inv, -Vri * inv, (Vrr + sq) * inv


def fold(moments, gam, beta):
    """moments [5][C] (running or batch), gam = (g_rr, g_ri, g_ii), beta = (b_r, b_i) -> fold [C][6]: idv_cbn_fold."""
    mur, mui, Vrr, Vri, Vii = moments.double()
    Wrr, Wri, Wii = whiten(Vrr, Vri, Vii)
    grr, gri, gii = (g.double() for g in gam)
    Zrr, Zri = grr * Wrr + gri * Wri, grr * Wri + gri * Wii
    Zir, Zii = gri * Wrr + gii * Wri, gri * Wri + gii * Wii
    return torch.stack((Zrr, Zri, Zir, Zii, beta[0].double() - (Zrr * mur + Zri * mui), beta[1].double() - (Zir * mur + Zii * mui)), dim=1)


def finalize(sums, count, gam, beta, running=None, momentum=0.9):
    """idv_cbn_finalize -> (moments [5][C], running buffers [5][C] in the moments' order, fold [C][6]).  running None: the first
    call, which copies; else momentum old + (1 - momentum) new."""
    m = moments_of(sums.double(), count)
    return m, (m.clone() if running is None else momentum * running.double() + (1.0 - momentum) * m), fold(m, gam, beta)


def _col(t, k):
    return t[:, k].double().view(-1, 1, 1, 1)


def pre_activation(y, fo):
    """u = Z y + s, [2, C, F, B, T]."""
    yr, yi = y[0].double(), y[1].double()
    return torch.stack((_col(fo, 0) * yr + _col(fo, 1) * yi + _col(fo, 4), _col(fo, 2) * yr + _col(fo, 3) * yi + _col(fo, 5)))


def apply(y, fo, slope):
    """z = PReLU(Z y + s); slope None: the identity activation."""
    u = pre_activation(y, fo)
    return u if slope is None else torch.where(u >= 0, u, slope * u)


# ----------------------------------------------------------------------------- backward, closed form (the three kernels)
def du_of(dz, u, slope):
    return dz.double() if slope is None else torch.where(u > 0, dz.double(), slope * dz.double())


def bwd_sums(dz, y, fo, slope):
    """idv_cbn_bwd_reduce: [C][8] = sum du_r, du_i, du_r y_r, du_r y_i, du_i y_r, du_i y_i, the slope term sum dz u over u <= 0, 0."""
    u = pre_activation(y, fo)
    du, y = du_of(dz, u, slope), y.double()
    s = lambda t: t.sum(dim=(1, 2, 3))
    zero = torch.zeros(y.shape[1], dtype=F64)
    s6 = zero if slope is None else s(torch.where(u > 0, torch.zeros_like(u), dz.double() * u).sum(0))
    return torch.stack((s(du[0]), s(du[1]), s(du[0] * y[0]), s(du[0] * y[1]), s(du[1] * y[0]), s(du[1] * y[1]), s6, zero), dim=1)


def bwd_finalize(sums, count, moments, gam, scale=1.0):
    """idv_cbn_bwd_finalize -> dict(coef [C][12], dgamma_rr, dgamma_ri, dgamma_ii, dbeta_r, dbeta_i [C], dslope [1]) from the sums
    [C][8] and the forward's moments [5][C]; scale = param_grad_scale (not applied to coef)."""
    s, N = sums.double(), float(count)
    mur, mui, Vrr, Vri, Vii = moments.double()
    grr, gri, gii = (g.double() for g in gam)
    delta = Vrr * Vii - Vri * Vri + EPS
    clamped = delta < CLAMP
    sq = torch.where(clamped, torch.full_like(delta, CLAMP), delta).sqrt()
    tt = (Vrr + Vii + 2.0 * sq + EPS).sqrt()
    inv = 1.0 / (sq * tt + EPS)
    Wrr, Wii, Wri = (Vii + sq) * inv, (Vrr + sq) * inv, -Vri * inv
    Zrr, Zri, Zir, Zii = grr * Wrr + gri * Wri, grr * Wri + gri * Wii, gri * Wrr + gii * Wri, gri * Wri + gii * Wii
    Sr, Si = s[:, 0], s[:, 1]
    dZrr, dZri, dZir, dZii = s[:, 2] - mur * Sr, s[:, 3] - mui * Sr, s[:, 4] - mur * Si, s[:, 5] - mui * Si
    out = dict(dgamma_rr=scale * (dZrr * Wrr + dZri * Wri), dgamma_ri=scale * (dZrr * Wri + dZri * Wii + dZir * Wrr + dZii * Wri),
               dgamma_ii=scale * (dZir * Wri + dZii * Wii), dbeta_r=scale * Sr, dbeta_i=scale * Si, dslope=scale * s[:, 6].sum().view(1))
    dWrr, dWri, dWii = dZrr * grr + dZir * gri, dZrr * gri + dZri * grr + dZir * gii + dZii * gri, dZri * gri + dZii * gii
    # W(V) in reverse
    dinv = dWrr * (Vii + sq) + dWii * (Vrr + sq) - dWri * Vri
    dq = -dinv * inv * inv
    dta = dq * sq / (2.0 * tt)
    dsq = (dWrr + dWii) * inv + dq * tt + 2.0 * dta
    ddelta = torch.where(clamped, torch.zeros_like(dsq), dsq / (2.0 * sq))
    dVrr = dWii * inv + dta + ddelta * Vii
    dVii = dWrr * inv + dta + ddelta * Vrr
    dVri = -dWri * inv - 2.0 * ddelta * Vri
    zero = torch.zeros_like(Sr)
    out["coef"] = torch.stack((Zrr, Zri, Zir, Zii, 2.0 * dVrr / N, dVri / N, 2.0 * dVii / N, -(Zrr * Sr + Zir * Si) / N,
                               -(Zri * Sr + Zii * Si) / N, mur, mui, zero), dim=1)
    return out


def bwd_terms(dz, y, fo, coef, slope):
    """The terms of dy = Z^T du + A (y - mu) + c, idv_cbn_bwd_apply: ([5 terms of dy_r], [5 terms of dy_i]).  The PReLU branch is
    decided with the forward's fold, the value uses coef."""
    du = du_of(dz, pre_activation(y, fo), slope)
    cyr, cyi = y[0].double() - _col(coef, 9), y[1].double() - _col(coef, 10)
    one = torch.ones_like(cyr)
    return ([_col(coef, 0) * du[0], _col(coef, 2) * du[1], _col(coef, 4) * cyr, _col(coef, 5) * cyi, _col(coef, 7) * one],
            [_col(coef, 1) * du[0], _col(coef, 3) * du[1], _col(coef, 6) * cyi, _col(coef, 5) * cyr, _col(coef, 8) * one])


def bwd_apply(dz, y, fo, coef, slope):
    tr, ti = bwd_terms(dz, y, fo, coef, slope)
    return torch.stack((sum(tr[1:], tr[0]), sum(ti[1:], ti[0])))


def backward_closed(y, dz, gam, beta, slope, scale=1.0):
    """The whole backward through the three closed-form steps, from the batch statistics of y."""
    count = y[0].numel() // y.shape[1]
    m, _, fo = finalize(moment_sums(y), count, gam, beta)
    out = bwd_finalize(bwd_sums(dz, y, fo, slope), count, m, gam, scale)
    out["dy"] = bwd_apply(dz, y, fo, out["coef"], slope)
    if slope is None:
        out["dslope"] = None
    return out


def backward_autograd(y, dz, gam, beta, slope):
    """The same gradients by torch autograd in float64 through the forward above, with one shared slope parameter."""
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    y, gam, beta = leaf(y), [leaf(g) for g in gam], [leaf(b) for b in beta]
    sl = None if slope is None else leaf(torch.tensor(float(slope)))
    count = y[0].numel() // y.shape[1]
    u = pre_activation(y, fold(moments_of(moment_sums(y), count), gam, beta))
    z = u if sl is None else torch.where(u > 0, u, sl * u)
    (z * dz.double()).sum().backward()
    return dict(dy=y.grad, dgamma_rr=gam[0].grad, dgamma_ri=gam[1].grad, dgamma_ii=gam[2].grad, dbeta_r=beta[0].grad,
                dbeta_i=beta[1].grad, dslope=None if sl is None else sl.grad.view(1))


def bias_grad(sums):
    """cconv_bias_grad_kernel: the conv's real output carries b_re - b_im, the imaginary one b_re + b_im."""
    return sums[:, 0].double() + sums[:, 1].double(), sums[:, 1].double() - sums[:, 0].double()


def cconv(x, w_re, w_im, b_re, b_im):
    """The causal ComplexConv2d block (kernel (5, 2), stride (2, 1), padding (2, 1), last column dropped) in float64:
    x [2, Cin, F, B, T], w [Cout, Cin, 5, 2] -> [2, Cout, (F - 1) // 2 + 1, B, T]."""
    conv = lambda t, w: torch.nn.functional.conv2d(t.double().permute(2, 0, 1, 3), w.double(), None, (2, 1), (2, 1))[..., :-1]
    v = lambda b: b.double().view(1, -1, 1, 1)
    re = conv(x[0], w_re) - conv(x[1], w_im) + v(b_re) - v(b_im)
    im = conv(x[1], w_re) + conv(x[0], w_im) + v(b_re) + v(b_im)
    return torch.stack((re, im)).permute(0, 2, 3, 1, 4)


# ----------------------------------------------------------------------------- layout
def guard_mask(B, T, Tp, device="cpu"):
    """[B Tp] bool: the guard columns tp == 0 and T < tp < Tp."""
    tp = torch.arange(B * Tp, device=device) % Tp
    return (tp < 1) | (tp > T)


def place(plane, v, Tp):
    """v [2, C, F, B, T] onto the kept columns of plane [>= 2 C F rows][Jp]."""
    _, C, F, B, T = v.shape
    plane[:2 * C * F, :B * Tp].view(2 * C * F, B, Tp)[:, :, 1:1 + T] = v.reshape(2 * C * F, B, T).to(plane)


def read(plane, C, F, B, T, Tp):
    """The kept columns of plane as [2, C, F, B, T]."""
    return plane[:2 * C * F, :B * Tp].reshape(2, C, F, B, Tp)[..., 1:1 + T]


# ----------------------------------------------------------------------------- cases
class Case(NamedTuple):
    name: str
    kind: str           # "exact" or "normal"
    C: int
    F: int
    B: int
    T: int
    pad: int            # Tp = T + pad, 1 or 3
    spare: int          # Jp = B Tp rounded up to 4, plus this
    prelu: bool
    seed: int

    @property
    def Tp(self):
        return self.T + self.pad

    @property
    def Jp(self):
        return (self.B * self.Tp + 3) // 4 * 4 + self.spare

    @property
    def count(self):
        return self.B * self.F * self.T

    @property
    def slope(self):
        return SLOPE[self.kind] if self.prelu else None


SLOPE = {"exact": 0.25, "normal": 0.25}        # nn.PReLU's initial slope
# The smallest shapes that reach each mechanism: C = 1, C = 4 (one octet of the image twins) and C = 5 (c = row / F with F > 1);
# F and B in {1, 3}; T in {1, 2, 33}; Tp in {T + 1, T + 3}; a pitch with 8 spare columns; and one case per grid cap, where the
# kernels' stride loops run (16 x 256 columns in idv_cbn_stats / idv_cbn_bwd_reduce, 64 x 256 in the apply kernels).  A channel
# of the normal kind has B F T >= 9 elements: its own covariance is whitened.  The seeds are the first ones at which the
# conditions of tests/test_cbn_ref_host.py hold.
CASES = [
    Case("e_one", "exact", 1, 1, 1, 1, 1, 0, False, 0),
    Case("e_c4", "exact", 4, 1, 1, 2, 3, 0, True, 0),
    Case("e_c4_id", "exact", 4, 3, 1, 1, 1, 0, False, 0),
    Case("e_c5", "exact", 5, 3, 3, 2, 3, 0, True, 0),
    Case("e_c4_t33", "exact", 4, 3, 3, 33, 1, 8, True, 0),
    Case("e_cap16", "exact", 1, 1, 1, 4099, 1, 0, True, 0),
    Case("e_cap64", "exact", 1, 1, 1, 16387, 3, 0, True, 0),
    Case("e_cap64_c4", "exact", 4, 1, 1, 16389, 1, 0, True, 0),
    Case("n_c5", "normal", 5, 3, 3, 33, 3, 0, True, 0),
    Case("n_c4_t2", "normal", 4, 3, 3, 2, 1, 8, True, 0),
    Case("n_c4_t1", "normal", 4, 3, 3, 1, 3, 0, True, 3),
    Case("n_c4_f1", "normal", 4, 1, 3, 33, 1, 0, True, 0),
    Case("n_c1", "normal", 1, 1, 1, 33, 1, 0, False, 0),
]
BY_NAME = {c.name: c for c in CASES}
CHAIN = "n_c5"
# idv_cbn_finalize / idv_cbn_bwd_finalize alone: more than one 64-thread block of the first, the c += 256 loop of the second
FINALIZE_CASES = [Case("f_c5", "normal", 5, 1, 1, 48, 1, 0, True, 0), Case("f_c300", "normal", 300, 1, 1, 48, 1, 0, True, 10)]
# the replica path of one conv entry: cin, cout, F, T, B
CONV = dict(cin=2, cout=4, F=5, T=9, B=2, seed=3)
Z_SET = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0)


def _gen(case, salt):
    return torch.Generator().manual_seed(100003 * case.seed + 7919 * salt + sum(map(ord, case.name)))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def draw(case, salt=0):
    """-> dict of float64 tensors: y, dz [2, C, F, B, T] for both kinds.
    exact:  integers in [-3, 3]; fold [C][6] with Z from Z_SET and integer s; coef [C][12] of small integers (coef[11] = 0).
    normal: standard normal with a per-channel offset (up to 3), scale (in [0.5, 2]) and correlation of the two parts; channel 0
            has imag = 0.5 real + noise; gam = the model's initialisation (1 / sqrt 2, 0, 1 / sqrt 2) + 0.1 randn with
            |gamma_ri| >= 0.05, beta = 0.3 randn."""
    g = _gen(case, salt)
    C, shape = case.C, (case.C, case.F, case.B, case.T)
    if case.kind == "exact":
        d = dict(y=_ints(g, (2,) + shape, -3, 3), dz=_ints(g, (2,) + shape, -3, 3))
        Z = torch.tensor(Z_SET, dtype=F64)[torch.randint(0, len(Z_SET), (C, 4), generator=g)]
        d["fold"] = torch.cat((Z, _ints(g, (C, 2), -3, 3)), dim=1)
        d["coef"] = torch.cat((_ints(g, (C, 11), -2, 2), torch.zeros(C, 1, dtype=F64)), dim=1)
        return d
    n1, n2 = torch.randn(shape, generator=g, dtype=F64), torch.randn(shape, generator=g, dtype=F64)
    u = lambda lo, hi: (lo + (hi - lo) * torch.rand(C, generator=g, dtype=F64)).view(C, 1, 1, 1)
    sign = lambda: torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    off_r, off_i, scale = u(-3, 3), u(-3, 3), u(0.5, 2.0)
    rho = u(0.15, 0.35) * sign().view(C, 1, 1, 1)
    k = u(0.8, 1.25)
    re = n1
    im = k * (rho * n1 + (1 - rho * rho).sqrt() * n2)
    im[0] = 0.5 * n1[0] + 0.8 * n2[0]
    d = dict(y=torch.stack((off_r + scale * re, off_i + scale * im)), dz=torch.randn((2,) + shape, generator=g, dtype=F64))
    r = lambda: 0.1 * torch.randn(C, generator=g, dtype=F64)
    gri = r()
    gri = torch.where(gri.abs() < 0.05, 0.05 * sign(), gri)
    d["gam"] = (2.0 ** -0.5 + r(), gri, 2.0 ** -0.5 + r())
    d["beta"] = (3 * r(), 3 * r())
    return d


def draw_conv():
    """The exact conv case: x [2, cin, F, B, T] integers in [-3, 3], weights [cout, cin, 5, 2] and biases integers in [-2, 2]."""
    g = torch.Generator().manual_seed(CONV["seed"])
    cin, cout = CONV["cin"], CONV["cout"]
    return dict(x=_ints(g, (2, cin, CONV["F"], CONV["B"], CONV["T"]), -3, 3), w_re=_ints(g, (cout, cin, 5, 2), -2, 2),
                w_im=_ints(g, (cout, cin, 5, 2), -2, 2), b_re=_ints(g, (cout,), -2, 2), b_im=_ints(g, (cout,), -2, 2))


def cov_eigen(moments):
    """moments [5][C] -> (smaller, larger) eigenvalue of each channel's covariance."""
    _, _, Vrr, Vri, Vii = moments.double()
    h, r = 0.5 * (Vrr + Vii), (0.25 * (Vrr - Vii) ** 2 + Vri * Vri).sqrt()
    return h - r, h + r


def worst(got, want, dims):
    """The worst block of got against want, a block being what is left after reducing `dims`: the largest element error of a block
    over its largest reference magnitude -> (error, index of the block)."""
    got, want = got.double().cpu(), want.double()
    e = (got - want).abs().amax(dim=dims) if dims else (got - want).abs()
    m = want.abs().amax(dim=dims) if dims else want.abs()
    rel = (e / m.clamp_min(1e-300)).reshape(-1)
    rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
    k = int(rel.argmax()) if rel.numel() else 0
    return (float(rel[k]) if rel.numel() else 0.0), k
