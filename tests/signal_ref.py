"""Float64 reference of the kernels at the two ends of every model, between the waveform and the first or last conv block --
idv_stft_frames, idv_stft_frames_kimage, idv_istft_ola, idv_mask_apply, idv_outtype_estimate, idv_datanorm, idv_datadenorm,
idv_planar_to_complex (csrc/elementwise.hip, csrc/pw_bf16.hip), idv_make_dft (csrc/pack.hip) and the gradients
idv_stft_frames_bwd, idv_istft_ola_bwd, idv_mask_apply_bwd, idv_datanorm_bwd, idv_datadenorm_bwd, idv_complex_to_planar
(csrc/backward.hip) -- written from the definitions in include/idccrn_hip.h and the reference lines they cite, not from the
kernels.  Plain torch float64: it calls nothing of the package under test, runs on CPU tensors and, given CUDA tensors, on the
GPU.  It also holds the input generators and the case tables the CPU and the GPU tests share.
tests/test_signal_ref_host.py checks this module on the CPU against the oracle; tests/test_gpu_signal.py holds every entry to it.

Shapes: a waveform is [B, L]; frames are [win, B, T] (sample k of frame t of utterance b); a spectrum is [B, F, T, 2]."""
import math

import torch

from loss_ref import SPEC_BLOCK, WAVE_BLOCK, gen, worst_block  # noqa: F401  (re-exported for the tests)
from pw_ref import guard_mask, place_planar, planar_columns, read_planar  # noqa: F401

EPS_NORM = float(torch.tensor(1e-6, dtype=torch.float32))      # pvae_module.py:217-221 adds 1e-6 to an fp32 tensor
EPS_EST = float(torch.tensor(1e-10, dtype=torch.float32))      # test_se_cvaefinetune.py:85-135, likewise


def geometry(n_fft, win, hop):
    """-> (left, half, F): the window sits at [left, left + win) of an n_fft frame, the signal is padded by half."""
    return (n_fft - win) // 2, n_fft // 2, n_fft // 2 + 1


def n_frames(L, hop):
    return 1 + L // hop


# ----------------------------------------------------------------------------- framing and overlap-add
def frame_index(L, n_fft, win, hop, device=None):
    """long [win, T]: the sample of x that frames[k, ., t] = xp[hop t + left + k] reads, xp = reflect-pad(x, n_fft / 2)."""
    left, half, _ = geometry(n_fft, win, hop)
    k = torch.arange(win, device=device)[:, None]
    t = torch.arange(n_frames(L, hop), device=device)[None, :]
    s = (hop * t + left + k - half).abs()                          # mirrored about sample 0
    s = torch.where(s >= L, 2 * (L - 1) - s, s)                    # mirrored about sample L - 1
    assert int(s.min()) >= 0 and int(s.max()) < L
    return s


def frames(x, n_fft, win, hop):
    """x [B, L] -> float64 [win, B, T]."""
    idx = frame_index(x.shape[1], n_fft, win, hop, x.device)
    return x.double()[:, idx].permute(1, 0, 2)


def frames_adj(dfr, L, n_fft, win, hop):
    """The adjoint of frames(): dfr [win, B, T] -> float64 [B, L], a scatter-add through the same index table."""
    idx = frame_index(L, n_fft, win, hop, dfr.device)
    B = dfr.shape[1]
    dx = torch.zeros(B, L, dtype=torch.float64, device=dfr.device)
    dx.index_add_(1, idx.reshape(-1), dfr.double().permute(1, 0, 2).reshape(B, -1))
    return dx


def ola_sum(fr, n_fft, win, hop):
    """fr [win, B, T] -> float64 [B, hop (T - 1)]: sum_t fr[s + half - hop t - left, b, t], the overlap-add before the envelope."""
    left, half, _ = geometry(n_fft, win, hop)
    _, B, T = fr.shape
    tot = torch.zeros(B, n_fft + hop * (T - 1), dtype=torch.float64, device=fr.device)
    for t in range(T):
        tot[:, hop * t + left:hop * t + left + win] += fr[:, :, t].double().t()
    return tot[:, half:half + hop * (T - 1)]


def ola(fr, env_inv, n_fft, win, hop):
    """y[b, s] = env_inv[s + half] * ola_sum for s < hop (T - 1)."""
    half, Lout = n_fft // 2, hop * (fr.shape[2] - 1)
    return ola_sum(fr, n_fft, win, hop) * env_inv.double()[half:half + Lout]


def ola_adj_parts(dy, env_inv, T, n_fft, win, hop):
    """The two factors of the adjoint of ola(): (dy[b, hop t + left + k - half] or 0 outside [0, hop (T - 1)),
    env_inv[hop t + left + k]) -> ([win, B, T], [win, 1, T]) in the dtypes given."""
    left, half, _ = geometry(n_fft, win, hop)
    Lout = hop * (T - 1)
    p = hop * torch.arange(T, device=dy.device)[None, :] + left + torch.arange(win, device=dy.device)[:, None]      # [win, T]
    s = p - half
    inside = (s >= 0) & (s < Lout)
    g = dy[:, s.clamp(0, Lout - 1)].permute(1, 0, 2)
    return torch.where(inside[:, None, :], g, torch.zeros((), dtype=dy.dtype, device=dy.device)), env_inv[p][:, None, :]


def ola_adj(dy, env_inv, T, n_fft, win, hop):
    g, e = ola_adj_parts(dy.double(), env_inv.double(), T, n_fft, win, hop)
    return g * e


# ----------------------------------------------------------------------------- idv_make_dft
def dft_tables(n_fft, win, hop, T):
    """-> (w_fwd [2F, win], w_inv [win, 2F], env_inv [n_fft + hop (T - 1)]) float64: the periodic Hann window hann(win) at
    [left, left + win) of the frame, X[f] = sum_n w[n] x[n] e^{-2 pi i f (n + left) / n_fft}, the one-sided inverse with the
    weights 1, 2, ..., 2, 1 over n_fft times the window, and 1 / (overlap-added squared window), 0 where that is 0.  The phase
    f (n + left) is reduced modulo n_fft in integers (the exponential is periodic), so the angle carries one rounding."""
    left, _, F = geometry(n_fft, win, hop)
    n = torch.arange(win)
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * n.double() / win)
    ang = 2 * math.pi * ((torch.arange(F)[:, None] * (n + left)[None, :]) % n_fft).double() / n_fft               # [F, win]
    w_fwd = torch.cat((w * torch.cos(ang), -w * torch.sin(ang)))
    cf = torch.full((F, 1), 2.0, dtype=torch.float64)
    cf[0], cf[F - 1] = 1.0, 1.0
    w_inv = (torch.cat((torch.cos(ang) * cf, -torch.sin(ang) * cf)) * w / n_fft).t().contiguous()
    env = torch.zeros(n_fft + hop * (T - 1), dtype=torch.float64)
    for t in range(T):
        env[hop * t + left:hop * t + left + win] += w * w
    return w_fwd, w_inv, torch.where(env > 1e-11, 1.0 / env, torch.zeros_like(env))


def env_min(n_fft, win, hop, T):
    """The smallest squared-window envelope over the samples the ISTFT keeps."""
    left, half, _ = geometry(n_fft, win, hop)
    inv = dft_tables(n_fft, win, hop, T)[2][half:half + hop * (T - 1)]
    assert bool((inv > 0).all())
    return float(1.0 / inv.max())


def stft(x, n_fft, win, hop):
    """x [B, L] -> float64 [B, F, T, 2] = w_fwd applied to the frames."""
    F = n_fft // 2 + 1
    w_fwd = dft_tables(n_fft, win, hop, 1)[0].to(x.device)
    X = torch.tensordot(w_fwd, frames(x, n_fft, win, hop), dims=([1], [0]))       # [2F, B, T]
    return X.reshape(2, F, *X.shape[1:]).permute(2, 1, 3, 0)


def spec_rows(S):
    """[B, F, T, 2] -> the planar rows [2F, B, T]."""
    B, F, T, _ = S.shape
    return S.permute(3, 1, 0, 2).reshape(2 * F, B, T)


def rows_spec(R):
    """planar rows [2F, B, T] -> [B, F, T, 2]."""
    F = R.shape[0] // 2
    return R.reshape(2, F, *R.shape[1:]).permute(2, 1, 3, 0)


def istft(S, n_fft, win, hop):
    """S [B, F, T, 2] -> float64 [B, hop (T - 1)] = overlap-add of w_inv applied to the spectrum."""
    T = S.shape[2]
    _, w_inv, env_inv = (t.to(S.device) for t in dft_tables(n_fft, win, hop, T))
    return ola(torch.tensordot(w_inv, spec_rows(S.double()), dims=([1], [0])), env_inv, n_fft, win, hop)


# ----------------------------------------------------------------------------- the mask
def spectrum_rows(X, B, x_div):
    """X [B / x_div, ...] -> [B, ...]: row b reads the spectrum of utterance b / x_div."""
    return X[torch.arange(B, device=X.device) // x_div]


def mask(M, X, x_div=1):
    """pvae_module.py:224-234: P = tanh|M| X M / |M|, 0 at M = 0.  M [B, F, T, 2], X [B / x_div, F, T, 2] -> float64."""
    M, X = M.double(), spectrum_rows(X.double(), M.shape[0], x_div)
    mr, mi, xr, xi = M[..., 0], M[..., 1], X[..., 0], X[..., 1]
    mm = torch.sqrt(mr * mr + mi * mi)
    s = torch.where(mm > 0, torch.tanh(mm) / mm.clamp_min(1e-300), torch.zeros_like(mm))          # g / |M|
    return torch.stack((s * (xr * mr - xi * mi), s * (xr * mi + xi * mr)), dim=-1)


def mask_bwd(M, X, x_div, G):
    """The closed form of csrc/backward.hip with G = dL/dP, u = M / |M|, q = X u, g = tanh|M|:
        dL/dM = (g' - g / |M|) (G . q) u + (g / |M|) conj(X) G,   g' = 1 - g^2;   dL/dX = conj(g u) G  (before the sum over x_div).
    At M = 0 its limit: g / |M| -> 1, g' - g / |M| -> 0, so dL/dM = conj(X) G and dL/dX = 0.  -> (dM, dX) float64, dX per row of M."""
    M, X, G = M.double(), spectrum_rows(X.double(), M.shape[0], x_div), G.double()
    mr, mi, xr, xi, Gr, Gi = M[..., 0], M[..., 1], X[..., 0], X[..., 1], G[..., 0], G[..., 1]
    mm = torch.sqrt(mr * mr + mi * mi)
    nz = mm > 0
    safe = mm.clamp_min(1e-300)
    one, zero = torch.ones_like(mm), torch.zeros_like(mm)
    g = torch.tanh(mm)
    ur, ui = torch.where(nz, mr / safe, one), torch.where(nz, mi / safe, zero)
    h = torch.where(nz, g / safe, one)
    k = torch.where(nz, (1 - g * g) - h, zero)
    gq = Gr * (xr * ur - xi * ui) + Gi * (xr * ui + xi * ur)
    dM = torch.stack((k * gq * ur + h * (Gr * xr + Gi * xi), k * gq * ui + h * (Gi * xr - Gr * xi)), dim=-1)
    dX = torch.stack((g * (Gr * ur + Gi * ui), g * (Gi * ur - Gr * ui)), dim=-1)
    return dM, dX


# ----------------------------------------------------------------------------- the two-latent estimators
def estimator_means(speech, noise, ns):
    """[B ns, F, T, 2] -> the float64 means over each utterance's ns rows, (S, N) [B, F, T, 2]."""
    m = lambda v: v.double().reshape(-1, ns, *v.shape[1:]).mean(dim=1)
    return m(speech), m(noise)


def estimate(mode, speech, noise, X, ns):
    """test_se_cvaefinetune.py:85-135 from the float64 means: mode 0 real_and_imag_mask, 1 complex_mask, 2 phase_sensitive_mask
    -> float64 [B, F, T, 2]."""
    S, N = estimator_means(speech, noise, ns)
    X = X.double()
    if mode == 0:
        return S * S / (S * S + N * N + EPS_EST) * X
    s, n, x = torch.complex(S[..., 0], S[..., 1]), torch.complex(N[..., 0], N[..., 1]), torch.complex(X[..., 0], X[..., 1])
    if mode == 1:
        return torch.view_as_real(s / (s + n + EPS_EST) * x)
    sm, nm = s.abs(), n.abs()
    # |S| / (|S| + |N| + eps) cos(angle S - angle X) |X| e^{j angle S} = S Re(S conj X) / (|S| (|S| + |N| + eps)); 0 at S = 0
    g = torch.where(sm > 0, (s * x.conj()).real / (sm * (sm + nm + EPS_EST)).clamp_min(1e-300), torch.zeros_like(sm))
    return torch.view_as_real(g * s)


def gen_estimator(kind, B, ns, F, T, seed):
    """-> (speech, noise [B ns, F, T, 2], X [B, F, T, 2]) fp32.  Mode 1 divides by S + N + eps and every mode forms S and N as
    fp32 means, so two cancellations would amplify the rounding of those means without limit and no kernel could be held to a
    bound: S against N, and the ns samples of a mean against each other.  Neither can happen here: per bin, speech sample k is a
    freely drawn complex s times a real gain g_k > 0 (normal: in [0.5, 1.5]; exact: 1 or 2), so |S| = mean |s_k|; noise sample k
    is c times speech sample k with one complex c per bin, Re c >= 0, so N = c S and |S + N| = |1 + c| |S| >=
    (|S| + |N|) / sqrt(2) in exact arithmetic.  Mode 2 multiplies by cos(angle S - angle X) = Re(S conj X) / (|S| |X|), a sum of
    two products that cancels where S and X are orthogonal; a block of T = 1 is a single bin, so one such bin would be a whole
    block.  The noisy bin is therefore X = +-d s with one complex d per bin, |Im d| <= Re d: the angle between S and X stays
    within 45 degrees of 0 or 180, |cos| >= 1 / sqrt(2).  Where s = 0 (exact kind) X = d, so that the S = 0 branch still meets
    a non-zero X.  tests/test_signal_ref_host.py asserts all three conditions with margin on the values drawn."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, 1, F, T)
    rn = lambda: torch.randn(shape, generator=g, dtype=torch.float64)
    if kind == "exact":
        ri = lambda lo, hi, sh=shape: torch.randint(lo, hi, sh, generator=g).double()
        s = torch.complex(ri(-3, 4), ri(-3, 4))
        gain = ri(1, 3, (B, ns, F, T))
        c = torch.complex(ri(0, 3), ri(-2, 3))
        d = torch.complex(ri(1, 3), ri(-1, 2)) * (2 * ri(0, 2) - 1)
    else:
        s = torch.complex(rn(), rn())
        gain = 0.5 + torch.rand((B, ns, F, T), generator=g, dtype=torch.float64)
        c = torch.complex(rn().abs(), rn())
        phi = (math.pi / 4) * (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1)
        d = torch.polar(0.5 + torch.rand(shape, generator=g, dtype=torch.float64), phi) * torch.sign(rn())
    speech = torch.view_as_real(s * gain).float()                                       # [B, ns, F, T, 2]
    noise = torch.view_as_real(c * torch.view_as_complex(speech.double().contiguous())).float()
    X = torch.view_as_real(torch.where(s == 0, d, s * d)).float()
    return speech.reshape(B * ns, F, T, 2), noise.reshape(B * ns, F, T, 2), X.reshape(B, F, T, 2)


# ----------------------------------------------------------------------------- data normalisation
def _edge_bins(F, device):
    f = torch.arange(F, device=device)
    return ((f == 0) | (f == F - 1))[None, :, None]


def datanorm(X, mean, std):
    """pvae_module.py:217-221: (X - mean) / (std + 1e-6) per (bin, part), the imaginary part of bins 0 and F - 1 zeroed.
    X [B, F, T, 2], mean / std [F, 2] -> float64."""
    out = (X.double() - mean.double()[None, :, None, :]) / (std.double()[None, :, None, :] + EPS_NORM)
    out[..., 1] = torch.where(_edge_bins(X.shape[1], X.device), torch.zeros((), dtype=torch.float64, device=X.device), out[..., 1])
    return out


def datanorm_bwd(dout, std):
    dX = dout.double() / (std.double()[None, :, None, :] + EPS_NORM)
    dX[..., 1] = torch.where(_edge_bins(dout.shape[1], dout.device), torch.zeros((), dtype=torch.float64, device=dout.device), dX[..., 1])
    return dX


def datadenorm(P, mean, std):
    """pvae_module.py:235-238: std P + mean."""
    return std.double()[None, :, None, :] * P.double() + mean.double()[None, :, None, :]


def datadenorm_bwd(dout, dout_c, std):
    """std times the sum of the two upstream gradients (either may be None)."""
    g = sum(d.double() for d in (dout, dout_c) if d is not None)
    return std.double()[None, :, None, :] * g


def gen_stats(kind, F, seed):
    """-> (mean, std) [F, 2] fp32; std > 0 (exact: 1, 2 or 4, so that products and quotients of the exact kind stay short)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        return torch.randint(-3, 4, (F, 2), generator=g).float(), (2.0 ** torch.randint(0, 3, (F, 2), generator=g)).float()
    return torch.randn(F, 2, generator=g), 0.25 + torch.rand(F, 2, generator=g)


def gen_mask(kind, B, F, T, seed):
    """A mask [B, F, T, 2] with exact zeros: every element with (b + 2 f + 3 t) % 5 == 4, besides those the exact kind draws."""
    M = gen(kind, (B, F, T, 2), seed)
    b, f, t = torch.meshgrid(torch.arange(B), torch.arange(F), torch.arange(T), indexing="ij")
    M[(b + 2 * f + 3 * t) % 5 == 4] = 0.0
    return M


# ----------------------------------------------------------------------------- shapes shared by the CPU and the GPU tests
KINDS = ("exact", "normal")
CAP_ELEM = 8192 * 256          # every element-wise launch here: grid_for() stops at 8192 blocks of 256, then the stride loop runs
GEOMS = {"project": (512, 400, 100), "small": (64, 50, 12)}    # small: win % 8 != 0, win % hop != 0, left = 7
# L: the minimum n_fft / 2 + 1 (every sample but the last mirrored on the left, every one but the first on the right); one
# 32-frame tile with the longest-but-one tail; one frame in a second tile; the longest tail past the last hop
LENGTHS = {"project": (257, 3199, 3200, 3299), "small": (33, 383, 384, 395)}
BATCH_PITCH = ((1, 1), (3, 3), (1, 3), (3, 1))                 # (B, Tp - T): B Tp is and is not a multiple of 4
WAVE_CASES = {f"{g}-L{L}-B{B}-p{d}": dict(geom=GEOMS[g], L=L, B=B, dTp=d) for g in GEOMS for L in LENGTHS[g] for B, d in BATCH_PITCH}
ENV_T = (2, 3, 32, 33, 34)
ENV_MIN = {"project": 1.25, "small": 1.28}                     # what env_min() may not fall below over ENV_T

SPEC_CASES = {f"F{F}-T{T}-B{B}-p{d}": dict(F=F, T=T, B=B, dTp=d) for F in (1, 2, 5, 257) for T in (1, 2, 33) for B, d in BATCH_PITCH}
SPEC_CASES["F5-T2-B2-p3"] = dict(F=5, T=2, B=2, dTp=3)         # x_div = 2
SPEC_CASES["cap"] = dict(F=257, B=3, T=2800, dTp=1)            # 2158800 elements > CAP_ELEM
NS = (1, 2, 5)
ROUND_TRIP = dict(geom=GEOMS["project"], L=3299, B=3, dTp=3)


def x_divs(B):
    return [d for d in (1, 2, 3) if B % d == 0 and (d == 1 or d == B)]
