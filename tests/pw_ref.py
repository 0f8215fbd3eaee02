"""Float64 reference of the point-wise GEMM family (csrc/cgemm.hip idv_pw_gemm, csrc/pw_bf16.hip), the two output layouts, the
exact-arithmetic model of the bf16x3 split, the LSTM gate-row permutation, Python mirrors of the two host-side form choices, and
the shapes the point-wise tests share.  A plain module: it calls nothing of the package under test, runs on CPU tensors and,
given CUDA tensors, on the GPU.

    out[m][j] = bias[m] + sum_k W[m][k] x[k][j],   then optionally  y >= 0 ? y : slope * y

over the planar columns j = b * Tp + tp, valid for 1 <= tp <= t_valid (tp = t + 1; tp == 0 and tp > t_valid are guard columns).
tests/test_pw_ref_host.py checks this module on the CPU; tests/test_gpu_pw.py holds every entry to it."""
import torch


# ----------------------------------------------------------------------------- the contraction
def pw_ref(w, bias, x, slope=None):
    """w [M, K], bias [M] or None, x [K, ...] -> float64 [M, ...]: W @ x + bias, then PReLU with one slope (None: none)."""
    w, x = w.double(), x.double()
    y = torch.tensordot(w, x, dims=([1], [0]))
    if bias is not None:
        y = y + bias.double().reshape((-1,) + (1,) * (y.dim() - 1))
    if slope is not None:
        y = torch.where(y >= 0, y, float(slope) * y)
    return y


# ----------------------------------------------------------------------------- layouts
def planar_columns(B, T, Tp, device=None):
    """Column j = b * Tp + t + 1 of every valid (b, t) -> long [B, T]."""
    b = torch.arange(B, device=device)[:, None]
    t = torch.arange(T, device=device)[None, :]
    return b * Tp + t + 1


def place_planar(dst, v, Tp):
    """Write v [rows, B, T] into the planar rows dst [>= rows, Jp] (every other entry of dst stays)."""
    rows, B, T = v.shape
    dst[:rows, planar_columns(B, T, Tp, dst.device).reshape(-1)] = v.reshape(rows, B * T).to(dst.dtype)


def read_planar(src, rows, B, T, Tp):
    """The valid entries of planar rows src [>= rows, Jp] -> [rows, B, T]."""
    return src[:rows, planar_columns(B, T, Tp, src.device).reshape(-1)].reshape(rows, B, T)


def guard_mask(B, T, Tp, device=None):
    """bool [B * Tp]: True at the guard columns tp == 0 and tp > T."""
    m = torch.ones(B * Tp, dtype=torch.bool, device=device)
    m[planar_columns(B, T, Tp, device).reshape(-1)] = False
    return m


def read_rows(src, M, B, T, ldo):
    """Row-major store src[((tp - 1) * B + b) * ldo + m] (src [>= T * B, ldo]) -> [M, B, T]."""
    return src[:T * B].reshape(T, B, ldo)[:, :, :M].permute(2, 1, 0)


# ----------------------------------------------------------------------------- the bf16x3 arithmetic in exact numbers
def split(v):
    """fp32 v -> (hi, lo) as float64: hi = v with the low 16 bits cleared (a bf16 by truncation), lo = round-to-nearest-even
    bf16 of the fp32 difference v - hi (which is exact)."""
    v = v.float().contiguous()
    hi = (v.view(torch.int32) & -65536).view(torch.float32)
    lo = (v - hi).to(torch.bfloat16)
    return hi.double(), lo.double()


def split_model(w, x):
    """The value the bf16x3 kernels define for W @ x: w_lo x_hi + w_hi x_lo + w_hi x_hi with every product and sum in float64
    (a bf16 product has 16 significant bits: exact; the float64 sums stand for the exact ones).  No bias."""
    wh, wl = split(w)
    xh, xl = split(x)
    dot = lambda a, b: torch.tensordot(a, b, dims=([1], [0]))
    return dot(wl, xh) + dot(wh, xl) + dot(wh, xh)


# ----------------------------------------------------------------------------- LSTM gate rows
def lstm_rows(H):
    """long [8H]: the row of [lstm_re.weight_ih | lstm_im.weight_ih] (torch order gate * H + unit within each set of 4H) that
    the packed row m holds.  Within a set the packed column is colp = ((u / 16) * 4 + g) * 16 + u % 16; set 1 follows set 0."""
    m = torch.arange(8 * H)
    s, colp = m // (4 * H), m % (4 * H)
    ub, g, ul = colp // 64, (colp // 16) % 4, colp % 16
    return s * 4 * H + g * H + ub * 16 + ul


def lstm_stack(w_re, w_im, b_ih_re, b_hh_re, b_ih_im, b_hh_im, H):
    """-> (W [8H, K], b [8H]) in float64, rows in the packed (gate-column) order."""
    rows = lstm_rows(H).to(w_re.device)
    W = torch.cat((w_re.double(), w_im.double()))[rows]
    b = torch.cat((b_ih_re.double() + b_hh_re.double(), b_ih_im.double() + b_hh_im.double()))[rows]
    return W, b


def lstm_proj_ref(W, b, x_parts):
    """Layer-0 projection G[part] = W x[part] + b for x_parts [parts, K, ...] with (W, b) of lstm_stack -> [parts, 8H, ...]."""
    return torch.stack([pw_ref(W, b, xp) for xp in x_parts])


def lstm_proj1_ref(W, b, h_runs, H):
    """Layer-1 projection: run = 2 z + s reads h_runs[run] [H, ...] with weight set s -> [4 runs, 4H, ...]."""
    return torch.stack([pw_ref(W[(r & 1) * 4 * H:((r & 1) + 1) * 4 * H], b[(r & 1) * 4 * H:((r & 1) + 1) * 4 * H], h_runs[r])
                        for r in range(4)])


# ----------------------------------------------------------------------------- per-block error
def block_errors(got, want):
    """got, want [M, B, T] -> (worst relative L2 error of a 32-row tile over all valid columns, worst of an utterance over all
    rows).  A block whose reference is exactly zero must be exactly zero (else inf)."""
    d, w = (got.double() - want.double()) ** 2, want.double() ** 2
    M = d.shape[0]
    pad = (-M) % 32

    def worst(e, r):
        nz = r > 0
        if bool((e[~nz] != 0).any()):
            return float("inf")
        return float((e[nz] / r[nz]).max().sqrt()) if bool(nz.any()) else 0.0

    tile = lambda t: torch.nn.functional.pad(t.sum(dim=(1, 2)), (0, pad)).reshape(-1, 32).sum(dim=1)
    return worst(tile(d), tile(w)), worst(d.sum(dim=(0, 2)), w.sum(dim=(0, 2)))


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


# ----------------------------------------------------------------------------- mirrors of the host-side form choices
# Only ever compared with the library's queries (idv_pw_gemm_form, idv_pw_bf16_coltile) to assert coverage; no expectation of a
# result depends on them.
def gemm_form(M, swap, Jp, addr):
    """Digits <WM><WN><swap><vec> of idv_pw_gemm_form: 4 x 1 waves where the 32-row tiles come in whole blocks of 8, float4
    staging where the pitch is whole float4s and x is 16-byte aligned."""
    wm = 4 if ((M + 31) // 32) % 8 == 0 else 2
    return wm * 1000 + (1 if wm == 4 else 2) * 100 + (10 if swap else 0) + (1 if Jp % 4 == 0 and addr % 16 == 0 else 0)


def bf16_coltile(M, B, Tp):
    """idv_pw_bf16_coltile: 64 where that fills the last round of 256 workgroup slots better by more than 0.02, else 128."""
    mb, J = (M + 255) // 256, B * Tp

    def eff(jt):
        n = (J + jt - 1) // jt * mb
        return n / ((n + 255) // 256 * 256)
    return 64 if eff(64) > eff(128) + 0.02 else 128


GEMM_FORMS = {wm * 1000 + wn * 100 + s * 10 + v for wm, wn in ((2, 2), (4, 1)) for s in (0, 1) for v in (0, 1)}
BF16_FORMS = {(jt, kind) for jt in (64, 128) for kind in ("planar", "rows", "two-part")}

# ----------------------------------------------------------------------------- shapes shared by the CPU and the GPU tests
# idv_pw_gemm: (M, K, B, T, Tp, slope, ldo extra, lstm H); J = B * Tp
GEMM_CASES = {
    "tiny": (2, 2, 1, 1, 2, False, 0, 0),            # one k-step of a ragged chunk, one column
    "row33": (33, 6, 3, 7, 8, True, 0, 0),           # one row past a tile, K < 8, slope
    "j130": (130, 22, 2, 64, 65, False, 3, 0),       # 2 columns in the second 128-column tile, 2 rows in the second row block
    "rows96": (96, 256, 3, 37, 38, False, 0, 0),     # the reference shape of test_pw_bf16x3_rows_matches_the_fp32_swap_store
    "m250": (250, 10, 7, 17, 19, True, 0, 0),        # 4 x 1 form, M % 256 != 0, two trailing guard columns, J = 133, slope
    "m256": (256, 64, 5, 26, 27, False, 0, 0),       # 4 x 1 form, 64-column tile boundary inside an utterance
    "dft": (514, 400, 2, 33, 34, False, 0, 0),       # forward DFT rows: 17 row tiles
    "idft": (400, 514, 2, 33, 34, False, 0, 0),      # inverse DFT: K = 64 * 8 + 2
    "push": (512, 8, 16, 1, 2, False, 0, 0),         # one frame per push: every other column a guard column
    "lstm": (1024, 24, 2, 40, 41, False, 0, 128),    # idv_pack_lstm_ih weights, ldo = 8H
}
# idv_pw_bf16x3 / idv_pw_bf16x3_rows: (M, K, B, T, Tp)
BF16_CASES = {
    "tiny": (2, 6, 1, 1, 2),
    "row33": (33, 22, 3, 7, 8),
    "m257": (257, 64, 2, 64, 65),
    "dft": (514, 400, 2, 99, 100),
    "idft": (400, 514, 2, 33, 34),
    "m300": (300, 128, 5, 65, 66),
    "m40": (40, 70, 13, 59, 60),
}
BF16_NO_BIAS, BF16_WIDE_LDO = "row33", "m257"        # bias = NULL in the planar entry; ldo = M + 3 in the rows entry
# idv_lstm_proj_bf16x3: (H, K, B, T); idv_lstm_proj1_bf16x3: (H, B, T); Tp = T + 1
PROJ_CASES = {"h32k64": (32, 64, 3, 9), "h32k128": (32, 128, 12, 64)}
PROJ1_CASES = {"h64": (64, 3, 9)}
