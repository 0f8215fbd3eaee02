"""Float64 reference of the weight-gradient contractions (csrc/wgrad.hip, csrc/wgrad_bf16.hip), the Python mirror of their
split-K plan, and the shapes the weight-gradient tests share.  A plain module: it calls nothing of the package under test, runs
on CPU tensors and, given CUDA tensors, on the GPU.

Written from the formula in the header comment of wgrad.hip,

    G[kf][kt][s][l] = sum_{b, fs, t} S[b, s, fs, t] * L[b, l, 2 fs + kf - 2, t + kt + dt0]      (outside the tensor: zero)

with conv: S = dy, L = x, dt0 = tshift; transposed conv: S = x, L = dy, dt0 = 0; tshift = -1 if causal or transposed else 0 (what
ops.cconv_wgrad passes), and from  y_r = W_r x_r - W_i x_i,  y_i = W_r x_i + W_i x_r:

    dW_r = dy_r (x) x_r + dy_i (x) x_i          dW_i = dy_i (x) x_r - dy_r (x) x_i

tests/test_wgrad_ref_host.py checks it against float64 autograd through the oracle with exact integers."""
import torch


# ----------------------------------------------------------------------------- the contraction
def conv_wgrad_ref(x5, dy5, transposed, causal):
    """x5 [B, Cx, Fin, T, 2], dy5 [B, Cout, Fout, Tout, 2] -> (dw_re, dw_im) in float64, [Cout, Cx, 5, 2] (conv) or
    [Cx, Cout, 5, 2] (transposed conv).  One torch.matmul per tap."""
    x5, dy5 = x5.double(), dy5.double()
    tshift = -1 if (causal or transposed) else 0
    S, L, dt0 = (x5, dy5, 0) if transposed else (dy5, x5, tshift)
    B, Cs, Fs, Ts, _ = S.shape
    _, Cl, Fl, Tl, _ = L.shape
    # rows -2 .. 2 Fs and columns -1 .. Ts of L, zero outside the tensor
    Lz = L.new_zeros(B, Cl, max(Fl, 2 * Fs + 1) + 2, max(Tl, Ts + 1) + 1, 2)
    Lz[:, :, 2:2 + Fl, 1:1 + Tl] = L
    Sm = S.permute(4, 1, 0, 2, 3).reshape(2 * Cs, B * Fs * Ts)              # planes (re | im) x (b, fs, t)
    dw_re = S.new_zeros(Cs, Cl, 5, 2)
    dw_im = S.new_zeros(Cs, Cl, 5, 2)
    for kf in range(5):
        for kt in range(2):
            c0 = kt + dt0 + 1
            Lk = Lz[:, :, kf:kf + 2 * Fs:2, c0:c0 + Ts]                    # [B, Cl, Fs, Ts, 2]: L[2 fs + kf - 2, t + kt + dt0]
            Lm = Lk.permute(4, 1, 0, 2, 3).reshape(2 * Cl, B * Fs * Ts)
            G = torch.matmul(Sm, Lm.t())                                    # [2 Cs, 2 Cl]
            rr, ri, ir, ii = G[:Cs, :Cl], G[:Cs, Cl:], G[Cs:, :Cl], G[Cs:, Cl:]     # S re/im x L re/im
            dw_re[:, :, kf, kt] = rr + ii
            # conv: S = dy, dW_i = dy_i x_r - dy_r x_i = ir - ri;  transposed: S = x, dW_i = x_r dy_i - x_i dy_r = ri - ir
            dw_im[:, :, kf, kt] = (ri - ir) if transposed else (ir - ri)
    return dw_re, dw_im


def lstm_gate_row(m, H):
    """Row of torch's (gate * H + unit) layout for the planar row m in the recurrent kernels' gate order,
    colp = ((unit / 16) * 4 + gate) * 16 + unit % 16 within every set of 4 H rows (include/idccrn_hip.h)."""
    s, colp = divmod(m, 4 * H)
    ub, gate, ul = colp // 64, (colp // 16) % 4, colp % 16
    return s * 4 * H + gate * H + ub * 16 + ul


def pw_wgrad_ref(dout, x, shift, rowmap, H):
    """dout [M, J], x [K, J] -> dw [M, K] float64 with dw[rowmap(m)][k] = sum_j dout[m][j] * x[k][j + shift], x[.][-1] = 0."""
    dout, x = dout.double(), x.double()
    if shift == -1:
        x = torch.cat((x.new_zeros(x.shape[0], 1), x[:, :-1]), dim=1)
    elif shift != 0:
        raise ValueError("shift is 0 or -1")
    G = torch.matmul(dout, x.t())
    if rowmap == 1:
        rows = torch.tensor([lstm_gate_row(m, H) for m in range(G.shape[0])], device=G.device)
        out = torch.empty_like(G)
        out[rows] = G
        return out
    return G


# ----------------------------------------------------------------------------- per-block error
def block_sq(t, bs=16):
    """Sum of squares of every (bs S-side channels) x (bs L-side channels) block of t [Cs, Cl, ...], per trailing index (the
    taps of a conv gradient [Cs, Cl, 5, 2]; none for a point-wise gradient [M, K]) -> [nS, nL, ...]."""
    Cs, Cl, rest = t.shape[0], t.shape[1], tuple(t.shape[2:])
    nS, nL = (Cs + bs - 1) // bs, (Cl + bs - 1) // bs
    z = t.new_zeros(nS * bs, nL * bs, *rest)
    z[:Cs, :Cl] = t
    return (z * z).reshape(nS, bs, nL, bs, *rest).sum(dim=(1, 3))


def worst_block_error(got, want):
    """(worst relative L2 error over the blocks with a non-zero reference, number of non-zero entries of `got` in blocks whose
    reference is exactly zero)."""
    err, ref = block_sq(got.double() - want.double()), block_sq(want.double())
    nz = ref > 0
    worst = float((err[nz] / ref[nz]).max().sqrt()) if bool(nz.any()) else 0.0
    return worst, int((err[~nz] != 0).sum())


# ----------------------------------------------------------------------------- the split-K plan (mirror of make_plan_rounds)
WGRAD_MAX_ROUNDS = 4


def plan_rounds(Sp, Lp, J, MS, ML, JT, nprod, occ, spt, cus):
    """(nsplit, jtiles) of make_plan_rounds (csrc/wgrad_common.hpp) on a device of `cus` compute units; spt = steps per
    column tile (its argument Fs; 0: the plan with the most splits, which bounds the workspace)."""
    tiles = -(-Sp // MS) * -(-Lp // ML) * nprod
    jtiles, slots = -(-J // JT), cus * occ
    splits = lambda r: min(max(slots * r // tiles, 1), jtiles)
    if spt <= 0:
        return splits(WGRAD_MAX_ROUNDS), jtiles
    best = None
    for r in range(1, WGRAD_MAX_ROUNDS + 1):
        ns = splits(r)
        cost = float(-(-tiles * ns // slots)) * (float(jtiles * spt) / float(ns) + 16.0)
        if best is None or cost < best[0]:
            best = (cost, ns)
    return best[1], jtiles


def split_bounds(nsplit, jtiles, spt):
    """Split i owns the steps [b[i], b[i + 1]) of the flattened (column tile, row) sequence."""
    return [i * jtiles * spt // nsplit for i in range(nsplit + 1)]


def mid_tile_boundaries(bounds, spt):
    """Split boundaries strictly inside a column tile."""
    return sum(1 for b in bounds[1:-1] if b % spt)


# ----------------------------------------------------------------------------- shapes shared by the CPU and the GPU tests
# (transposed, Cx, Cout, Cin_total, ci_off, Fin, T, B, causal); Tp = T + 1 columns per utterance, J = B * Tp
FOUR_CASES = {
    "A1": (False, 1, 16, 1, 0, 17, 21, 3, True),          # skinny kernel, L = x, J = 66
    "A2": (True, 17, 1, 17, 0, 9, 300, 1, True),          # skinny kernel, L = dy, 34 S planes (ragged group of 4), two column splits
    "A3": (False, 24, 40, 24, 0, 9, 30, 3, True),         # one ragged S tile (80 planes), two L tiles (second ragged), J = 93
    "A4": (True, 72, 20, 100, 28, 4, 37, 2, True),        # two S tiles (second ragged), ci_off > 0, even Fin
    "A5": (False, 16, 16, 16, 0, 5, 9, 2, False),         # tshift = 0, dy has T - 1 frames
    "A6": (False, 96, 160, 96, 0, 9, 641, 2, True),       # mid-tile: J = 1284, 28 splits over 81 column tiles x 5 rows
    "A7t": (True, 8, 8, 8, 0, 1, 12, 2, True),            # one frequency row: only the tap kf = 2 is non-zero
    "A7c": (False, 8, 8, 8, 0, 1, 12, 2, True),
    "A8": (False, 8, 1, 8, 0, 9, 20, 2, True),            # one channel on the S side (MFMA kernel, 2 S planes)
}
GAUSS_CASES = {
    "G1": (True, 130, 40, 130, 0, 8, 30, 3, True),        # Winograd at the Fs = 8 threshold, even Fs, ragged S and L tiles, J = 93
    "G2": (True, 130, 40, 130, 0, 7, 30, 3, True),        # ten-product form just below the threshold
    "G3": (False, 32, 128, 32, 0, 17, 29, 2, True),       # Fs = 9: the last row pair is half empty
    "G3n": (False, 32, 128, 32, 0, 17, 29, 2, False),     # ... with tshift = 0
    "G4": (True, 256, 160, 300, 44, 9, 299, 2, True),     # mid-tile: Winograd, J = 600, 17 splits over 19 tiles x 5 row pairs
    "G5": (True, 256, 160, 300, 44, 5, 299, 2, True),     # mid-tile: ten-product form, 17 splits over 38 tiles x 5 rows
    "G6": (True, 128, 32, 128, 0, 10, 20, 2, True),       # even Fs above the threshold
}
BF16_CASES = {k: FOUR_CASES[k] for k in ("A3", "A4", "A5", "A6")}
BF16_CASES["B5"] = (True, 64, 32, 64, 0, 5, 31, 2, True)  # J % 4 = 0: no padding columns
MID_TILE = {"A6": ("four", 22), "G4": ("gauss", 13), "G5": ("gauss", 13)}      # boundaries inside a column tile at 256 CUs
# (M, K, J, shift, rowmap, H, accumulate, ldw)
PW_CASES = {
    "P1": (200, 72, 93, 0, 0, 0, 0, 72),
    "P2": (200, 72, 93, -1, 0, 0, 1, 77),                 # added to what dw holds; columns [K, ldw) stay
    "P3": (384, 64, 66, -1, 1, 48, 0, 64),                # gate-order rows, M = 2 * 4H
    "P4": (1536, 768, 1284, 0, 0, 0, 0, 768),             # several splits
    "P5": (128, 130, 35, 0, 1, 16, 1, 130),
}
ROWSUM_CASES = [(200, 93), (7, 1284)]
WINO_MIN_ROWS = 8


def conv_geometry(case):
    """-> (Cs, Cl, Fs, Fout, Tout, Tp, J) of a conv case."""
    transposed, cx, cout, _, _, fin, T, B, causal = case
    fout = 2 * fin - 1 if transposed else (fin - 1) // 2 + 1
    tout = T if causal else (T + 1 if transposed else T - 1)
    cs, cl, fs = (cx, cout, fin) if transposed else (cout, cx, fout)
    tp = max(T, tout) + 1
    return cs, cl, fs, fout, tout, tp, B * tp


def conv_plan_args(entry, case):
    """Arguments (Sp, Lp, J, MS, ML, JT, products, occupancy, steps per tile) the entry gives make_plan_rounds for a case, or
    None where it does not use that plan (the skinny kernel)."""
    cs, cl, fs, _, _, _, J = conv_geometry(case)
    if entry == "four":
        return None if 2 * cl <= 2 else (2 * cs, 2 * cl, J, 128, 32, 16, 1, 2, fs)
    wino = fs >= WINO_MIN_ROWS
    return (cs, cl, J, 128, 32, 32 if wino else 16, 3, 2, (fs + 1) // 2 if wino else fs)


def pw_plan_args(case):
    M, K, J = case[:3]
    return (M, K, J, 128, 128, 32, 1, 1, 1)


def all_plan_args():
    out = [conv_plan_args("four", c) for c in FOUR_CASES.values()] + [conv_plan_args("gauss", c) for c in GAUSS_CASES.values()]
    out += [pw_plan_args(c) for c in PW_CASES.values()]
    return [a for a in out if a is not None]
