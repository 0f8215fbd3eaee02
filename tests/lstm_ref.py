"""Plain torch reference of the complex LSTM (reference model/complex_progress.py:50-74) as the recurrent kernels compute it --
csrc/lstm.hip, lstm_coop_f32.hip, lstm_stack2_f32.hip (training forward) and csrc/lstm_bwd.hip, lstm_bptt_coop_f32.hip,
lstm_bptt_stack2_f32.hip (back-propagation through time) -- with every intermediate the kernels save or overwrite, and the
per-block error the LSTM tests use.  A plain module: it calls nothing of the package under test, runs on CPU tensors, in float64
unless told otherwise.

Four real two-layer passes, run = 2 z + s with z the input part (0 real, 1 imaginary) and s the weight set (0 lstm_re, 1 lstm_im):

    out_re = run0 - run3            out_im = run2 + run1

Per layer and run, gates in torch's row order (i, f, g, o), h_{-1} = c_{-1} = 0:

    A_t = x_t W_ih^T + h_{t-1} W_hh^T + b_ih + b_hh        (i, f, o) = sigmoid(A), g = tanh(A)
    c_t = f c_{t-1} + i g                                   h_t = o tanh(c_t)

and backwards, t = T-1 .. 0, layer 1 then layer 0 (layer 0 receives dh_out = dA1 W_ih1):

    dh_t = dh_out[t] + dA_{t+1} W_hh                        dc_t = dc_{t+1} f_{t+1} + dh_t o_t (1 - tanh(c_t)^2)
    dA_t = (dc g i (1 - i), dc c_{t-1} f (1 - f), dc i (1 - g^2), dh tanh(c_t) o (1 - o))

tests/test_lstm_ref_host.py checks both against the oracle and torch.autograd through it."""
import torch

SETS = ("lstm_re", "lstm_im")
NAMES = [f"{m}.{n}_l{l}" for m in SETS for l in (0, 1) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
BLOCK = 16                                 # sequences per tile of every recurrent kernel
LADDER_SEED = 29                           # make_case seed of the kernel-boundary tests of tests/test_gpu_lstm_ladder.py


def make_case(H, I, T, B, seed):
    """Float32 parameters (scaled 1 / sqrt(H)), input x [T, B, I, 2] and output gradient R [T, B, H, 2], drawn from one generator
    in the order of test_gpu_backward._clstm_grads: the parameters of lstm_re, then lstm_im (nn.LSTM's order), x, R."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for m in SETS:
        for l in (0, 1):
            for n, shape in (("weight_ih", (4 * H, I if l == 0 else H)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)),
                             ("bias_hh", (4 * H,))):
                sd[f"{m}.{n}_l{l}"] = torch.randn(*shape, generator=g) * (1.0 / H ** 0.5)
    x = torch.randn(T, B, I, 2, generator=g)
    R = torch.randn(T, B, H, 2, generator=g)
    return sd, x, R


def _layer_fwd(xin, w_ih, w_hh, b):
    T, B, _ = xin.shape
    H = w_hh.shape[1]
    h = xin.new_zeros(B, H)
    c = xin.new_zeros(B, H)
    gx = xin @ w_ih.t() + b
    gates, cs, hs = [], [], []
    for t in range(T):
        a = gx[t] + h @ w_hh.t()
        i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        gates.append(torch.cat((i, f, g, o), dim=1))
        cs.append(c)
        hs.append(h)
    return torch.stack(gates), torch.stack(cs), torch.stack(hs)


def forward(x, sd, dtype=torch.float64):
    """x [T, B, I, 2] -> dict: x; gates [2 layers, 4 runs, T, B, 4H] (ACTIVATED i, f, g, o in torch's gate-row order);
    c, h [2, 4, T, B, H]; out [T, B, H, 2]."""
    x = x.detach().to(dtype)
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    gates, cs, hs = [[], []], [[], []], [[], []]
    for z in range(2):
        for s in range(2):
            inp = x[..., z]
            for l in range(2):
                m = SETS[s]
                g, c, h = _layer_fwd(inp, sd[f"{m}.weight_ih_l{l}"], sd[f"{m}.weight_hh_l{l}"],
                                     sd[f"{m}.bias_ih_l{l}"] + sd[f"{m}.bias_hh_l{l}"])
                gates[l].append(g)
                cs[l].append(c)
                hs[l].append(h)
                inp = h
    st = lambda q: torch.stack([torch.stack(r) for r in q])
    h = st(hs)
    out = torch.stack((h[1, 0] - h[1, 3], h[1, 2] + h[1, 1]), dim=-1)
    return {"x": x, "gates": st(gates), "c": st(cs), "h": h, "out": out}


def _layer_bwd(gates, c, dh_out, w_hh):
    T, B, H = c.shape
    dA = gates.new_zeros(T, B, 4 * H)
    dc_next = c.new_zeros(B, H)
    for t in range(T - 1, -1, -1):
        dh = dh_out[t] if t == T - 1 else dh_out[t] + dA[t + 1] @ w_hh
        i, f, g, o = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:3 * H], gates[t, :, 3 * H:]
        tc = torch.tanh(c[t])
        cprev = c[t - 1] if t > 0 else torch.zeros_like(c[0])
        dc = dc_next + dh * o * (1 - tc * tc)
        dA[t] = torch.cat((dc * g * i * (1 - i), dc * cprev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), dim=1)
        dc_next = dc * f
    return dA


def uncombine(dout):
    """dout [T, B, H, 2] -> the gradient arriving at layer 1's output per run, [4, T, B, H]."""
    return torch.stack((dout[..., 0], dout[..., 1], dout[..., 1], -dout[..., 0]))


def bptt(saved, dout, sd, dtype=torch.float64, dh0=None):
    """saved: forward()'s dict (any float type: a GPU forward's saved buffers, brought to this layout, are a valid input);
    dout [T, B, H, 2].  -> dict: dA [2 layers, 4 runs, T, B, 4H] (pre-activation gate gradients, torch's gate-row order),
    dh0 [4, T, B, H] (= dA1 W_ih1, the gradient arriving at layer 0's output), dx [T, B, I, 2], grads {name: gradient} of all
    16 parameters (bias_ih == bias_hh).  dh0: use this gradient for layer 0 in place of dA1 W_ih1."""
    x = saved["x"].to(dtype)
    gates, c, h = saved["gates"].to(dtype), saved["c"].to(dtype), saved["h"].to(dtype)
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    dout = dout.to(dtype)
    T, B, I, _ = x.shape
    H = c.shape[-1]
    dh1 = uncombine(dout)
    dA1 = torch.stack([_layer_bwd(gates[1, r], c[1, r], dh1[r], sd[f"{SETS[r & 1]}.weight_hh_l1"]) for r in range(4)])
    if dh0 is None:
        dh0 = torch.stack([dA1[r] @ sd[f"{SETS[r & 1]}.weight_ih_l1"] for r in range(4)])
    else:
        dh0 = dh0.to(dtype)
    dA0 = torch.stack([_layer_bwd(gates[0, r], c[0, r], dh0[r], sd[f"{SETS[r & 1]}.weight_hh_l0"]) for r in range(4)])
    dx = torch.stack([dA0[2 * z] @ sd["lstm_re.weight_ih_l0"] + dA0[2 * z + 1] @ sd["lstm_im.weight_ih_l0"] for z in range(2)], dim=-1)
    flat = lambda t: t.reshape(T * B, -1)
    prev = lambda t: torch.cat((torch.zeros_like(t[:1]), t[:-1]))             # h_{t-1}, h_{-1} = 0
    grads = {}
    for s, m in enumerate(SETS):
        runs = (s, 2 + s)                                                      # z = 0, 1
        grads[f"{m}.weight_ih_l1"] = sum(flat(dA1[r]).t() @ flat(h[0, r]) for r in runs)
        grads[f"{m}.weight_hh_l1"] = sum(flat(dA1[r]).t() @ flat(prev(h[1, r])) for r in runs)
        grads[f"{m}.bias_ih_l1"] = grads[f"{m}.bias_hh_l1"] = sum(flat(dA1[r]).sum(0) for r in runs)
        grads[f"{m}.weight_ih_l0"] = sum(flat(dA0[r]).t() @ flat(x[..., r >> 1]) for r in runs)
        grads[f"{m}.weight_hh_l0"] = sum(flat(dA0[r]).t() @ flat(prev(h[0, r])) for r in runs)
        grads[f"{m}.bias_ih_l0"] = grads[f"{m}.bias_hh_l0"] = sum(flat(dA0[r]).sum(0) for r in runs)
    return {"dA": torch.stack((dA0, dA1)), "dh0": dh0, "dx": dx, "grads": grads}


# ----------------------------------------------------------------------------- per-block error
def block_errors(got, want, B):
    """got, want [T, B, ...]: (worst relative L2 error over the (time step, 16-sequence tile) blocks against that block's
    reference norm, number of non-zero entries of `got` in blocks whose reference is exactly zero) -- the LSTM twin of
    wgrad_ref.worst_block_error: one wrong row of the ragged last tile of one step is not diluted by T * B."""
    T = want.shape[0]
    assert got.shape == want.shape and want.shape[1] == B, (got.shape, want.shape, B)
    got, want = got.detach().cpu().double().reshape(T, B, -1), want.detach().cpu().double().reshape(T, B, -1)
    nt = (B + BLOCK - 1) // BLOCK
    sq = lambda t: torch.cat((t * t, t.new_zeros(T, nt * BLOCK - B, t.shape[2])), dim=1).reshape(T, nt, -1).sum(-1)
    err, ref = sq(got - want), sq(want)
    nz = ref > 0
    worst = float((err[nz] / ref[nz]).max().sqrt()) if bool(nz.any()) else 0.0
    return worst, int(sq((got != 0).double())[~nz].sum())
