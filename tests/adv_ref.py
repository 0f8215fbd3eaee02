"""float64 numpy restatement of the pieces the adversarial fine-tune adds (test_adversarial_host.py pins it to the reference's
float64 run in tests/golden/op_dis_mini.npz and grad_adv_mini.npz; test_gpu_adversarial.py may use it as a reference):

* the two-layer LSTM with hidden size 1 (torch.nn.LSTM(K, 1, 2) semantics: gate order i, f, g, o, zero initial state), forward and
  back-propagation through time;
* the two LSGAN losses of model/nsvae_loss.adversarial_second_phase_loss and their gradients.
"""
import numpy as np

NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1")


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _cell(pre, c):
    i, f, g, o = _sig(pre[:, 0]), _sig(pre[:, 1]), np.tanh(pre[:, 2]), _sig(pre[:, 3])
    c = f * c + i * g
    tc = np.tanh(c)
    return o * tc, c, (i, f, g, o, c, tc)


def lstm1_forward(x, w):
    """x [T, B, K], w: dict of the eight tensors -> (y [T, B, 1], tape)."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    x = np.asarray(x, dtype=np.float64)
    T, B, _ = x.shape
    G0 = x @ w["weight_ih_l0"].T + w["bias_ih_l0"] + w["bias_hh_l0"]            # [T, B, 4]
    h0 = c0 = h1 = c1 = np.zeros(B)
    y = np.zeros((T, B, 1))
    tape = []
    for t in range(T):
        h0p, c0p, h1p, c1p = h0, c0, h1, c1
        h0, c0, s0 = _cell(G0[t] + h0p[:, None] * w["weight_hh_l0"][:, 0], c0p)
        pre1 = h0[:, None] * w["weight_ih_l1"][:, 0] + h1p[:, None] * w["weight_hh_l1"][:, 0] + w["bias_ih_l1"] + w["bias_hh_l1"]
        h1, c1, s1 = _cell(pre1, c1p)
        y[t, :, 0] = h1
        tape.append((s0, s1, h0p, c0p, h1p, c1p, h0))
    return y, (x, w, tape)


def _cell_bwd(s, cprev, dh, dcn):
    i, f, g, o, _, tc = s
    dc = dh * o * (1.0 - tc * tc) + dcn
    dG = np.stack([dc * g * i * (1.0 - i), dc * cprev * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], axis=1)
    return dG, dc * f


def lstm1_backward(dy, tape):
    """dy [T, B, 1] -> (dx [T, B, K], dict of the eight parameter gradients)."""
    x, w, steps = tape
    T, B, K = x.shape
    dy = np.asarray(dy, dtype=np.float64)
    g = {k: np.zeros_like(v) for k, v in w.items()}
    dG0 = np.zeros((T, B, 4))
    dG0n = dG1n = np.zeros((B, 4))
    dc0n = dc1n = np.zeros(B)
    for t in range(T - 1, -1, -1):
        s0, s1, h0p, c0p, h1p, c1p, h0 = steps[t]
        dh1 = dy[t, :, 0] + dG1n @ w["weight_hh_l1"][:, 0]
        dG1, dc1n = _cell_bwd(s1, c1p, dh1, dc1n)
        dh0 = dG1 @ w["weight_ih_l1"][:, 0] + dG0n @ w["weight_hh_l0"][:, 0]
        dG0[t], dc0n = _cell_bwd(s0, c0p, dh0, dc0n)
        g["weight_hh_l1"][:, 0] += dG1.T @ h1p
        g["weight_ih_l1"][:, 0] += dG1.T @ h0
        g["bias_ih_l1"] += dG1.sum(0)
        g["weight_hh_l0"][:, 0] += dG0[t].T @ h0p
        g["bias_ih_l0"] += dG0[t].sum(0)
        dG0n, dG1n = dG0[t], dG1
    g["bias_hh_l0"], g["bias_hh_l1"] = g["bias_ih_l0"].copy(), g["bias_ih_l1"].copy()
    g["weight_ih_l0"] = dG0.reshape(T * B, 4).T @ x.reshape(T * B, K)
    return dG0 @ w["weight_ih_l0"], g


def distinguisher_loss(dis_true, dis_est):
    """mean((D(clean) - 1)^2 + D(estimate)^2) -> (loss, d/d dis_true, d/d dis_est)"""
    a, b = np.asarray(dis_true, dtype=np.float64), np.asarray(dis_est, dtype=np.float64)
    return float(np.mean((a - 1.0) ** 2 + b ** 2)), 2.0 * (a - 1.0) / a.size, 2.0 * b / b.size


def generator_dis_loss(dis_est):
    """mean((D(estimate) - 1)^2) -> (loss, d/d dis_est); generator_loss adds 0.5 of it to the SI-SNR."""
    a = np.asarray(dis_est, dtype=np.float64)
    return float(np.mean((a - 1.0) ** 2)), 2.0 * (a - 1.0) / a.size
