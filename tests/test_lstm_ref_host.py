"""tests/lstm_ref.py is the reference of the GPU tests of the complex-LSTM kernel ladder (tests/test_gpu_lstm_ladder.py): here it
is checked itself, on the CPU -- its forward against the oracle, its hand-written back-propagation through time against
torch.autograd through the oracle -- and the inputs the GPU tests draw are shown to leave a float32 computation an order of
magnitude inside the bounds those tests assert."""
import pytest
import torch

import lstm_ref
from oracle import idccrn_oracle as O

SHAPES = [(16, 6, 4, 3), (32, 10, 1, 17)]             # H, I, T, B
TOL, GTOL = 2e-5, 2e-4                                 # what the GPU tests assert per block (forward / gradients)


def _rel(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


@pytest.mark.parametrize("H,I,T,B", SHAPES)
def test_forward_is_the_oracle(H, I, T, B):
    sd, x, _ = lstm_ref.make_case(H, I, T, B, seed=5)
    want = O.complex_lstm(x.double(), {k: v.double() for k, v in sd.items()}, "", 2)
    got = lstm_ref.forward(x, sd)
    assert got["out"].dtype == torch.float64 and got["out"].shape == (T, B, H, 2)
    assert got["gates"].shape == (2, 4, T, B, 4 * H) and got["c"].shape == got["h"].shape == (2, 4, T, B, H)
    assert _rel(got["out"], want) <= 1e-12
    # the saved activations are consistent with each other: h = o tanh(c), c_t = f c_{t-1} + i g
    g, c, h = got["gates"], got["c"], got["h"]
    assert _rel(g[..., 3 * H:] * torch.tanh(c), h) <= 1e-14
    cprev = torch.cat((torch.zeros_like(c[:, :, :1]), c[:, :, :-1]), dim=2)
    assert _rel(g[..., H:2 * H] * cprev + g[..., :H] * g[..., 2 * H:3 * H], c) <= 1e-14


@pytest.mark.parametrize("H,I,T,B", SHAPES)
def test_bptt_is_autograd_through_the_oracle(H, I, T, B):
    sd, x, R = lstm_ref.make_case(H, I, T, B, seed=6)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    (O.complex_lstm(x64, sd64, "", 2) * R.double()).sum().backward()
    saved = lstm_ref.forward(x, sd)
    got = lstm_ref.bptt(saved, R, sd)
    assert _rel(got["dx"], x64.grad) <= 1e-10
    assert sorted(got["grads"]) == sorted(lstm_ref.NAMES)
    for k in lstm_ref.NAMES:
        if T == 1 and "weight_hh" in k:                                 # no recurrence: exactly zero on both sides
            assert not sd64[k].grad.any() and not got["grads"][k].any(), k
            continue
        assert _rel(got["grads"][k], sd64[k].grad) <= 1e-10, k
    # float32 saved tensors are upcast: the same answer to float32 rounding of the inputs
    saved32 = {k: v.float() for k, v in saved.items()}
    got32 = lstm_ref.bptt(saved32, R, sd)
    assert got32["dx"].dtype == torch.float64 and _rel(got32["dx"], got["dx"]) <= 1e-5
    # a given gradient for layer 0 replaces dA1 W_ih1
    again = lstm_ref.bptt(saved, R, sd, dh0=got["dh0"])
    assert torch.equal(again["dA"], got["dA"]) and torch.equal(again["dx"], got["dx"])


def test_make_case_draws_what_the_module_test_draws():
    """The order of test_gpu_backward._clstm_grads: the parameters in nn.LSTM's order (lstm_re, then lstm_im), x, R."""
    H, I, T, B = 16, 6, 3, 2
    sd, x, R = lstm_ref.make_case(H, I, T, B, seed=11)
    g = torch.Generator().manual_seed(11)
    mods = {m: torch.nn.LSTM(input_size=I, hidden_size=H, num_layers=2) for m in lstm_ref.SETS}
    names = [f"{m}.{n}" for m in lstm_ref.SETS for n, _ in mods[m].named_parameters()]
    assert names == lstm_ref.NAMES
    for n in names:
        assert torch.equal(sd[n], torch.randn(*sd[n].shape, generator=g) * (1.0 / H ** 0.5)), n
    assert torch.equal(x, torch.randn(T, B, I, 2, generator=g)) and torch.equal(R, torch.randn(T, B, H, 2, generator=g))


def test_block_errors_sees_one_row_of_one_step():
    T, B, W = 5, 19, 8
    want = torch.randn(T, B, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    got = want.clone()
    got[3, 18] *= 1.01                                                  # the third row of the ragged last tile, one step
    worst, stray = lstm_ref.block_errors(got, want, B)
    rows = want[3, 16:19]
    assert stray == 0 and abs(worst - 0.01 * float(want[3, 18].norm() / rows.norm())) < 1e-12
    assert _rel(got, want) < worst / 4                                  # what the whole-tensor norm makes of it
    want[2, 16:] = 0
    got = want.clone()
    got[2, 17, 5] = 1e-30
    assert lstm_ref.block_errors(got, want, B) == (0.0, 1)
    assert lstm_ref.block_errors(want, want, B) == (0.0, 0)


# the largest cases of tests/test_gpu_lstm_ladder.py with the seeds it uses: (a) / (b) at the top batch of the ladder on an
# MI355X (16 * 15 + 1 sequences), (c) the same and the DCCRN-CL input width at the first batch of the second rung
@pytest.mark.parametrize("H,I,T,B,seed", [(128, 64, 5, 241, lstm_ref.LADDER_SEED), (128, 64, 5, 241, 11), (128, 1280, 5, 113, 11)])
def test_gpu_test_inputs_leave_float32_a_tenth_of_the_bounds(H, I, T, B, seed):
    """The reference itself in float32 (CPU), per (time step, 16-sequence tile) block against float64: every saved activation
    within TOL / 10, every gate gradient and dx within GTOL / 10.  A seed that misses this is replaced; the bounds stay."""
    sd, x, R = lstm_ref.make_case(H, I, T, B, seed)
    s64, s32 = lstm_ref.forward(x, sd), lstm_ref.forward(x, sd, dtype=torch.float32)
    assert s32["gates"].dtype == torch.float32
    worst = 0.0
    for k in ("gates", "c", "h"):
        for l in range(2):
            for r in range(4):
                e, stray = lstm_ref.block_errors(s32[k][l, r], s64[k][l, r], B)
                worst = max(worst, e)
                assert stray == 0 and e <= TOL / 10, (k, l, r, e)
    e, _ = lstm_ref.block_errors(s32["out"], s64["out"], B)
    assert e <= TOL / 10
    b64, b32 = lstm_ref.bptt(s64, R, sd), lstm_ref.bptt(s32, R, sd, dtype=torch.float32)
    assert b32["dA"].dtype == torch.float32
    gworst = 0.0
    for l in range(2):
        for r in range(4):
            e, stray = lstm_ref.block_errors(b32["dA"][l, r], b64["dA"][l, r], B)
            gworst = max(gworst, e)
            assert stray == 0 and e <= GTOL / 10, ("dA", l, r, e)
    e, stray = lstm_ref.block_errors(b32["dx"], b64["dx"], B)
    assert stray == 0 and e <= GTOL / 10, ("dx", e)
    print(f"float32 reference, worst block: activations {worst:.2e}, dA {gworst:.2e}, dx {e:.2e}")
