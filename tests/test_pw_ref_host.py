"""CPU tests behind the point-wise GEMM suite (tests/test_gpu_pw.py).

1. The float64 reference (tests/pw_ref.py) against torch.nn.functional.linear and the oracle's complex_dense, the two output
   layouts against their index formulas, the LSTM gate-row permutation against its formula and against nn.LSTM's own
   W_ih x + b_ih + b_hh.
2. The exact-arithmetic model of the bf16x3 split: integers in [-3, 3] have lo == 0 and the model equals the reference exactly;
   for standard-normal operands the model stays below the 2e-5 the GPU test asks of the kernels, so that bound is reachable by
   the arithmetic itself.
3. What the library decides on the host, with the library loaded and no GPU: the two form queries are declared, prototyped and
   exported and agree with the Python mirrors on a grid; every refusal of the five entries is IDV_EINVAL with dummy pointers,
   before any GPU work."""
import importlib
import itertools

import pytest
import torch

import pw_ref as R
from oracle import idccrn_oracle as O

LIB = importlib.import_module("i-dccrn-vae_amd._lib")
TOL = 2e-5


def ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).double()


# ----------------------------------------------------------------------------- the reference
def test_reference_equals_linear_and_the_oracle_dense():
    g = torch.Generator().manual_seed(1)
    M, K, B, T = 7, 10, 3, 5
    w, b, x = ints(g, M, K), ints(g, M), ints(g, K, B, T)
    y = R.pw_ref(w, b, x)
    assert y.dtype == torch.float64 and tuple(y.shape) == (M, B, T)
    assert torch.equal(y, torch.nn.functional.linear(x.permute(1, 2, 0), w, b).permute(2, 0, 1))
    assert torch.equal(R.pw_ref(w, None, x), torch.nn.functional.linear(x.permute(1, 2, 0), w).permute(2, 0, 1))
    s = R.pw_ref(w, b, x, 0.25)
    assert torch.equal(s, torch.where(y >= 0, y, 0.25 * y)) and bool((s != y).any())
    # ComplexDense: two independent real linears on the real and the imaginary part
    w_i, b_i = ints(g, M, K), ints(g, M)
    xc = ints(g, B, T, K, 2)
    want = O.complex_dense(xc, w, b, w_i, b_i)
    assert torch.equal(R.pw_ref(w, b, xc[..., 0].permute(2, 0, 1)), want[..., 0].permute(2, 0, 1))
    assert torch.equal(R.pw_ref(w_i, b_i, xc[..., 1].permute(2, 0, 1)), want[..., 1].permute(2, 0, 1))
    # normal operands: float32 inputs are widened, not rounded
    wn, xn = torch.randn(M, K, generator=g), torch.randn(K, 4, generator=g)
    assert torch.allclose(R.pw_ref(wn, None, xn), wn.double() @ xn.double(), rtol=0, atol=1e-14)


def test_layout_helpers_follow_the_index_formulas():
    B, T, Tp, rows, ldo = 3, 4, 6, 5, 7
    J, Jp = B * Tp, B * Tp + 2
    v = torch.arange(rows * B * T, dtype=torch.float64).reshape(rows, B, T) + 1
    buf = torch.full((rows + 1, Jp), -9.0, dtype=torch.float64)
    R.place_planar(buf, v, Tp)
    guard = R.guard_mask(B, T, Tp)
    assert int(guard.sum()) == B * (Tp - T)
    for r, b, t in itertools.product(range(rows), range(B), range(T)):
        assert buf[r, b * Tp + t + 1] == v[r, b, t] and not guard[b * Tp + t + 1]
    for b in range(B):
        assert guard[b * Tp] and guard[b * Tp + T + 1:(b + 1) * Tp].all()
    assert bool((buf[:rows, :J][:, guard] == -9.0).all()) and bool((buf[rows] == -9.0).all()) and bool((buf[:, J:] == -9.0).all())
    assert torch.equal(R.read_planar(buf, rows, B, T, Tp), v)
    flat = torch.full(((T * B + 2) * ldo,), -9.0, dtype=torch.float64)
    for m, b, t in itertools.product(range(rows), range(B), range(T)):
        flat[(t * B + b) * ldo + m] = v[m, b, t]                   # tp - 1 = t
    assert torch.equal(R.read_rows(flat.reshape(-1, ldo), rows, B, T, ldo), v)


@pytest.mark.parametrize("H", [16, 32, 48, 128])
def test_lstm_rows_is_a_bijection_with_the_documented_formula(H):
    rows = R.lstm_rows(H).tolist()
    assert sorted(rows) == list(range(8 * H))
    for s, gate, u in itertools.product(range(2), range(4), range(H)):
        assert rows[s * 4 * H + ((u // 16) * 4 + gate) * 16 + u % 16] == s * 4 * H + gate * H + u


def test_projection_reference_equals_the_lstm_input_rows_permuted():
    g = torch.Generator().manual_seed(2)
    H, K, B, T = 32, 6, 2, 3
    torch.manual_seed(3)
    re, im = torch.nn.LSTM(K, H).double(), torch.nn.LSTM(K, H).double()
    x = torch.randn(2, K, B, T, generator=g, dtype=torch.float64)
    W, b = R.lstm_stack(re.weight_ih_l0, im.weight_ih_l0, re.bias_ih_l0, re.bias_hh_l0, im.bias_ih_l0, im.bias_hh_l0, H)
    G = R.lstm_proj_ref(W, b, x).detach()
    assert tuple(G.shape) == (2, 8 * H, B, T)
    for part in range(2):
        for s, net in enumerate((re, im)):
            gates = (torch.einsum("mk,kbt->mbt", net.weight_ih_l0, x[part]) + (net.bias_ih_l0 + net.bias_hh_l0)[:, None, None]).detach()
            for gate, u in itertools.product(range(4), range(H)):
                got = G[part, s * 4 * H + ((u // 16) * 4 + gate) * 16 + u % 16]
                assert torch.allclose(got, gates[gate * H + u], rtol=0, atol=1e-14)
    # layer 1: run = 2 z + s takes weight set s
    W1, b1 = ints(g, 8 * H, H), ints(g, 8 * H)
    h = ints(g, 4, H, B, T)
    G1 = R.lstm_proj1_ref(W1, b1, h, H)
    for run in range(4):
        s = run % 2
        assert torch.equal(G1[run], R.pw_ref(W1[s * 4 * H:(s + 1) * 4 * H], b1[s * 4 * H:(s + 1) * 4 * H], h[run]))


# ----------------------------------------------------------------------------- the bf16x3 model
def test_split_of_small_integers_has_no_low_part_and_the_model_is_exact():
    g = torch.Generator().manual_seed(4)
    w, x = ints(g, 37, 70).float(), ints(g, 70, 11).float()
    for v in (w, x, 0.25 * w):
        hi, lo = R.split(v)
        assert torch.equal(hi, v.double()) and bool((lo == 0).all())
    assert torch.equal(R.split_model(w, x), R.pw_ref(w, None, x))


def test_split_is_truncation_then_nearest_even():
    v = torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -9, -(1.0 + 2.0 ** -8 + 2.0 ** -14 + 2.0 ** -23), 3.0e-3, 0.0])
    hi, lo = R.split(v)
    assert hi[0] == 1.0 + 2.0 ** -7 and lo[0] == 2.0 ** -9
    assert hi[1] == -1.0 and lo[1] == -(2.0 ** -8 + 2.0 ** -14)          # the 2^-23 bit is below lo's eight bits: rounded off
    assert bool((hi.abs() <= v.double().abs()).all())                    # truncation never grows the magnitude
    assert bool(((hi + lo - v.double()).abs() <= v.double().abs() * 2.0 ** -16).all())
    # a tie rounds to even: lo = 2^-9 (1 + 2^-8) lies half way between two bf16 neighbours
    t = torch.tensor([1.0 + 2.0 ** -9 + 2.0 ** -17])
    assert R.split(t)[1][0] == 2.0 ** -9


@pytest.mark.parametrize("K", [6, 22, 64, 400, 1280])
def test_split_model_reaches_the_forward_tolerance(K):
    g = torch.Generator().manual_seed(K)
    w, x = 0.1 * torch.randn(96, K, generator=g), torch.randn(K, 200, generator=g)
    err = R.rel_l2(R.split_model(w, x), R.pw_ref(w, None, x))
    print(f"split model against float64, K = {K}: {err:.2e} (bound {TOL:.0e})")
    assert 0 < err < TOL


def test_model_comparison_notices_a_truncated_lo_and_a_missing_cross_term():
    """What comparison (a) of the GPU test is for: a `lo` cut off instead of rounded, or one cross term dropped, moves the model
    by more than the largest bound that comparison asserts (4 x 2.28e-7, tests/test_gpu_pw.py MODEL_TOL)."""
    g = torch.Generator().manual_seed(7)
    w, x = 0.1 * torch.randn(96, 400, generator=g), torch.randn(400, 200, generator=g)
    (wh, wl), (xh, xl) = R.split(w), R.split(x)
    model = R.split_model(w, x)
    assert torch.equal(model, wl @ xh + wh @ xl + wh @ xh)
    cut = lambda v, hi: ((v.double() - hi).float().view(torch.int32) & -65536).view(torch.float32).double()
    truncated = cut(w, wh) @ xh + wh @ cut(x, xh) + wh @ xh
    assert R.rel_l2(truncated, model) > 2e-6 > 4 * 2.28e-7
    assert R.rel_l2(wh @ xl + wh @ xh, model) > 1e-4


def test_block_errors():
    want = torch.ones(40, 2, 3, dtype=torch.float64)
    got = want.clone()
    assert R.block_errors(got, want) == (0.0, 0.0)
    got[33, 1, 2] += 0.5                                   # second tile (8 rows x 6 columns), second utterance (40 x 3)
    tile, utt = R.block_errors(got, want)
    assert abs(tile - 0.5 / 48 ** 0.5) < 1e-15 and abs(utt - 0.5 / 120 ** 0.5) < 1e-15
    want[:32] = 0
    assert R.block_errors(got, want)[0] == float("inf")     # a non-zero entry where the reference tile is exactly zero


# ----------------------------------------------------------------------------- what the library decides on the host
def test_query_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name, proto in (("idv_pw_gemm_form", ("int", ["int", "int", "int", "ptr"])), ("idv_pw_bf16_coltile", ("int", ["int", "int", "int"]))):
        assert name in declared and protos[name] == proto and hasattr(lib, name)
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries


def test_queries_agree_with_the_mirrors():
    lib = LIB.lib()
    seen = set()
    for M in (1, 2, 32, 33, 96, 130, 224, 225, 250, 256, 257, 400, 480, 481, 512, 514, 1024, 1025, 3072):
        for swap, Jp, addr in itertools.product((0, 1, 7), (1, 2, 4, 133, 136, 1284), (4096, 4100, 4104, 4108, 4112, 4097)):
            got = lib.idv_pw_gemm_form(M, swap, Jp, addr)
            assert got == R.gemm_form(M, swap, Jp, addr), (M, swap, Jp, addr)
            seen.add(got)
        for B, Tp in itertools.product((1, 2, 3, 5, 12, 13, 16, 64, 256), (2, 8, 34, 60, 65, 66, 100, 642)):
            got = lib.idv_pw_bf16_coltile(M, B, Tp)
            assert got == R.bf16_coltile(M, B, Tp) and got in (64, 128), (M, B, Tp)
    assert seen == R.GEMM_FORMS
    assert lib.idv_pw_gemm_form(0, 0, 4, 16) == lib.idv_pw_gemm_form(4, 0, 0, 16) == -1
    assert lib.idv_pw_bf16_coltile(0, 1, 2) == lib.idv_pw_bf16_coltile(1, 0, 2) == lib.idv_pw_bf16_coltile(1, 1, 1) == -1


def test_case_tables_reach_the_forms_they_are_for():
    """With an aligned x and a float4 pitch; the GPU test asserts the same through the queries on its real buffers."""
    four = {k for k, c in R.GEMM_CASES.items() if R.gemm_form(c[0], 0, 4, 0) // 100 == 41}
    assert four == {"m250", "m256", "push", "lstm"}
    tiles = {k: R.bf16_coltile(c[0], c[2], c[4]) for k, c in R.BF16_CASES.items()}
    assert tiles == dict(tiny=128, row33=128, m257=128, dft=64, idft=128, m300=64, m40=64)
    assert [R.bf16_coltile(8 * H, B, T + 1) for H, _, B, T in R.PROJ_CASES.values()] == [128, 64]
    assert [R.bf16_coltile(4 * H, B, T + 1) for H, B, T in R.PROJ1_CASES.values()] == [128]
    for M, K, B, T, Tp, _, _, H in R.GEMM_CASES.values():
        assert K % 2 == 0 and Tp > T and (H == 0 or M == 8 * H)


def refusals(fn, order, good, bad):
    for kw in bad:
        a = dict(good, **kw)
        assert fn(*[a[k] for k in order], None) == -1, kw


def test_every_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    good = dict(x=16, K=8, wfrag=16, bias=16, slope=None, out=16, M=40, B=2, Tp=5, Jp=12, t_valid=4, swap=0, ldo=0)
    refusals(lib.idv_pw_gemm, list(good), good,
             [dict(x=None), dict(wfrag=None), dict(bias=None), dict(out=None), dict(K=0), dict(K=-2), dict(K=7), dict(M=0), dict(M=-1),
              dict(B=0), dict(Tp=1), dict(Tp=0), dict(t_valid=0), dict(t_valid=-1), dict(Jp=9), dict(swap=1, ldo=39), dict(swap=1, ldo=0),
              dict(swap=2, ldo=-40)])
    good = dict(ximg=16, lo=64, K=8, wfrag=16, bias=16, out=16, M=40, B=2, Tp=5, Jp=12, t_valid=4)
    refusals(lib.idv_pw_bf16x3, list(good), good,
             [dict(ximg=None), dict(wfrag=None), dict(out=None), dict(K=0), dict(M=0), dict(B=0), dict(Tp=1), dict(t_valid=0),
              dict(t_valid=-3), dict(Jp=9), dict(ximg=24), dict(ximg=20)])
    good = dict(ximg=16, lo=64, K=8, wfrag=16, bias=16, out=16, M=40, ldo=40, B=2, T=4, Tp=5, Jp=12)
    refusals(lib.idv_pw_bf16x3_rows, list(good), good,
             [dict(ximg=None), dict(wfrag=None), dict(bias=None), dict(out=None), dict(K=0), dict(M=0), dict(ldo=39), dict(B=0), dict(T=0),
              dict(Tp=4), dict(Jp=9), dict(ximg=24)])
    good = dict(ximg=16, lo=64, K=64, wfrag=16, bias=16, G=16, H=32, B=2, T=4, Tp=5, Jp=12)
    refusals(lib.idv_lstm_proj_bf16x3, list(good), good,
             [dict(ximg=None), dict(wfrag=None), dict(bias=None), dict(G=None), dict(H=0), dict(H=16), dict(K=32), dict(K=0), dict(B=0),
              dict(T=0), dict(Tp=4), dict(Jp=9), dict(ximg=24)])
    good = dict(himg=16, lo=64, wfrag=16, bias=16, G1=16, H=64, B=2, T=4, Tp=5, Jp=12)
    refusals(lib.idv_lstm_proj1_bf16x3, list(good), good,
             [dict(himg=None), dict(wfrag=None), dict(bias=None), dict(G1=None), dict(H=0), dict(H=32), dict(H=96), dict(B=0), dict(T=0),
              dict(Tp=4), dict(Jp=9), dict(himg=24)])
