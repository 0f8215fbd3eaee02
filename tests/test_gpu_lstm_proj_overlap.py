"""The layer-0 input projection of the H = 128 complex LSTM inside the cooperative launch (csrc/lstm_stack2_f32.hip PROJ,
csrc/lstm_proj_split.hpp) against the hoisted projection (idv_pw_gemm in front of the launch; flags bit 4 of idv_clstm_fwd3).

Nothing in the arithmetic changes -- the tile is idv_pw_gemm's K loop over another column map -- so every comparison is
torch.equal: the output planes and every word of [G | h0 | h1] (evaluation) or of [G0 | G1 | h0 | h1 | c0 | c1] (training
forward: the activated gates of both layers and both cell-state buffers).  Shapes: K = 16, 20 (ragged K chunk of 8 planes) and
1280 once; B = 5 (one ragged tile), 16, 40 (ragged last tile), 64; T = 1, CH - 1, CH, CH + 1, 3 CH + 5; the opening phase forced
to 0 chunks (the recurrence waits for every chunk), 1, all (only the opening phase computes) and automatic; the headline shape
(B = 64, T = 641, K = 1280, automatic split) once; the forced-0 case 20 times over (every output equal to the first, every
status 0).  Work buffers have exactly the size their sizer reports, NaN-filled, with sentinels behind."""
import pytest
import torch

pytestmark = pytest.mark.gpu
H, CH, DEV = 128, 16, "cuda"
SENT, SENTV = 1024, -7.25
TS = (1, CH - 1, CH, CH + 1, 3 * CH + 5)

_PACKS, _X, _HOIST = {}, {}, {}


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def _packs(ops, K):
    if K not in _PACKS:
        g = torch.Generator().manual_seed(1000 + K)
        sd = {}
        for part in ("re", "im"):
            for l, kin in ((0, K), (1, H)):
                sd[f"lstm_{part}.weight_ih_l{l}"] = (torch.randn(4 * H, kin, generator=g) / kin ** 0.5).to(DEV)
                sd[f"lstm_{part}.weight_hh_l{l}"] = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(DEV)
                sd[f"lstm_{part}.bias_ih_l{l}"] = (torch.randn(4 * H, generator=g) * 0.1).to(DEV)
                sd[f"lstm_{part}.bias_hh_l{l}"] = (torch.randn(4 * H, generator=g) * 0.1).to(DEV)
        _PACKS[K] = (ops.pack_lstm(sd.__getitem__, H, K, 0, DEV), ops.pack_lstm(sd.__getitem__, H, H, 1, DEV))
    return _PACKS[K]


def _input(ops, K, B, T):
    if (K, B, T) not in _X:
        g = torch.Generator(device=DEV).manual_seed(K * 100003 + B * 1009 + T)
        x5 = torch.randn(B, K, 1, T, 2, generator=g, device=DEV) * 0.5
        _X[(K, B, T)] = ops.Planar.from_tensor5(x5, Tp=T + 3)                    # Tp is no multiple of 4 for most T
    return _X[(K, B, T)]


def _forward(ops, K, B, T, flags, c0):
    """-> (output planes, the saved region of the work buffer), both on the device; asserts status 0 and intact sentinels."""
    lib = ops.L.lib()
    p0, p1 = _packs(ops, K)
    x = _input(ops, K, B, T)
    train = bool(flags & 4)
    n = int((lib.idv_clstm_train_work_floats if train else lib.idv_clstm_work_floats)(H, B, T, x.Jp))
    work = torch.full((n + SENT,), float("nan"), dtype=torch.float32, device=DEV)
    work[n:] = SENTV
    out = ops.Planar.empty(H, 1, B, T, x.Tp, DEV)
    out.buf.fill_(float("nan"))
    ops.call("idv_clstm_fwd3", x.ptr(), ops.i(K), ops.p(p0.wih), ops.p(p0.bih), ops.p(p0.whh), ops.p(p1.wih), ops.p(p1.bih),
             ops.p(p1.whh), ops.p(p1.wih_hh), ops.i(H), ops.i(B), ops.i(T), ops.i(x.Tp), ops.i(x.Jp), ops.p(work), out.ptr(),
             ops.i(flags), ops.p(None), ops.i(c0), ops.stream_ptr())
    torch.cuda.synchronize()
    assert lib.idv_coop_last_status(1) == 0, f"K={K} B={B} T={T} flags={flags} c0={c0}: a cooperative launch timed out"
    assert bool((work[n:] == SENTV).all()), "sentinels behind the work buffer overwritten"
    saved = work[:(48 if train else 24) * T * B * H]
    assert bool(torch.isfinite(saved).all()) and bool(torch.isfinite(out.planes()[..., 1:T + 1]).all())
    return out.planes().clone(), saved


def _hoisted(ops, K, B, T, flags=0):
    k = (K, B, T, flags)
    if k not in _HOIST:
        _HOIST[k] = _forward(ops, K, B, T, flags | 16, -1)
    return _HOIST[k]


def _same(ops, K, B, T, c0, flags=0):
    lib = ops.L.lib()
    nch = -(-T // CH)
    force = nch if c0 == "all" else c0
    taken = lib.idv_lstm_stack2_f32_proj_split(H, B, T, K, force, None, None)
    assert taken == 1 or force == -1, (K, B, T, c0)              # a forced opening phase always runs the fused kernel
    want_out, want_saved = _hoisted(ops, K, B, T, flags)
    out, saved = _forward(ops, K, B, T, flags, force)
    what = f"K={K} B={B} T={T} opening={c0} flags={flags} (fused path taken: {taken})"
    assert torch.equal(saved, want_saved), f"{what}: saved buffers differ in {int((saved != want_saved).sum())} words"
    assert torch.equal(out, want_out), f"{what}: output differs"
    return taken


@pytest.mark.parametrize("B", (5, 16, 40, 64))
@pytest.mark.parametrize("K", (16, 20))
def test_fused_projection_has_the_bits_of_the_hoisted_one(ops, K, B):
    assert ops.L.lib().idv_lstm_stack2_f32_supported(H, B)
    taken = 0
    for T in TS:
        for c0 in (0, 1, "all", -1):
            taken += _same(ops, K, B, T, c0)
    assert taken >= 3 * len(TS)
    _HOIST.clear()
    _X.clear()


def test_full_depth_contraction(ops):
    _same(ops, 1280, 40, 3 * CH + 5, 1)
    _HOIST.clear()
    _X.clear()


def test_training_forward_keeps_gates_and_cell_states(ops):
    for c0 in (0, 1, -1):
        _same(ops, 20, 40, 3 * CH + 5, c0, flags=4)
    _HOIST.clear()


def test_headline_shape_automatic_split(ops):
    lib = ops.L.lib()
    assert _same(ops, 1280, 64, 641, -1) == 1 or lib.idv_coop_max_workgroups() < 129
    _HOIST.clear()
    _X.clear()
    torch.cuda.empty_cache()


def test_recurrence_waiting_for_every_chunk_repeats_its_bits(ops):
    K, B, T = 20, 40, 3 * CH + 5
    first = _forward(ops, K, B, T, 0, 0)
    for n in range(19):
        again = _forward(ops, K, B, T, 0, 0)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), f"call {n + 2} differs from the first"
    _X.clear()
