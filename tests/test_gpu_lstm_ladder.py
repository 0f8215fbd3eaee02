"""The complex LSTM at H = 128 (DCCRN-CL bottleneck) picks its kernels by batch size; every rung is a kernel family of its own:

    16-sequence tiles        training / evaluation forward                        back-propagation through time
    32 tiles <= max          lstm_stack2_f32.hip (both layers, one launch)        lstm_bptt_stack2_f32.hip
    16 tiles <= max          lstm_coop_f32.hip per layer + gemm_rm_kernel<4>      lstm_bptt_coop_f32.hip per layer + dh0 GEMM
    above                    one-CU lstm_rec_kernel<true>                         lstm_step_bwd_kernel<2>, one launch per step

(max = idv_coop_max_workgroups(), 240 on an MI355X: batches <= 112, 113 .. 240, >= 241.)  Here every rung runs at the batches
where the ladder changes rung -- all tiles full, a last tile of one row, a ragged last tile at the widest grid -- and at T = 1 (no
recurrence; the layer that runs one step behind has a single step), 2 (both parities of the exchange buffers) and 5:

(a) the training forward through idv_clstm_fwd2 as autograd.LstmFn.forward calls it, the test choosing the rung: every saved
    activation (gates, c, h of both layers and four runs) against tests/lstm_ref.py in float64;
(b) the BPTT entries called directly on the saved buffers of one such forward, against lstm_ref.bptt in float64 ON THOSE float32
    BUFFERS (the forward's rounding does not enter); idv_lstm_bptt_coop also at the small batches where the dispatch never
    chooses it, idv_lstm_bptt also at H = 96 / 48 (both per-step kernels on a ragged tile) and with a work pointer that is not
    16-byte aligned (its documented fall-back from the cooperative form to the per-step kernels);
(c) the module's forward + backward per state of ops.LSTM_STACK2 / ops.LSTM_PERSISTENT in both arithmetic modes against float64
    autograd through the oracle -- the glue of autograd.LstmFn.backward around the non-fused entries included.

Errors are relative L2 per (time step, 16-sequence tile) block (lstm_ref.block_errors): a wrong row of the ragged last tile of one
step is not diluted by T * B.  Bounds: 2e-5 forward / 2e-4 gradients (1e-4 / 1e-3 in bf16x3 mode), those of tests/test_gpu_ops.py
and tests/test_gpu_backward.py; float32 arithmetic on these inputs stays a tenth inside them (tests/test_lstm_ref_host.py).
Scratch buffers have exactly the size their sizer reports, with sentinels behind.  DESIGN.md 3.5 has the measured figures."""
import importlib

import pytest
import torch

import lstm_ref
from test_gpu_backward import _clstm_oracle, _clstm_setup, _clstm_step, check

pytestmark = pytest.mark.gpu
TOL, GTOL = 2e-5, 2e-4
SENT, SENTV = 1024, -7.25                  # sentinel floats behind every scratch buffer, and their value
FRAMES = (1, 2, 5)
DEV = "cuda"


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


@pytest.fixture(scope="module")
def AG(amd):
    return importlib.import_module("i-dccrn-vae_amd.autograd")


@pytest.fixture(scope="module")
def cp():
    return importlib.import_module("i-dccrn-vae_amd.model.complex_progress")


# ----------------------------------------------------------------------------- the batch edges, from the device
def _edges(lib):
    m = lib.idv_coop_max_workgroups()
    ts, tc = min(16, m // 32), m // 16
    assert ts >= 1 and tc > ts, (m, ts, tc)
    return ts, tc


def _batch(sym, lib):
    ts, tc = _edges(lib)
    return {"1": 1, "16": 16, "17": 17, "S": 16 * ts, "S+1": 16 * ts + 1, "C-10": 16 * tc - 10, "C+1": 16 * tc + 1}[sym]


def _rung(H, B, lib):
    """0: both layers in one launch, 1: one cooperative launch per layer, 2: one-CU forward / per-step BPTT -- as the table
    predicts; the four predicates must say the same."""
    ts, tc = _edges(lib)
    tiles = (B + 15) // 16
    r = 2 if H != 128 else (0 if tiles <= ts else (1 if tiles <= tc else 2))
    got = (lib.idv_lstm_stack2_f32_supported(H, B), lib.idv_lstm_coop_f32_supported(H, B),
           lib.idv_lstm_bptt_stack2_supported(H, B), lib.idv_lstm_bptt_coop_supported(H, B))
    assert got == (int(r == 0), int(r <= 1), int(r == 0), int(r <= 1)), (H, B, r, got)
    return r


def test_batch_edges_of_this_device(ops):
    lib = ops.L.lib()
    ts, tc = _edges(lib)
    bs = [_batch(s, lib) for s in ("1", "16", "17", "S", "S+1", "C-10", "C+1")]
    assert bs == sorted(bs) and bs[3] >= 17 and bs[5] > bs[4]
    assert [_rung(128, b, lib) for b in bs] == [0, 0, 0, 0, 1, 1, 2]
    assert (16 * tc - 10 + 15) // 16 == tc and (16 * tc - 10) % 16 != 0          # the widest grid, ragged last tile
    print(f"LADDER edges: max workgroups {lib.idv_coop_max_workgroups()}, batches {bs}")


# ----------------------------------------------------------------------------- shared inputs and references (computed once)
_CASE, _PACK, _FWD, _REF = {}, {}, {}, {}


def _case(H, I, T, B):
    """(sd, x, R, float64 forward) of lstm_ref.make_case(H, I, T, B, LADDER_SEED); read-only."""
    k = (H, I, T, B)
    if k not in _CASE:
        sd, x, R = lstm_ref.make_case(H, I, T, B, lstm_ref.LADDER_SEED)
        _CASE[k] = (sd, x, R, lstm_ref.forward(x, sd))
    return _CASE[k]


def _packs(ops, H, I):
    """The parameters on the device and packed as ComplexLSTM._packed does (the same for every T, B: make_case draws them
    first), and the BPTT fragments of autograd.LstmFn.backward."""
    if (H, I) not in _PACK:
        sd = {k: v.to(DEV) for k, v in lstm_ref.make_case(H, I, 1, 1, lstm_ref.LADDER_SEED)[0].items()}
        get = lambda n: sd[n]
        p0, p1 = ops.pack_lstm(get, H, I, 0, DEV), ops.pack_lstm(get, H, H, 1, DEV)
        frag = {}
        for name in ("weight_hh_l1", "weight_ih_l1", "weight_hh_l0"):
            t = torch.empty(2 * 4 * H * H, dtype=torch.float32, device=DEV)
            ops.call("idv_pack_lstm_hh_bwd", ops.p(sd[f"lstm_re.{name}"]), ops.p(sd[f"lstm_im.{name}"]), ops.i(H), ops.p(t),
                     ops.stream_ptr())
            frag[name] = t
        _PACK[(H, I)] = (p0, p1, frag)
    return _PACK[(H, I)]


def _saved_of(work, perm, H, B, T):
    """The saved buffers [G0 16 TBH | G1 16 TBH | h0 | h1 | c0 | c1] of a training forward (csrc/lstm.hip) in lstm_ref's
    layout, float32 on the CPU: gates [2 layers, 4 runs, T, B, 4H] in torch's gate-row order, c, h [2, 4, T, B, H]."""
    TBH = T * B * H
    w = work[:48 * TBH].detach().cpu()
    perm = perm.cpu()
    G0 = w[:16 * TBH].view(2, T, B, 2, 4 * H)                                   # [z][t][b][s][colp]
    G1 = w[16 * TBH:32 * TBH].view(4, T, B, 4 * H)                              # [run][t][b][colp]
    g = torch.empty(2, 4, T, B, 4 * H)
    for z in range(2):
        for s in range(2):
            g[0, 2 * z + s][..., perm] = G0[z, :, :, s]
    g[1][..., perm] = G1
    hc = w[32 * TBH:48 * TBH].view(2, 2, 4, T, B, H)                            # [h | c][layer][run]
    return {"gates": g, "h": hc[0].clone(), "c": hc[1].clone()}


def _worst_blocks(got, want, B, keys, tol, what):
    """Every (layer, run) of every tensor in `keys`, per (t, tile) block -> the worst error; asserts bound and no stray values."""
    worst = 0.0
    for k in keys:
        for l in range(2):
            for r in range(4):
                e, stray = lstm_ref.block_errors(got[k][l, r], want[k][l, r], B)
                worst = max(worst, e)
                assert stray == 0, (what, k, l, r, stray)
                assert e <= tol, f"{what}: {k} layer {l} run {r}: worst (t, tile) block {e:.3e} > {tol:.1e}"
    return worst


# ----------------------------------------------------------------------------- (a) training forward, per rung
def _forward_once(ops, rung, H, I, T, B, Tp):
    lib = ops.L.lib()
    sd, x, _, _ = _case(H, I, T, B)
    p0, p1, _ = _packs(ops, H, I)
    xp = ops.Planar.from_tensor5(x.permute(1, 2, 0, 3).unsqueeze(2).to(DEV), Tp=Tp)
    out = ops.Planar.empty(H, 1, B, T, Tp, DEV)
    out.buf.fill_(float("nan"))
    n = int(lib.idv_clstm_train_work_floats(H, B, T, xp.Jp))
    work = torch.full((n + SENT,), float("nan"), dtype=torch.float32, device=DEV)
    work[n:] = SENTV
    flags, wih1_hh = {"stack2": (4, p1.wih_hh), "coop": (4, None), "one-cu": (4 | 8, p1.wih_hh), "generic": (4, None)}[rung]
    assert rung != "stack2" or wih1_hh is not None
    ops.call("idv_clstm_fwd2", xp.ptr(), ops.i(I), ops.p(p0.wih), ops.p(p0.bih), ops.p(p0.whh), ops.p(p1.wih), ops.p(p1.bih),
             ops.p(p1.whh), ops.p(wih1_hh), ops.i(H), ops.i(B), ops.i(T), ops.i(Tp), ops.i(xp.Jp), ops.p(work), out.ptr(),
             ops.i(flags), ops.p(None), ops.stream_ptr())
    torch.cuda.synchronize()
    assert lib.idv_coop_last_status(1) == 0, f"{rung} forward at B = {B}: a cooperative recurrence timed out"
    return xp, out, work, n


def _checked_forward(ops, AG, rung, H, I, T, B):
    """One training forward on the chosen rung with every assertion of (a); -> (saved buffers on the CPU, float32, as the
    kernels left them; the same in lstm_ref's layout).  Cached: (b) reads what (a) checked."""
    key = (rung, H, I, T, B)
    if key in _FWD:
        return _FWD[key]
    lib = ops.L.lib()
    r = _rung(H, B, lib)
    assert {"stack2": r == 0, "coop": r <= 1, "one-cu": H == 128, "generic": H != 128}[rung], (rung, H, B)
    sd, x, _, ref = _case(H, I, T, B)
    Tp = T + 3                                                                  # two columns behind the T valid ones
    xp, out, work, n = _forward_once(ops, rung, H, I, T, B, Tp)
    TBH = T * B * H
    assert bool((work[n:] == SENTV).all()), "sentinels behind the work buffer overwritten"
    # exact fp32 mode: the split image of h0 (the last 4 H Jp floats) is no one's scratch
    assert bool(work[n - 4 * H * xp.Jp:n].isnan().all()), "the split-image region behind the scratch was written"
    assert bool(torch.isfinite(work[:48 * TBH]).all())
    saved = _saved_of(work, AG._colp_perm(H, DEV), H, B, T)
    worst = _worst_blocks(saved, ref, B, ("gates", "c", "h"), TOL, f"{rung} forward H={H} B={B} T={T}")
    y = out.channel_slice(0, H).permute(1, 0, 2, 3)                              # [T, B, H, 2]
    e, stray = lstm_ref.block_errors(y, ref["out"], B)
    assert stray == 0 and e <= TOL, f"{rung} forward B={B} T={T}: output block {e:.3e}"
    pl = out.planes()                                                           # [2, H, 1, B, Tp]
    assert not bool(pl[..., 0].any()) and not bool(pl[..., T + 1:].any()), "guard / tail columns of the output not zero"
    # the same call again: the same bits
    _, out2, work2, _ = _forward_once(ops, rung, H, I, T, B, Tp)
    assert torch.equal(work2[:48 * TBH], work[:48 * TBH]) and torch.equal(out2.planes(), pl), "second call differs"
    print(f"LADDER (a) {rung:8s} H={H:3d} B={B:3d} T={T}: worst block saved {worst:.2e} output {e:.2e}")
    saved["x"] = x
    _FWD[key] = (work[:48 * TBH].cpu(), saved)
    return _FWD[key]


FWD_CASES = [("stack2", 128, s) for s in ("1", "16", "17", "S")] + [("coop", 128, s) for s in ("17", "S+1", "C-10")] + \
            [("one-cu", 128, s) for s in ("17", "C+1")] + [("generic", 96, "17"), ("generic", 48, "17")]


@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("rung,H,bsym", FWD_CASES)
def test_training_forward_of_every_rung(ops, AG, rung, H, bsym, T):
    _checked_forward(ops, AG, rung, H, 64, T, _batch(bsym, ops.L.lib()))


# ----------------------------------------------------------------------------- (b) the BPTT entries at the kernel boundary
def _scratch(nfloats, misalign=False):
    """Exactly nfloats floats of scratch (NaN) with SENT sentinel floats behind; 16-byte aligned unless `misalign` (then 4 bytes
    past an aligned address, a sentinel in front as well)."""
    off = 1 if misalign else 0
    buf = torch.full((off + nfloats + SENT,), SENTV, dtype=torch.float32, device=DEV)
    view = buf[off:off + nfloats]
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == (4 if misalign else 0)
    return buf, view, off + nfloats


def _bptt_refs(fkey, saved, R, sd):
    """lstm_ref.bptt in float64 on the float32 saved buffers: fused (layer 0 receives dA1 W_ih1) and per layer (layer 0
    receives that gradient rounded to float32, as the per-layer entries do)."""
    if fkey not in _REF:
        fused = lstm_ref.bptt(saved, R, sd)
        _REF[fkey] = (fused, lstm_ref.bptt(saved, R, sd, dh0=fused["dh0"].float()))
    return _REF[fkey]


def _run_entry(ops, entry, H, B, T, work_cpu, dh1, dh0, frag):
    """One BPTT entry on a fresh copy of the saved buffers, argument lists of autograd.LstmFn.backward -> the buffers after."""
    lib = ops.L.lib()
    TBH = T * B * H
    w = work_cpu.to(DEV)
    G0, G1 = w[:16 * TBH], w[16 * TBH:32 * TBH]
    c0, c1 = w[40 * TBH:44 * TBH], w[44 * TBH:48 * TBH]
    c, p, i, ll, st = ops.call, ops.p, ops.i, ops.ll, ops.stream_ptr
    guards = []
    if entry == "stack2":
        buf, bw, n = _scratch((int(lib.idv_lstm_bptt_stack2_work_bytes(H, B)) + 3) // 4)
        guards.append((buf, n))
        c("idv_lstm_bptt_stack2", p(G1), p(G0), ll(T * B * 8 * H), ll(4 * H), i(8 * H), p(c1), p(c0), p(dh1), p(frag["weight_hh_l1"]),
          p(frag["weight_ih_l1"]), p(frag["weight_hh_l0"]), i(H), i(B), i(T), p(bw), st())
    else:
        name = "idv_lstm_bptt_coop" if entry == "coop" else "idv_lstm_bptt"
        nfl = (int(lib.idv_lstm_bptt_coop_work_bytes(H, B)) + 3) // 4 if entry == "coop" else int(lib.idv_lstm_bptt_work_floats(H, B))
        for layer in (1, 0):
            buf, bw, n = _scratch(nfl, misalign=(entry == "misaligned"))
            guards.append((buf, n))
            if layer == 1:
                c(name, p(G1), ll(2 * T * B * 4 * H), ll(T * B * 4 * H), i(4 * H), p(c1), p(dh1), p(frag["weight_hh_l1"]), i(H), i(B),
                  i(T), p(bw), st())
            else:
                c(name, p(G0), ll(T * B * 8 * H), ll(4 * H), i(8 * H), p(c0), p(dh0), p(frag["weight_hh_l0"]), i(H), i(B), i(T),
                  p(bw), st())
    torch.cuda.synchronize()
    assert lib.idv_coop_last_status(1) == 0, f"BPTT entry {entry} at B = {B}: a cooperative recurrence timed out"
    for buf, n in guards:
        assert bool((buf[n:] == SENTV).all()) and (entry != "misaligned" or float(buf[0]) == SENTV), "scratch sentinels overwritten"
    return w


# entry, H, batch: idv_lstm_bptt_stack2 on its rung; idv_lstm_bptt_coop on its own rung and below; idv_lstm_bptt where it runs the
# per-step kernels: above both rungs (<2>), H = 96 (<2>) and 48 (<1>) on a ragged tile, and on a work pointer it cannot hand on
BPTT_CASES = [("stack2", 128, s) for s in ("1", "16", "17", "S")] + \
             [("coop", 128, s) for s in ("1", "16", "17", "S", "S+1", "C-10")] + \
             [("per-step", 128, "C+1"), ("per-step", 96, "17"), ("per-step", 48, "17"), ("misaligned", 128, "17")]


@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("entry,H,bsym", BPTT_CASES)
def test_bptt_entries_on_the_saved_buffers(ops, AG, entry, H, bsym, T):
    lib = ops.L.lib()
    I = 64
    B = _batch(bsym, lib)
    r = _rung(H, B, lib)
    assert {"stack2": r == 0, "coop": r <= 1, "per-step": r == 2, "misaligned": r <= 1}[entry], (entry, H, B, r)
    fwd_rung = "generic" if H != 128 else ("stack2", "coop", "one-cu")[r]
    fkey = (fwd_rung, H, I, T, B)
    work_cpu, saved = _checked_forward(ops, AG, fwd_rung, H, I, T, B)
    sd, _, R, _ = _case(H, I, T, B)
    fused, per_layer = _bptt_refs(fkey, saved, R, sd)
    ref = fused if entry == "stack2" else per_layer
    TBH = T * B * H
    Tp = T + 3
    do = ops.Planar.from_tensor5(R.permute(1, 2, 0, 3).unsqueeze(2).to(DEV), Tp=Tp)
    dh1 = torch.full((4 * TBH,), float("nan"), dtype=torch.float32, device=DEV)
    ops.call("idv_lstm_uncombine", do.ptr(), ops.i(H), ops.i(B), ops.i(T), ops.i(Tp), ops.i(do.Jp), ops.p(dh1), ops.stream_ptr())
    assert torch.equal(dh1.view(4, T, B, H).cpu(), lstm_ref.uncombine(R)), "idv_lstm_uncombine"
    dh0 = per_layer["dh0"].float().contiguous().to(DEV)                          # the reference's dA1 W_ih1, rounded
    _, _, frag = _packs(ops, H, I)
    w = _run_entry(ops, entry, H, B, T, work_cpu, dh1, dh0, frag)
    assert torch.equal(w[32 * TBH:].cpu(), work_cpu[32 * TBH:]), "h / c buffers changed"
    got = _saved_of(w, AG._colp_perm(H, DEV), H, B, T)
    worst = _worst_blocks({"dA": got["gates"]}, ref, B, ("dA",), GTOL, f"BPTT {entry} H={H} B={B} T={T}")
    w2 = _run_entry(ops, entry, H, B, T, work_cpu, dh1, dh0, frag)
    assert torch.equal(w2, w), "a repeat on a fresh copy differs"
    print(f"LADDER (b) {entry:10s} H={H:3d} B={B:3d} T={T}: worst block dA {worst:.2e}")


# ----------------------------------------------------------------------------- (c) through the module, per rung and precision
class _Switches:
    """ops.LSTM_STACK2 / LSTM_PERSISTENT / the arithmetic mode, restored afterwards."""

    def __init__(self, ops, stack2, persistent, precision):
        self.ops, self.want = ops, (stack2, persistent, precision)

    def __enter__(self):
        o = self.ops
        self.keep = o.LSTM_STACK2, o.LSTM_PERSISTENT, o.PRECISION
        o.LSTM_STACK2, o.LSTM_PERSISTENT = self.want[:2]
        o.set_precision(self.want[2])
        return self

    def __exit__(self, *exc):
        o = self.ops
        o.LSTM_STACK2, o.LSTM_PERSISTENT = self.keep[:2]
        o.set_precision(self.keep[2])
        return False


_ORACLE = {}
MODULE_CASES = [("fp32", 64, "17"), ("fp32", 64, "S+1"), ("fp32", 64, "C+1"), ("bf16x3", 64, "17"), ("bf16x3", 1280, "S+1")]
MODULE_TOL = {"fp32": (2e-5, 2e-4), "bf16x3": (1e-4, 1e-3)}


@pytest.mark.parametrize("stack2,persistent", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("precision,I,bsym", MODULE_CASES)
def test_module_step_per_switch_state(ops, cp, precision, I, bsym, stack2, persistent):
    lib = ops.L.lib()
    H, T = 128, 5
    B = _batch(bsym, lib)
    _rung(H, B, lib)
    ftol, gtol = MODULE_TOL[precision]
    m, x, R = _clstm_setup(cp, H, I, T, B)
    if (I, B) not in _ORACLE:
        _ORACLE[(I, B)] = _clstm_oracle(m, x, R)
    want, dx, grads = _ORACLE[(I, B)]
    with _Switches(ops, stack2, persistent, precision):
        y, xp, gbuf = _clstm_step(ops, m, x, R)
        torch.cuda.synchronize()
        assert lib.idv_coop_last_status(1) == 0
        pg = {k: p_.grad.clone() for k, p_ in m.named_parameters()}
        y2, _, gbuf2 = _clstm_step(ops, m, x, R)
        torch.cuda.synchronize()
        assert lib.idv_coop_last_status(1) == 0
    check("forward", y, want, ftol)
    gp = ops.rewrap(gbuf, xp)
    gx = gp.tensor5()[:, :, 0].permute(2, 0, 1, 3)                               # [T, B, I, 2]
    check("dx", gx, dx, gtol)
    assert sorted(pg) == sorted(lstm_ref.NAMES)
    for k in lstm_ref.NAMES:
        check(k, pg[k], grads[k], gtol)
    e, stray = lstm_ref.block_errors(gx, dx, B)
    assert stray == 0 and e <= gtol, f"dx: worst (t, tile) block {e:.3e} > {gtol:.1e}"
    fe, _ = lstm_ref.block_errors(y, want, B)
    assert not bool(gp.planes()[..., 0].any()), "guard column of the input gradient not zero"
    assert torch.equal(y2, y), "the same step again: another forward"
    assert torch.equal(ops.rewrap(gbuf2, xp).planes(), gp.planes()), "the same step again: another input gradient"
    for k, p_ in m.named_parameters():
        assert torch.equal(p_.grad, pg[k]), f"the same step again: another gradient of {k}"
    print(f"LADDER (c) {precision:6s} I={I:4d} B={B:3d} stack2={int(stack2)} persistent={int(persistent)}: worst block forward {fe:.2e} "
          f"dx {e:.2e}")
