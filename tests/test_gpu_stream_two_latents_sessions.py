"""Streaming two-latent sessions (streaming.StreamingVAETwoLatentsSessions) and the per-slot seeds of both VAE sessions classes on
the MI355X: the draws entry idv_stream_eps_pair_rows against its lock-step twin, and slots that start, receive samples and end
on their own, each with its own seed, against the lock-step StreamingVAETwoLatents / StreamingVAE, bit for bit, for the same
signal in the same slot."""
import functools
import importlib
import random

import pytest
import torch

from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4          # the streaming-to-offline bar of tests/test_gpu_streaming.py
OUTTYPES = ["clean_direct", "real_imag_mask", "complex_mask", "phase_mask"]


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.streaming"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"),
            importlib.import_module("i-dccrn-vae_amd.inference"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def load_synth(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(O.synth_state_dict(shapes, seed), strict=True)
    return module.cuda()


@functools.lru_cache(maxsize=None)
def _trio(base=4, zdim=16, ns=2, phase=2, seed=40):
    """(noisy encoder, speech decoder, noise decoder): phase 2 the fine-tuned decoders (mask), phase 1 the pre-trained zero-skip
    class (real_imag).  Built once per shape and shared (nobody writes to them)."""
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    enc = load_synth(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2), seed + 1)
    if phase == 1:
        mk = lambda sd: load_synth(pm.pvae_dccrn_decoder_skip_prepare(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "real_imag", SKIP), sd)
    else:
        mk = lambda sd: load_synth(pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP,
                                                                        False), sd)
    return enc, mk(seed + 2), mk(seed + 3)


def _signals(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(L, generator=g) * 0.1).cuda() for L in lengths]


def _lockstep(ref, slot, sig):
    """The signal whole in slot ``slot`` of the lock-step streamer ``ref`` (the other slots carry zeros), then flushed -> [1, m]."""
    x = torch.zeros(ref.B, len(sig), device="cuda")
    x[slot] = sig
    y = torch.cat([ref.push(x), ref.flush()], dim=1)
    return y[slot:slot + 1]


def _serve(st, queues, starts, width, count_of, on_call=None):
    """tests/test_gpu_stream_vae_sessions.py's ``_serve``: feeds ``queues[b]`` (the signals of slot b, one after the other, the
    first from call ``starts[b]``) through ``st`` with ``count_of(b, call, remaining)`` samples per call; a signal ends in the
    call that brings its last samples.  Every call's x[b, counts[b]:] is NaN; every output is finite and zero behind m[b].
    Returns {(slot, index of the signal in its queue): output [1, samples]}."""
    B = st.B
    queues = [list(q) for q in queues]
    cur, pos, idx = [None] * B, [0] * B, [-1] * B
    outs = {}
    ci = 0
    while any(queues) or any(c is not None for c in cur):
        x = torch.full((B, width), float("nan"), device="cuda")
        counts, end = [0] * B, []
        for b in range(B):
            if cur[b] is None and queues[b] and ci >= starts[b]:
                cur[b], pos[b], idx[b] = queues[b].pop(0), 0, idx[b] + 1
            if cur[b] is None:
                continue
            n = min(count_of(b, ci, len(cur[b]) - pos[b]), len(cur[b]) - pos[b], width)
            x[b, :n] = cur[b][pos[b]:pos[b] + n]
            counts[b], pos[b] = n, pos[b] + n
            if pos[b] == len(cur[b]):
                end.append(b)
        assert st.positions == [pos[b] - counts[b] if cur[b] is not None else 0 for b in range(B)]
        y, m = st.push(x, counts, end)
        assert y.shape == (B, max(m)) and bool(torch.isfinite(y).all())
        for b in range(B):
            assert not bool(y[b, m[b]:].any())
            if cur[b] is not None:
                outs.setdefault((b, idx[b]), []).append(y[b:b + 1, :m[b]])
            else:
                assert m[b] == 0
        for b in end:
            cur[b] = None
        if on_call is not None:
            on_call(ci, cur, pos)
        ci += 1
    return {k: torch.cat(v, dim=1) for k, v in outs.items()}


def _rows(S, B, **fields):
    t = torch.zeros(B, S.NF, dtype=torch.int64)
    for name, v in fields.items():
        t[:, S.ROW_FIELDS.index(name)] = torch.tensor(v, dtype=torch.int64)
    return t


# ------------------------------------------------------------------------------------------------------------ 1. the entry
def test_eps_pair_rows_entry():
    _, S, _, L, _ = _mods()
    B, ns, zdim, KL = 5, 3, 16, 5
    ks, t0 = [3, 0, 5, 1, 5], [0, 7, 2 ** 32 + 1, 7, 0]
    seeds = [0, 5, 2 ** 40 + 3, 0x1234567890ABCDEF >> 1, 9]
    rows = _rows(S, B, t0=t0, k=ks).cuda()
    sd = torch.tensor(seeds, dtype=torch.int64).cuda()
    got = torch.full((4, B, ns, KL, zdim), float("nan"), device="cuda")

    def entry(seeds_t, rows_t, out, pair=True):
        L.call("idv_stream_eps_pair_rows", L.p(seeds_t), L.p(rows_t), L.i(B), L.i(ns), L.i(zdim), L.i(KL), L.p(out[0]), L.p(out[1]),
               L.p(out[2]) if pair else L.p(None), L.p(out[3]) if pair else L.p(None), L.stream_ptr())
    entry(sd, rows, got)
    for b in range(B):
        assert not bool(got[:, b, :, ks[b]:].any()), b             # zeros, and no NaN, from frame k_b on in all four outputs
        if ks[b] == 0:
            continue
        want = torch.empty(4, B, ns, ks[b], zdim, device="cuda")
        L.call("idv_stream_eps_pair", L.ll(seeds[b]), L.ll(t0[b]), L.i(ks[b]), L.i(B), L.i(ns), L.i(zdim), L.p(want[0]), L.p(want[1]),
               L.p(want[2]), L.p(want[3]), L.stream_ptr())
        assert torch.equal(got[:, b, :, :ks[b]], want[:, b]), b
        assert all(bool(want[j, b].any()) for j in range(4))
    # slots 1 and 3 share t0, slots 0 and 4 too: the seeds (and b) tell them apart
    assert not torch.equal(got[0, 0, :, :3], got[0, 4, :, :3])
    # the single-pair form with equal seeds is idv_stream_eps_rows
    same = torch.full((B,), seeds[3], dtype=torch.int64).cuda()
    one = torch.full((4, B, ns, KL, zdim), float("nan"), device="cuda")
    entry(same, rows, one, pair=False)
    assert bool(torch.isnan(one[2:]).all())                        # the noise pair is not written
    ref = torch.full((2, B, ns, KL, zdim), float("nan"), device="cuda")
    L.call("idv_stream_eps_rows", L.ll(seeds[3]), L.p(rows), L.i(B), L.i(ns), L.i(zdim), L.i(KL), L.p(ref[0]), L.p(ref[1]), L.stream_ptr())
    assert torch.equal(one[:2], ref) and bool(ref.any())
    # and the speech pair of the full form with the same seeds, too
    both = torch.full((4, B, ns, KL, zdim), float("nan"), device="cuda")
    entry(same, rows, both)
    assert torch.equal(both[:2], ref)
    for args in ((sd, rows, (got[0], got[1], got[2], None)), (sd, rows, (got[0], got[1], None, got[3])), (None, rows, got),
                 (sd, None, got)):
        with pytest.raises(L.IdvError):
            L.call("idv_stream_eps_pair_rows", L.p(args[0]), L.p(args[1]), L.i(B), L.i(ns), L.i(zdim), L.i(KL), L.p(args[2][0]),
                   L.p(args[2][1]), L.p(args[2][2]), L.p(args[2][3]), L.stream_ptr())
    for bad in (dict(B=0), dict(ns=0), dict(zdim=0), dict(KL=0)):
        d = {**dict(B=B, ns=ns, zdim=zdim, KL=KL), **bad}
        with pytest.raises(L.IdvError):
            L.call("idv_stream_eps_pair_rows", L.p(sd), L.p(rows), L.i(d["B"]), L.i(d["ns"]), L.i(d["zdim"]), L.i(d["KL"]), L.p(got[0]),
                   L.p(got[1]), L.p(got[2]), L.p(got[3]), L.stream_ptr())


# ------------------------------------------------------------------------------------------------------ 2. staggered serving
def _staggered(st, seed=4):
    """The schedule of tests/test_gpu_stream_sessions.py: queues [[a], [b1, b2], [c]], starts at calls 0, 1, 3."""
    a, b1, b2, c = _signals([1234, 777, 701, 2345], 31)
    rng = random.Random(seed)
    got = _serve(st, [[a], [b1, b2], [c]], [0, 1, 3], 300, lambda b, ci, left: rng.choice([0, 0, 1, 37, 100, 250, 300]))
    assert st.positions == [0, 0, 0]
    return got, {(0, 0): a, (1, 0): b1, (1, 1): b2, (2, 0): c}


def test_staggered_sessions_equal_the_lockstep_streamer():
    S = _mods()[1]
    enc, ds, dn = _trio()
    st = S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=3, outtype="phase_mask", phase=2, seed=3, frames_per_launch=8)
    assert st.H == 96 and st.cap == 8 and st.seeds == [3, 3, 3]
    got, sigs = _staggered(st)
    ref = S.StreamingVAETwoLatents(enc, ds, dn, batch=3, outtype="phase_mask", phase=2, seed=3, frames_per_launch=8)
    for (slot, j), sig in sigs.items():
        want = _lockstep(ref, slot, sig)
        assert got[(slot, j)].shape == want.shape == (1, HOP * (len(sig) // HOP))
        assert torch.equal(got[(slot, j)], want), (slot, j)
        assert float(want.abs().max()) > 0
    assert all(torch.equal(u, v) for u, v in zip(st.eps(5, 3), ref.eps(5, 3)))


# --------------------------------------------------------------------------------------------------------- 3. all estimators
@pytest.mark.parametrize("outtype", OUTTYPES)
@pytest.mark.parametrize("phase", [1, 2])
def test_every_estimator_with_idle_slots(outtype, phase):
    """Two slots; slot 1 idles for calls 2 .. 4 in the middle of its signal and slot 0 for calls 6 and 7, so launch groups with
    k_b = 0 < k_launch occur for either slot: the estimator runs on the idle slot's columns too, and nothing of them may reach
    a returned sample (complex_mask divides by S + N, which is 0 where an idle slot's spectrum is 0)."""
    _, S, _, _, inf = _mods()
    enc, ds, dn = _trio(phase=phase)
    sigs = _signals([1100, 900], 36)

    def count_of(b, ci, left):
        if (b == 1 and 2 <= ci <= 4) or (b == 0 and ci in (6, 7)):
            return 0
        return [250, 100, 300, 37][(b + ci) % 4]
    st = S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=2, outtype=outtype, phase=phase, seed=7, frames_per_launch=8)
    got = _serve(st, [[sigs[0]], [sigs[1]]], [0, 0], 300, count_of)
    ref = S.StreamingVAETwoLatents(enc, ds, dn, batch=2, outtype=outtype, phase=phase, seed=7, frames_per_launch=8)
    for b, sig in enumerate(sigs):
        want = _lockstep(ref, b, sig)
        assert want.shape == (1, HOP * (len(sig) // HOP)) and torch.equal(got[(b, 0)], want), b
    if (outtype, phase) == ("complex_mask", 2):
        for b, sig in enumerate(sigs):
            own = tuple(e[b:b + 1] for e in st.eps(0, 1 + len(sig) // HOP))
            off = inf.enhance_vae_two_latents(enc, ds, dn, sig[None], outtype, phase, eps=own)
            err = relerr(got[(b, 0)], off)
            print(f"slot {b} ({len(sig)} samples) {outtype} phase {phase} vs enhance_vae_two_latents: {err:.3e}")
            assert off.shape == got[(b, 0)].shape and err < TOL, b


# -------------------------------------------------------------------------------------------------------------- 4. nine slots
def test_nine_slots_cross_the_lstm_stream_tile():
    """9 slots: the wide LSTM runs 8 streams per workgroup.  Slots 7 and 8 complete different frame counts in the same call,
    slot 3 idles for calls 3 .. 6 in the middle of its signal."""
    S = _mods()[1]
    enc, ds, dn = _trio()
    sigs = _signals([900, 750, 1000, 1100, 800, 700, 950, 1200, 700], 32)
    steps = [100, 250, 37, 300, 1, 163]

    def count_of(b, ci, left):
        if b == 3 and 3 <= ci <= 6:
            return 0
        return {7: 300, 8: 100}.get(b, steps[(b + ci) % len(steps)])
    st = S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=9, outtype="real_imag_mask", seed=1, frames_per_launch=8)
    got = _serve(st, [[s] for s in sigs], [0] * 9, 300, count_of)
    ref = S.StreamingVAETwoLatents(enc, ds, dn, batch=9, outtype="real_imag_mask", seed=1, frames_per_launch=8)
    for b, sig in enumerate(sigs):
        assert torch.equal(got[(b, 0)], _lockstep(ref, b, sig)), b


# ------------------------------------------------------------------------------------------------------------------ 5. seeds
@pytest.mark.parametrize("cls", ["StreamingVAESessions", "StreamingVAETwoLatentsSessions"])
def test_per_slot_seeds(cls):
    S = _mods()[1]
    enc, ds, dn = _trio()
    if cls == "StreamingVAESessions":
        st = S.StreamingVAESessions(enc, ds, slots=3, seed=9, frames_per_launch=8)
        ref = S.StreamingVAE(enc, ds, batch=3, seed=9, frames_per_launch=8)
    else:
        st = S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=3, outtype="phase_mask", seed=9, frames_per_launch=8)
        ref = S.StreamingVAETwoLatents(enc, ds, dn, batch=3, outtype="phase_mask", seed=9, frames_per_launch=8)
    seeds = [0, 5, 2 ** 40 + 3]
    for b, v in enumerate(seeds):
        st.set_seed([b], v)
    assert st.seeds == seeds and st.seed == 9
    a, b1, b2, c = _signals([1500, 700, 800, 900], 37)
    NEW = 77
    done = []

    def on_call(ci, cur, pos):
        if cur[1] is None and not done:               # slot 1 has just ended b1; slot 0 is in mid-signal
            assert st.positions[0] > 0 and st.positions[1] == 0 and st.seeds == seeds     # the seed outlives the signal
            with pytest.raises(ValueError, match="slot 0"):
                st.set_seed([0, 1], NEW)
            assert st.seeds == seeds
            st.set_seed([1], NEW)
            done.append(ci)
    got = _serve(st, [[a], [b1, b2], [c]], [0, 0, 0], 300, lambda b, ci, left: [100, 250, 37, 300][(b + ci) % 4], on_call)
    assert done and st.seeds == [0, NEW, 2 ** 40 + 3]
    for (slot, j), sig, seed in (((0, 0), a, 0), ((1, 0), b1, 5), ((1, 1), b2, NEW), ((2, 0), c, 2 ** 40 + 3)):
        ref.seed = seed
        assert torch.equal(got[(slot, j)], _lockstep(ref, slot, sig)), (slot, j)
    ref.seed = 9                                       # the default seed would have drawn otherwise
    assert not torch.equal(got[(0, 0)], _lockstep(ref, 0, a))
    # eps(t0, k): row b with slot b's seed
    for t0, k in ((0, 4), (2 ** 32 + 1, 3)):
        own = st.eps(t0, k)
        assert len(own) == (2 if cls == "StreamingVAESessions" else 4)
        for b, seed in enumerate(st.seeds):
            ref.seed = seed
            want = ref.eps(t0, k)
            assert all(torch.equal(u[b], v[b]) for u, v in zip(own, want)) and bool(want[0][b].any()), (t0, b)
    # seed = clears the overrides
    st.seed = 4
    assert st.seeds == [4, 4, 4]
    ref.seed = 4
    assert all(torch.equal(u, v) for u, v in zip(st.eps(1, 2), ref.eps(1, 2)))


# ---------------------------------------------------------------------------------------------------------------- 6. engines
@pytest.mark.parametrize("outtype,n_packs", [("complex_mask", 18), ("clean_direct", 12)])
def test_mfma_engine_gives_the_bits_of_valu(outtype, n_packs):
    S = _mods()[1]
    enc, ds, dn = _trio()
    mk = lambda conv: S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=3, outtype=outtype, seed=3, frames_per_launch=8, conv=conv)
    stm, stv = mk("mfma"), mk("valu")
    assert len(stm.conv_engines) == len(stv.conv_engines) == n_packs
    assert "mfma" in stm.conv_engines and stv.conv_engines == ["valu"] * n_packs
    gm, sigs = _staggered(stm)
    gv, _ = _staggered(stv)
    for key in sigs:
        assert torch.equal(gm[key], gv[key]), key


# ------------------------------------------------------------------------------------------------------------ 7. other paths
def test_clean_direct_phase2_is_streaming_vae_sessions():
    S = _mods()[1]
    enc, ds, dn = _trio()
    for noise in (None, dn):
        two = S.StreamingVAETwoLatentsSessions(enc, ds, noise, slots=3, outtype="clean_direct", phase=2, seed=3, frames_per_launch=8)
        one = S.StreamingVAESessions(enc, ds, slots=3, seed=3, frames_per_launch=8)
        assert two.noise is None and len(two.conv_engines) == 12
        for st in (two, one):
            st.set_seed([1], 2 ** 40 + 3)
        g2, sigs = _staggered(two)
        g1, _ = _staggered(one)
        for key in sigs:
            assert g2[key].shape == (1, HOP * (len(sigs[key]) // HOP)) and torch.equal(g2[key], g1[key]), key


def test_drop_reuse_and_reset():
    S = _mods()[1]
    enc, ds, dn = _trio()
    a, b_old, b_new, c = _signals([1000, 900, 700, 1100], 34)
    mk = lambda: S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=3, outtype="complex_mask", seed=5, frames_per_launch=8)
    st = mk()

    def on_call(ci, cur, pos):
        if ci == 3:                                   # slot 1 is 400 samples into b_old: abandon it
            assert st.positions[1] == 400
            st.drop([1])
            assert st.positions[1] == 0
            cur[1] = None
    got = _serve(st, [[a], [b_old, b_new], [c]], [0, 0, 0], 100, lambda b, ci, left: 100, on_call)
    ref = S.StreamingVAETwoLatents(enc, ds, dn, batch=3, outtype="complex_mask", seed=5, frames_per_launch=8)
    assert got[(1, 0)].shape == (1, 100)              # what b_old returned before it was dropped
    for key, sig in (((0, 0), a), ((1, 1), b_new), ((2, 0), c)):
        assert torch.equal(got[key], _lockstep(ref, key[0], sig)), key
    # reset() in the middle of three signals: every slot starts anew
    st.push(torch.stack([a[:600], c[:600], b_new[:600]]))
    assert st.positions == [600, 600, 600]
    st.reset()
    assert st.positions == [0, 0, 0]
    again = _serve(st, [[], [b_new], []], [0, 0, 0], 250, lambda b, ci, left: 250)
    assert torch.equal(again[(1, 0)], got[(1, 1)])


def test_phase1_makes_no_repeat_call_and_equals_lockstep(monkeypatch):
    S = _mods()[1]
    names = []
    real = S.call
    monkeypatch.setattr(S, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    sigs = _signals([900, 1000], 38)
    for phase in (1, 2):
        enc, ds, dn = _trio(phase=phase)
        del names[:]
        st = S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=2, outtype="phase_mask", phase=phase, seed=2, frames_per_launch=8)
        got = _serve(st, [[sigs[0]], [sigs[1]]], [0, 1], 300, lambda b, ci, left: [300, 100, 250][(b + ci) % 3])
        assert "idv_stream_eps_pair_rows" in names and "idv_stream_estimate" in names and "idv_stream_eps_rows" not in names
        if phase == 1:
            assert st.skip_n == {} and all(cp.C1 == 0 for ch in st.chains for cp in ch.dec)
            assert "idv_stream_repeat_rows" not in names and "idv_stream_repeat" not in names
            ref = S.StreamingVAETwoLatents(enc, ds, dn, batch=2, outtype="phase_mask", phase=1, seed=2, frames_per_launch=8)
            for b, sig in enumerate(sigs):
                assert torch.equal(got[(b, 0)], _lockstep(ref, b, sig)), b
        else:
            assert "idv_stream_repeat_rows" in names


# ------------------------------------------------------------------------------------------------------ 8. full width once
def test_full_width():
    """base 32, zdim 128, num_samples 3: H = 768, the widest LSTM the entry takes; two short signals staggered by one call."""
    S = _mods()[1]
    enc, ds, dn = _trio(32, 128, 3, 2, 80)
    sigs = _signals([800, 700], 35)
    st = S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=2, outtype="phase_mask", phase=2, seed=5)
    assert st.H == 768 and st.ns == 3
    steps = [300, 100, 250]
    got = _serve(st, [[sigs[0]], [sigs[1]]], [0, 1], 300, lambda b, ci, left: steps[(b + ci) % 3])
    assert st.positions == [0, 0]
    ref = S.StreamingVAETwoLatents(enc, ds, dn, batch=2, outtype="phase_mask", phase=2, seed=5)
    for b, sig in enumerate(sigs):
        want = _lockstep(ref, b, sig)
        assert want.shape == (1, HOP * (len(sig) // HOP))
        assert torch.equal(got[(b, 0)], want), b
