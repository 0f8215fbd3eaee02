"""Save, load and move a slot's stream (streaming._Slots.save / load, csrc/stream_state.hip, idv_stream_eps_pair_rows_as) on the
MI355X: the gather / scatter entries against torch indexing, the draws entry against its sibling, the slot-index independence the
contract rests on, and streams that move between slots, objects, engines and the host in mid-signal and continue bit for bit."""
import functools
import importlib

import pytest
import torch

from oracle import idccrn_oracle as O

pytestmark = pytest.mark.gpu

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
TOL = 1e-4                      # the waveform tolerance of tests/test_gpu_streaming.py
NAN = float("nan")


def _mods():
    return (importlib.import_module("i-dccrn-vae_amd.model.pvae_module"), importlib.import_module("i-dccrn-vae_amd.streaming"),
            importlib.import_module("i-dccrn-vae_amd.ops"), importlib.import_module("i-dccrn-vae_amd._lib"))


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _model(base=4, seed=21):
    pm = _mods()[0]
    m = pm.DCCRN_(NFFT, HOP, O.net_params(True, base), True, "cuda", WIN, SKIP, "mask", False, None, None)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k not in ("data_mean", "data_std")}, seed)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def load_synth(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(O.synth_state_dict(shapes, seed), strict=True)
    return module.cuda()


@functools.lru_cache(maxsize=None)
def _trio(base=4, zdim=16, ns=2, seed=40):
    """(noisy encoder, speech decoder, noise decoder) of tests/test_gpu_stream_two_latents_sessions.py; the first two are the pair
    of tests/test_gpu_stream_vae_sessions.py.  Built once and shared (nobody writes to them)."""
    pm = _mods()[0]
    np_ = O.net_params(True, base)
    enc = load_synth(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", zdim, NFFT, HOP, WIN, ns, 2), seed + 1)
    mk = lambda sd: load_synth(pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", ns, zdim, NFFT, HOP, WIN, "mask", True, SKIP, False), sd)
    return enc, mk(seed + 2), mk(seed + 3)


@functools.lru_cache(maxsize=None)
def _signals():
    """a (1234 samples, the stream that moves), b (2345) and two that keep the other slots busy."""
    g = torch.Generator().manual_seed(31)
    return tuple((torch.randn(n, generator=g) * 0.1).cuda() for n in (1234, 2345, 3000, 3000))


def _lockstep(ref, slot, sig):
    """The signal whole in slot ``slot`` of the lock-step streamer ``ref`` (the other slots carry zeros), then flushed."""
    x = torch.zeros(ref.B, len(sig), device="cuda")
    x[slot] = sig
    return torch.cat([ref.push(x), ref.flush()], dim=1)[slot]


@functools.lru_cache(maxsize=None)
def _ref_dccrn(B, slot, which=0):
    """Computed once and shared: signal ``which`` whole in slot ``slot`` of StreamingDCCRN(batch=B)."""
    S = _mods()[1]
    return _lockstep(S.StreamingDCCRN(_model(), batch=B, frames_per_launch=8), slot, _signals()[which])


def _push(st, feeds, end=()):
    """One call: ``feeds[b]`` are slot b's new samples, everything else of x is NaN -> ({slot: its output}, m)."""
    width = max([len(v) for v in feeds.values()] + [1])
    x = torch.full((st.B, width), NAN, device="cuda")
    counts = [0] * st.B
    for b, v in feeds.items():
        x[b, :len(v)] = v
        counts[b] = len(v)
    y, m = st.push(x, counts, list(end))
    assert y.shape[1] == max(m) and bool(torch.isfinite(y).all())
    return {b: y[b, :m[b]].clone() for b in feeds}, m


class _Feeder:
    """Feeds one signal into one slot piece by piece while the other slots of the object receive the busy signals at their own
    pace (slot b: 37 + 63 b samples per call, so the slots stand at staggered counts)."""

    def __init__(self, st, slot, sig, pos=0, busy=None):
        self.st, self.slot, self.sig, self.pos, self.out, self.m = st, slot, sig, pos, [], []
        self.busy = {b: [_signals()[2 + j % 2], 0] for j, b in enumerate(range(st.B) if busy is None else busy) if b != slot}

    def step(self, n, end=False):
        feeds = {self.slot: self.sig[self.pos:self.pos + n]}
        self.pos += n
        for b, (sig, at) in self.busy.items():
            c = 37 + 63 * b
            feeds[b] = sig[at:at + c]
            self.busy[b][1] = at + c
        got, m = _push(self.st, feeds, [self.slot] if end else [])
        self.out.append(got[self.slot])
        self.m.append(m[self.slot])

    def run(self, sizes, to=None):
        """Pieces of ``sizes`` (cycled) up to position ``to`` (default: the end of the signal, which then ends)."""
        stop = len(self.sig) if to is None else to
        j = 0
        while self.pos < stop:
            n = min(sizes[j % len(sizes)], stop - self.pos)
            self.step(n, end=to is None and self.pos + n == stop)
            j += 1
        return self

    def cat(self):
        return torch.cat(self.out)


ODD = [163, 37, 301, 1, 99]
# the pieces signal a arrives in before each cut: no frame yet; ring not wrapped; ring wrapped; an exact hop multiple; late
CUTS = {1: [1], 300: [100, 200], 777: [100, 250, 37, 300, 90], 800: [400, 400], 1201: [100, 250, 37, 300, 1, 163, 350]}


def _host_plan(n):
    S = _mods()[1]
    pl = S.StreamPlan(NFFT, HOP, WIN, 8)
    for c in CUTS[n]:
        pl.push(c)
    assert pl.n == n
    return (pl.n, pl.k, pl.emitted, pl.carry, pl.parity)


# ------------------------------------------------------------------------------------------------------------ 1. entries
@pytest.mark.parametrize("B", [1, 9])
def test_gather_and_scatter_entries_against_torch_indexing(B):
    """Three views at once: inner = 1 with a large outer (a history), inner = 7, and outer = 1 (a ring)."""
    _, S, _, L = _mods()
    g = torch.Generator().manual_seed(B)
    shapes = [(5003, 1), (3, 7), (1, 512)]
    per = sum(o * n for o, n in shapes)
    src = [torch.randn(o, B, n, generator=g).cuda() for o, n in shapes]

    def table(bufs):
        rows, off = [], 0
        for t, (o, n) in zip(bufs, shapes):
            rows += [t.data_ptr(), o, n, off]
            off += o * n
        return torch.tensor(rows, dtype=torch.int64)

    def run(name, bufs, slots, rec):
        host, sl = table(bufs), torch.tensor(slots, dtype=torch.int64)
        assert L.lib().idv_stream_state_check(L._P(host.data_ptr()), 3, B, L._P(sl.data_ptr()), len(slots), per) == 0
        L.call(name, L.p(host.cuda()), L.i(3), L.i(B), L.p(sl.cuda()), L.i(len(slots)), L.p(rec), L.ll(per), L.stream_ptr())
        torch.cuda.synchronize()

    record = lambda bufs, b: torch.cat([t[:, b, :].reshape(-1) for t in bufs])
    for slots in ([B // 2], [(2 * b + 1) % B for b in range(B)]):
        # gather: the unnamed slots hold NaN, which must not be read
        masked = [t.clone() for t in src]
        for t in masked:
            for b in set(range(B)) - set(slots):
                t[:, b, :] = NAN
        before = [t.clone() for t in masked]
        rec = torch.full((len(slots), per), NAN, device="cuda")
        run("idv_stream_state_gather", masked, slots, rec)
        for j, b in enumerate(slots):
            assert torch.equal(rec[j], record(src, b)), (slots, b)
        assert all(torch.equal(bits(u), bits(v)) for u, v in zip(masked, before))           # a gather writes no buffer
        # scatter into other slots of NaN-filled buffers: the named slots take the records, the others keep their bits
        to = [(b + 1) % B for b in slots] if len(slots) == 1 else [(5 * b + 2) % B for b in range(B)]
        dst = [torch.full_like(t, NAN) for t in src]
        keep = rec.clone()
        run("idv_stream_state_scatter", dst, to, rec)
        assert torch.equal(rec, keep)
        for j, b in enumerate(to):
            assert torch.equal(record(dst, b), record(src, slots[j])), (to, b)
        for t in dst:
            for b in set(range(B)) - set(to):
                assert bool((bits(t[:, b, :]) == bits(torch.full_like(t[:, b, :], NAN))).all())


# --------------------------------------------------------------------------------------------------------- 2. eps entry
@pytest.mark.parametrize("pair", [False, True])
def test_eps_entry_with_draw_slots(pair):
    _, S, _, L = _mods()
    B, ns, zdim, KL = 5, 2, 16, 4
    F = S.ROW_FIELDS.index
    rows = torch.zeros(B, S.NF, dtype=torch.int64)
    rows[:, F("t0")] = torch.tensor([0, 7, 2 ** 32 + 1, 3, 100])
    rows[:, F("k")] = torch.tensor([4, 1, 3, 0, 2])
    seeds = torch.tensor([0, 5, 2 ** 40 + 3, 9, 9], dtype=torch.int64)
    n_out = 4 if pair else 2

    def old(seeds_, rows_):
        out = torch.full((4, B, ns, KL, zdim), NAN, device="cuda")
        L.call("idv_stream_eps_pair_rows", L.p(seeds_.cuda()), L.p(rows_.cuda()), L.i(B), L.i(ns), L.i(zdim), L.i(KL), L.p(out[0]),
               L.p(out[1]), L.p(out[2]) if pair else L.p(None), L.p(out[3]) if pair else L.p(None), L.stream_ptr())
        torch.cuda.synchronize()
        return out

    def new(draw):
        out = torch.full((4, B, ns, KL, zdim), NAN, device="cuda")
        L.call("idv_stream_eps_pair_rows_as", L.p(seeds.cuda()), L.p(torch.tensor(draw, dtype=torch.int64).cuda()), L.p(rows.cuda()),
               L.i(B), L.i(ns), L.i(zdim), L.i(KL), L.p(out[0]), L.p(out[1]), L.p(out[2]) if pair else L.p(None),
               L.p(out[3]) if pair else L.p(None), L.stream_ptr())
        torch.cuda.synchronize()
        return out

    base = old(seeds, rows)
    same = new(list(range(B)))
    assert torch.equal(bits(same), bits(base)) and bool(base[:n_out, 0].any())
    assert bool(torch.isnan(base[n_out:]).all()) and not bool(torch.isnan(base[:n_out]).any())      # the single-pair form writes two
    perm = [3, 0, 4, 1, 2]
    at = torch.tensor(perm)
    seeds_p, rows_p = torch.empty_like(seeds), torch.empty_like(rows)
    seeds_p[at], rows_p[at] = seeds, rows                    # slot perm[b] of the old entry does what slot b does here
    want = old(seeds_p, rows_p)
    got = new(perm)
    for b in range(B):
        assert torch.equal(got[:n_out, b], want[:n_out, perm[b]]), b
    assert not torch.equal(got[:n_out, 0], base[:n_out, 0])   # another draw slot: other draws


# ------------------------------------------------------------------------------------------------ 3. slot-index check
def test_a_signal_gives_the_same_bits_in_slot_0_and_slot_2():
    """What moving between slot indices rests on: position b of the batch plays no part in a stream's arithmetic (the K split of
    idv_stream_cconv_splits depends on the batch size B, not on the slot).  Holds on the code before save / load existed."""
    a = _ref_dccrn(3, 0)
    assert a.shape == (1200,) and torch.equal(a, _ref_dccrn(3, 2))


# ------------------------------------------------------------------------------------------------- 4. a move midway
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_move_midway_is_bit_identical(cut):
    """Signal a runs in slot 2 of st1 to the cut, is saved, dropped and loaded into slot 0 of other objects, whose other slots are
    busy elsewhere: as device states, through .cpu() / tobytes() / frombytes(), and into the MFMA engine with another
    frames_per_launch."""
    S = _mods()[1]
    plans = {n: _host_plan(n) for n in CUTS}
    assert {v[4] for v in plans.values()} == {0, 1} and {v[4] for v in plans.values() if v[1]} == {0, 1}     # both parities
    assert plans[1][1] == 0 and any(v[3] for v in plans.values()) and plans[300][0] < NFFT < plans[777][0] and plans[800][0] % HOP == 0
    m, a = _model(), _signals()[0]
    want = _ref_dccrn(3, 2)
    src = _Feeder(S.StreamingSessions(m, slots=3, frames_per_launch=8), 2, a)
    for n in CUTS[cut]:
        src.step(n)
    st1 = src.st
    state = st1.save([2])[0]
    assert state.kind == "dccrn" and state.plan == plans[cut] == st1.sessions.slot_state(2) and state.data.is_cuda
    assert state.seed is None and state.draw_slot is None
    st1.drop([2])
    assert st1.positions[2] == 0 and st1.positions[0] > 0
    head = torch.cat(src.out)
    assert torch.equal(head, want[:len(head)])                # everything returned before the move
    for how in ("device", "bytes", "mfma"):
        st2 = S.StreamingSessions(m, slots=3, **(dict(frames_per_launch=5, conv="mfma") if how == "mfma" else dict(frames_per_launch=8)))
        dst = _Feeder(st2, 0, a, pos=cut)
        for b in dst.busy:                                    # the other slots are in mid-signal when the stream arrives
            dst.busy[b][1] = 100 * b
        _push(st2, {b: _signals()[3][:100 * b] for b in dst.busy})
        given = state
        if how == "bytes":
            given = S.SlotState.frombytes(state.cpu().tobytes())
            assert given.data.device.type == "cpu" and given.plan == state.plan and given.layout == state.layout
        st2.load([0], [given])
        assert st2.positions[0] == cut and st2.sessions.slot_state(0) == state.plan
        dst.run(ODD)
        assert st2.positions[0] == 0
        got = torch.cat([head, dst.cat()])
        assert got.shape == want.shape and torch.equal(got, want), how


# --------------------------------------------------------------------------------------------------------- 5. a fork
def test_fork_source_and_copy_continue_alike_and_save_changes_nothing():
    S = _mods()[1]
    m, a = _model(), _signals()[0]
    want = _ref_dccrn(3, 2)
    st = S.StreamingSessions(m, slots=3, frames_per_launch=8)
    src = _Feeder(st, 2, a, busy=[0]).run([100, 250, 37], to=777)
    states = st.save([2, 0])
    assert states[0].data.data_ptr() + 4 * states[0].data.numel() == states[1].data.data_ptr()      # rows of one tensor
    assert [s.plan[0] for s in states] == [777, st.positions[0]]
    st.load([1], states[:1])                                  # slot 1 is free: the copy lives next to its source
    assert st.positions[1] == st.positions[2] == 777
    outs = {1: [], 2: []}
    pos = 777
    for j in range(99):
        n = min(ODD[j % len(ODD)], len(a) - pos)
        got, mm = _push(st, {1: a[pos:pos + n], 2: a[pos:pos + n]}, [1, 2] if pos + n == len(a) else [])
        assert mm[1] == mm[2]
        for b in outs:
            outs[b].append(got[b])
        pos += n
        if pos == len(a):
            break
    tail = torch.cat(outs[2])
    assert torch.equal(tail, torch.cat(outs[1]))
    assert torch.equal(torch.cat([src.cat(), tail]), want)    # the source: as without the save
    # overwrite=True abandons what the target served
    st.load([0], states[:1], overwrite=True)
    assert st.positions == [777, 0, 0]
    dst = _Feeder(st, 0, a, pos=777, busy=[]).run(ODD)
    assert torch.equal(dst.cat(), tail)


# ------------------------------------------------------------------------------------------------------- 6. nine slots
def test_nine_slots_from_slot_8_to_slot_7_across_the_lstm_tile():
    S = _mods()[1]
    m, a = _model(), _signals()[0]
    want = _ref_dccrn(9, 8)
    st = S.StreamingSessions(m, slots=9, frames_per_launch=8)
    src = _Feeder(st, 8, a, busy=[0, 3, 6]).run([100, 250, 37], to=777)
    state = st.save([8])[0]
    st.drop([8])
    st.load([7], [state])
    dst = _Feeder(st, 7, a, pos=777, busy=[0, 3, 6])
    for b in dst.busy:
        dst.busy[b][1] = src.busy[b][1]
    dst.run(ODD)
    assert torch.equal(torch.cat([src.cat(), dst.cat()]), want)


# ---------------------------------------------------------------------------------------------- 7. another slot count
@pytest.mark.parametrize("slots,busy", [(5, None), (256, [0, 1, 7])])
def test_three_slots_to_another_slot_count_within_tolerance(slots, busy):
    """The K split of the conv blocks depends on the batch, so the sum order may differ between slot counts: identical before the
    move, within the streaming tolerance after it, the same sample counts call by call.  3 and 5 slots happen to split alike
    (idv_stream_cconv_splits gives the same parts up to 16 slots); 256 slots split two decoder blocks otherwise."""
    S = _mods()[1]
    m, a = _model(), _signals()[0]
    want = _ref_dccrn(3, 2)
    sizes = [100, 250, 37, 300, 90] + ODD * 3
    whole = _Feeder(S.StreamingSessions(m, slots=3, frames_per_launch=8), 2, a).run(sizes)
    assert torch.equal(whole.cat(), want)
    src = _Feeder(S.StreamingSessions(m, slots=3, frames_per_launch=8), 2, a).run(sizes, to=777)
    state = src.st.save([2])[0]
    st5 = S.StreamingSessions(m, slots=slots, frames_per_launch=8)
    assert ([cp.nsplit for cp in st5.enc + st5.dec] != [cp.nsplit for cp in src.st.enc + src.st.dec]) == (slots == 256)
    st5.load([slots - 1], [state])
    dst = _Feeder(st5, slots - 1, a, pos=777, busy=busy).run(ODD)
    head, tail = src.cat(), dst.cat()
    assert torch.equal(head, want[:len(head)])
    assert src.m + dst.m == whole.m and len(head) + len(tail) == len(want)
    err = relerr(tail, want[len(head):])
    print(f"3 slots -> {slots} slots, samples after the move against the uninterrupted stream: {err:.3e}")
    assert err < TOL


# ----------------------------------------------------------------------------------------------------------- 8. guards
def test_refused_loads_change_nothing():
    S = _mods()[1]
    m, a = _model(), _signals()[0]
    enc, ds, _ = _trio()
    pair = [_Feeder(S.StreamingSessions(m, slots=3, frames_per_launch=8), 0, a, busy=[2]).run([100, 250], to=500) for _ in range(2)]
    st = pair[0].st
    good = pair[1].st.save([0])[0]
    base12 = S.StreamingSessions(_model(12, 5), slots=3, frames_per_launch=8).save([1])[0]
    vae = S.StreamingVAESessions(enc, ds, slots=3, frames_per_launch=8).save([1])[0]
    assert base12.kind == "dccrn" and base12.layout != good.layout and vae.kind == "vae"
    tampered = S.SlotState(good.kind, good.layout, good.plan[:1] + (good.plan[1] + 1,) + good.plan[2:], good.data)
    short = S.SlotState(good.kind, good.layout, good.plan, good.data[:-1])
    refused = {
        "busy target": ([0], [good]),
        "duplicate target": ([1, 1], [good, good]),
        "base-12 state": ([1], [base12]),
        "VAE state": ([1], [vae]),
        "lengths": ([1], [good, good]),
        "no states": ([1], []),
        "slot out of range": ([3], [good]),
        "tampered plan": ([1], [tampered]),
        "short data": ([1], [short]),
        "not a state": ([1], [good.data]),
    }
    snap = st.sessions.snapshot()
    for name, (slots, states) in refused.items():
        with pytest.raises(ValueError):
            st.load(slots, states)
        assert st.positions == pair[1].st.positions and st.sessions.snapshot() == snap, name
    with pytest.raises(ValueError):
        st.save([0, 0])
    with pytest.raises(ValueError):
        st.save([3])
    assert st.save([]) == [] and st.load([], []) is None
    for f in pair:
        f.run(ODD)
    assert torch.equal(pair[0].cat(), pair[1].cat()) and torch.equal(pair[0].cat(), _ref_dccrn(3, 0))


# -------------------------------------------------------------------------------------------------------- 9. VAE kinds
def _vae_move(make, make_ref, names=None):
    """Signal a in slot 2 with a seed of its own to sample 777, then into slot 0 of a second object -> what the lock-step
    streamer with that seed returns for the signal whole in slot 2."""
    S = _mods()[1]
    a = _signals()[0]
    SEED = 2 ** 40 + 3
    st1 = make(9)
    st1.set_seed([2], SEED)
    src = _Feeder(st1, 2, a).run([100, 250, 37], to=777)
    assert st1.draw_slots == [0, 1, 2]
    if names is not None:
        assert "idv_stream_eps_pair_rows" in names and "idv_stream_eps_pair_rows_as" not in names     # never loaded: as before
        del names[:]
    state = S.SlotState.frombytes(st1.save([2])[0].tobytes())
    assert (state.seed, state.draw_slot, state.plan[0]) == (SEED, 2, 777)
    st1.drop([2])
    st2 = make(1)
    dst = _Feeder(st2, 0, a, pos=777)
    st2.load([0], [state])
    assert st2.draw_slots == [2, 1, 2] and st2.seeds == [SEED, 1, 1] and st2.positions[0] == 777
    with pytest.raises(ValueError):
        st2.set_seed([0], 4)                                  # a loaded slot is mid-signal
    with pytest.raises(ValueError):
        st2.seed = 4
    ref = make_ref(SEED)
    mine, theirs = st2.eps(3, 2), ref.eps(3, 2)
    assert all(torch.equal(u[0], v[2]) for u, v in zip(mine, theirs))
    dst.run(ODD[:2], to=1000)
    assert st2.draw_slots == [2, 1, 2]
    dst.run(ODD)
    assert st2.draw_slots == [0, 1, 2] and st2.seeds == [SEED, 1, 1] and st2.positions[0] == 0
    want = _lockstep(ref, 2, a)
    got = torch.cat([src.cat(), dst.cat()])
    assert got.shape == want.shape and torch.equal(got, want)
    if names is not None:
        assert "idv_stream_eps_pair_rows_as" in names
        del names[:]
        _push(st2, {0: a[:300]})                              # the moved signal has ended: the slot draws as itself again
        assert "idv_stream_eps_pair_rows" in names and "idv_stream_eps_pair_rows_as" not in names
    # a state of another seed or class option does not fit another kind
    with pytest.raises(ValueError):
        S.StreamingSessions(_model(), slots=3, frames_per_launch=8).load([0], [state])


def test_vae_sessions_move_keeps_seed_and_draw_slot(monkeypatch):
    S = _mods()[1]
    names = []
    real = S.call
    monkeypatch.setattr(S, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    enc, ds, _ = _trio()
    _vae_move(lambda seed: S.StreamingVAESessions(enc, ds, slots=3, seed=seed, frames_per_launch=8),
              lambda seed: S.StreamingVAE(enc, ds, batch=3, seed=seed, frames_per_launch=8), names)


@pytest.mark.parametrize("outtype", ["phase_mask", "clean_direct"])
def test_two_latent_sessions_move(outtype):
    S = _mods()[1]
    enc, ds, dn = _trio()
    _vae_move(lambda seed: S.StreamingVAETwoLatentsSessions(enc, ds, dn, slots=3, outtype=outtype, phase=2, seed=seed, frames_per_launch=8),
              lambda seed: S.StreamingVAETwoLatents(enc, ds, dn, batch=3, outtype=outtype, phase=2, seed=seed, frames_per_launch=8))


# ----------------------------------------------------------------------------------------------- 10. resampler and rates
@pytest.mark.parametrize("fs_in,fs_out", [(44100, 16000), (16000, 44100)])
def test_resampler_sessions_move(fs_in, fs_out):
    S = _mods()[1]
    b = _signals()[1]
    x = torch.zeros(3, len(b), device="cuda")
    x[2] = b
    lock = S.StreamingResampler(fs_in, fs_out, 3)
    want = torch.cat([lock.push(x), lock.flush()], dim=1)[2]
    src = _Feeder(S.StreamingResamplerSessions(fs_in, fs_out, 3), 2, b).run([441, 1, 300], to=1000)
    state = src.st.save([2])[0]
    assert state.kind == "resampler" and state.plan[0] == 1000
    src.st.drop([2])
    st2 = S.StreamingResamplerSessions(fs_in, fs_out, 5)      # a resampled row's bits do not depend on the slot count
    dst = _Feeder(st2, 0, b, pos=1000)
    st2.load([0], [S.SlotState.frombytes(state.tobytes())])
    with pytest.raises(ValueError):
        S.StreamingResamplerSessions(fs_out, fs_in, 3).load([0], [state])
    dst.run(ODD)
    got = torch.cat([src.cat(), dst.cat()])
    assert got.shape == want.shape and torch.equal(got, want)


def test_sessions_at_rate_move_and_refused_stage():
    S = _mods()[1]
    m, b = _model(), _signals()[1]
    fs = 44100
    x = torch.zeros(3, len(b), device="cuda")
    x[2] = b
    lock = S.AtRate(S.StreamingDCCRN(m, batch=3, frames_per_launch=8), fs)
    want = torch.cat([lock.push(x), lock.flush()], dim=1)[2]
    src = _Feeder(S.SessionsAtRate(S.StreamingSessions(m, slots=3, frames_per_launch=8), fs), 2, b).run([441, 1, 300], to=1000)
    state = src.st.save([2])[0]
    assert state.kind == "at_rate" and [s.kind for s in state.stages] == ["resampler", "dccrn", "resampler"]
    assert state.stages[0].plan[0] == 1000
    src.st.drop([2])
    state = S.SlotState.frombytes(state.cpu().tobytes())
    st2 = S.SessionsAtRate(S.StreamingSessions(m, slots=3, frames_per_launch=8), fs)
    dst = _Feeder(st2, 0, b, pos=1000)
    _push(st2, {1: _signals()[2][:500]})
    # a network stage that does not fit (a base-12 model's): refused before the resampler stages change
    other = S.StreamingSessions(_model(12, 5), slots=3, frames_per_launch=8).save([0])[0]
    bad = S.SlotState("at_rate", state.layout, (), state.data, stages=[state.stages[0], other, state.stages[2]])
    apart = S.SlotState("at_rate", state.layout, (), state.data,
                        stages=[state.stages[0], state.stages[1], S.SlotState("resampler", state.stages[2].layout, (5, 1), state.stages[2].data)])
    before = (st2.positions, st2.sessions.positions, st2.up.positions, st2.down.hist.clone(), st2.up.hist.clone())
    for wrong in (bad, apart, state.stages[1]):
        with pytest.raises(ValueError):
            st2.load([0], [wrong])
        assert (st2.positions, st2.sessions.positions, st2.up.positions) == before[:3]
        assert torch.equal(st2.down.hist, before[3]) and torch.equal(st2.up.hist, before[4])
    st2.load([0], [state])
    assert st2.positions[0] == 1000
    dst.run(ODD + [441])
    got = torch.cat([src.cat(), dst.cat()])
    assert got.shape == want.shape and torch.equal(got, want)
