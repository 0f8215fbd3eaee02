"""CPU tests of the streaming resampler's host side (streaming.ResamplePlan / ResampleSessionPlan, the guards, the float64
restatement tests/stream_resample_ref.py against scipy, idv_stream_resample_rows_check and the library entries); no GPU needed."""
import importlib
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_resample_ref as R  # noqa: E402

S = importlib.import_module("i-dccrn-vae_amd.streaming")
OPS = importlib.import_module("i-dccrn-vae_amd.ops")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")

# 48k -> 16k, 16k -> 48k, 44.1k -> 16k, 16k -> 44.1k, 8k -> 16k, 22.05k -> 16k, and the two ratios with max(up, down) = 640
RATES = [(48000, 16000), (16000, 48000), (44100, 16000), (16000, 44100), (8000, 16000), (22050, 16000), (640, 1), (1, 640)]
H_TABLE = {(48000, 16000): 61, (16000, 48000): 21, (44100, 16000): 56, (16000, 44100): 21, (640, 1): 12801}
NEW_ENTRIES = ["idv_stream_resample_hist", "idv_stream_resample_final", "idv_stream_resample", "idv_stream_resample_row_fields",
               "idv_stream_resample_rows_check", "idv_stream_resample_rows"]
F = {name: j for j, name in enumerate(OPS.SR_ROW_FIELDS)}


def _lengths(H):
    return sorted({1, 2, H - 1, H, H + 1, 257, 2345})


@pytest.mark.parametrize("fs_in,fs_out", RATES)
def test_ref_equals_scipy_and_plan_counts(fs_in, fs_out):
    """The state machine of the ref (history of H samples, n_final, flush) is scipy.signal.resample_poly for every cut, and
    ResamplePlan returns the ref's sample counts push by push."""
    from scipy import signal as sig
    up, down = OPS.resample_ratio(fs_in, fs_out)
    rs = R.RefResampler(up, down)
    assert np.array_equal(rs.h, OPS.resample_taps_host(up, down))
    plan = S.ResamplePlan(up, down)
    assert plan.H == rs.H == OPS.stream_resample_hist(up, down) == H_TABLE.get((fs_in, fs_out), rs.H)
    rng = np.random.RandomState(up * 1000 + down)
    worst = 0.0
    for L in _lengths(rs.H):
        x = rng.randn(L)
        want = sig.resample_poly(x, up, down)
        for name, sizes in R.chunkings(L, down, L).items():
            y, counts = R.run(rs, x, sizes)
            assert len(y) == len(want) == plan.n_out(L), (L, name)
            err = np.linalg.norm(y - want) / np.linalg.norm(want)
            worst = max(worst, err)
            assert err < 1e-12, (L, name, err)
            got = []
            for s in sizes:
                st = plan.push(s)
                assert st.n0 == plan.n_final(st.P0) and st.P0 + s == plan.n
                got.append(st.n1 - st.n0)
            st = plan.flush()
            got.append(st.n1 - st.n0)
            assert st.n1 == len(want) and plan.n == L
            plan.reset()
            assert got == counts, (L, name)
    print(f"{fs_in} -> {fs_out}: worst relative difference from scipy {worst:.2e}")


def test_plan_snapshot_restore_and_advance():
    plan = S.ResamplePlan(160, 441)
    plan.push(100)
    snap = plan.snapshot()
    a = [plan.push(n) for n in (441, 0, 37)]
    fl = plan.flush()
    plan.restore(snap)
    assert plan.n == 100 and plan.snapshot() == snap
    assert [plan.push(n) for n in (441, 0, 37)] == a and plan.flush() == fl
    # advance: periods * down inputs and periods * up outputs further on, the parity untouched
    plan.restore(snap)
    par, em = plan.parity, plan.emitted
    plan.advance(1 << 25)                                       # > 2^33 input samples
    assert plan.n == 100 + (1 << 25) * 441 > 2 ** 33 and plan.emitted == em + (1 << 25) * 160 and plan.parity == par
    b = [plan.push(n) for n in (441, 0, 37)]
    assert [(s.n1 - s.n0, s.parity) for s in b] == [(s.n1 - s.n0, s.parity) for s in a]
    fresh = S.ResamplePlan(160, 441)
    with pytest.raises(ValueError):
        fresh.advance(1)                                        # before the first half filter length has arrived
    assert fresh.n == 0


def test_plan_guards():
    for bad in [(0, 1), (1, 0), (2, 4), (641, 1), (1, 641), (True, 3), (1.0, 3)]:
        with pytest.raises(ValueError):
            S.ResamplePlan(*bad)
    plan = S.ResamplePlan(1, 3)
    plan.push(10)
    snap = plan.snapshot()
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            plan.push(bad)
        assert plan.snapshot() == snap
    with pytest.raises(ValueError):
        S.ResampleSessionPlan(0, 1, 3)
    sp = S.ResampleSessionPlan(2, 1, 3)
    sp.push([5, 0], [])
    snap = _state(sp)
    for counts, end in [([1], []), ([1, -1], []), ([1, 2], [2]), ([1, 2.0], []), ([1, 2], [True])]:
        with pytest.raises(ValueError):
            sp.push(counts, end)
        assert _state(sp) == snap and sp.positions == [5, 0]


def _state(sp):
    """A sessions plan's snapshot as plain lists."""
    return [v.tolist() for v in sp.snapshot()]


def _staggered(seed, slots=4, width=300):
    """A seeded schedule of calls (counts, end) for ``slots`` slots: staggered starts, idle calls, ends with the last samples or
    in a later call, the end of a slot that has received nothing, second signals."""
    rng = random.Random(seed)
    todo = {b: [rng.choice([1, 61, 257, 900]), rng.choice([2, 500])] for b in range(slots)}
    start = {b: 2 * b for b in range(slots)}
    left, calls, pending = {}, [], set()
    ci = 0
    while any(todo.values()) or left or pending:
        counts, end = [0] * slots, sorted(pending)
        pending = set()
        for b in range(slots):
            if b in end:
                continue
            if b not in left and todo[b] and ci >= start[b]:
                left[b] = todo[b].pop(0)
            if b not in left:
                if rng.random() < 0.2:
                    end.append(b)                                # ending a slot that has received nothing
                continue
            n = min(rng.choice([0, 1, 37, 100, width]), left[b])
            counts[b] = n
            left[b] -= n
            if left[b] == 0:
                del left[b]
                (end.append(b) if rng.random() < 0.5 else pending.add(b))
        calls.append((counts, sorted(end)))
        ci += 1
    return calls


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (441, 160)])
def test_sessions_plan_equals_lockstep_plan_per_slot(up, down):
    """Under staggered starts and ends every slot's rows are what a lock-step plan of its own gives, and the library's
    idv_stream_resample_rows_check passes every table."""
    slots = 4
    lib = LIB.lib()
    for seed in range(3):
        sp = S.ResampleSessionPlan(slots, up, down)
        own = [S.ResamplePlan(up, down) for _ in range(slots)]
        ended = 0
        for counts, end in _staggered(seed, slots):
            call = sp.push(counts, end)
            host = torch.from_numpy(call.rows.ravel().copy())
            assert call.rows.shape == (slots, len(OPS.SR_ROW_FIELDS)) and host.dtype == torch.int64
            assert lib.idv_stream_resample_rows_check(host.data_ptr(), slots, max(counts), up, down, own[0].H, max(call.m)) == 0
            for b in range(slots):
                r = call.rows[b].tolist()
                had = own[b].n
                st = own[b].push(counts[b])
                ends = b in end and own[b].n > 0
                m = (own[b].flush().n1 if ends else st.n1) - st.n0
                assert r == [had, counts[b], st.n0, m, st.parity, int(ends), int(counts[b] == 0 and not ends)], (seed, b)
                assert call.m[b] == m
                if ends:
                    own[b].reset()
                    ended += 1
                assert (b in call.zero) == ends
            assert sp.positions == [pl.n for pl in own]
        assert ended == 2 * slots and sp.positions == [0] * slots
    # snapshot / restore and drop
    sp = S.ResampleSessionPlan(2, up, down)
    sp.push([100, 7], [])
    snap = sp.snapshot()
    a = sp.push([50, 0], [1])
    assert sp.positions == [150, 0]
    sp.restore(snap)
    assert sp.positions == [100, 7] and _state(sp) == [v.tolist() for v in snap]
    b = sp.push([50, 0], [1])
    assert b.rows.tolist() == a.rows.tolist() and b.m == a.m and b.zero == a.zero == [1]
    sp.drop([0])
    sp.drop([])
    assert sp.positions == [0, 0] and _state(sp)[1] == [0, 0]


def test_rows_check_refuses_bad_tables():
    lib = LIB.lib()
    up, down = 1, 3
    H = OPS.stream_resample_hist(up, down)
    sp = S.ResampleSessionPlan(3, up, down)
    sp.push([100, 40, 0], [])
    good = sp.push([30, 12, 0], [1]).rows.tolist()
    ldy = max(r[F["m"]] for r in good)

    def rc(rows, n_x=30, ldy=ldy, H=H, up=up, down=down):
        host = torch.tensor([v for r in rows for v in r], dtype=torch.int64)
        return lib.idv_stream_resample_rows_check(host.data_ptr(), len(rows), n_x, up, down, H, ldy)

    assert rc(good) == 0
    assert rc(good, n_x=29) != 0 and rc(good, ldy=ldy - 1) != 0 and rc(good, H=H + 1) != 0 and rc(good, up=2, down=6) != 0
    for field, delta in [("P0", 3), ("P0", -200), ("count", 1), ("count", -31), ("n0", 1), ("n0", -1), ("m", 1), ("m", -1), ("parity", 2),
                         ("end", 1), ("end", 2), ("idle", 1)]:
        rows = [list(r) for r in good]
        rows[0][F[field]] += delta
        assert rc(rows) != 0, (field, delta)
    rows = [list(r) for r in good]
    rows[2][F["idle"]] = 0                                       # no samples and no end is idle
    assert rc(rows) != 0
    rows = [list(r) for r in good]
    rows[1][F["end"]] = 0                                        # the outputs of an end without the end
    assert rc(rows) != 0


def test_library_entries_and_host_formulas():
    with open(LIB.HEADER_PATH) as f:
        src = f.read()
    lib = LIB.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in LIB.declared_symbols() and hasattr(lib, name), name
    assert int(lib.idv_stream_resample_row_fields()) == len(OPS.SR_ROW_FIELDS) == 7
    assert re.search(r"#define\s+IDV_SR_ROW_FIELDS\s+7\b", src)
    for j, name in enumerate(OPS.SR_ROW_FIELDS):
        assert re.search(r"#define\s+IDV_SR_ROW_%s\s+%d\b" % (name.upper(), j), src), name
    for mode, v in OPS.SR_TAPS_MODES.items():
        assert re.search(r"#define\s+IDV_SR_TAPS_%s\s+%d\b" % (mode.upper(), v), src), mode
    for fs_in, fs_out in RATES:
        up, down = OPS.resample_ratio(fs_in, fs_out)
        assert lib.idv_stream_resample_hist(up, down) == OPS.stream_resample_hist(up, down)
        for P in (0, 1, 9, 10, 11, 30, 31, 1000, 2 ** 33 + 5, 2 ** 50):
            assert lib.idv_stream_resample_final(P, up, down) == OPS.stream_resample_final(P, up, down), (up, down, P)
    assert lib.idv_stream_resample_hist(2, 6) == -1 and lib.idv_stream_resample_hist(641, 1) == -1
    assert lib.idv_stream_resample_final(-1, 1, 3) == -1 and lib.idv_stream_resample_final(2 ** 50 + 1, 1, 3) == -1
    # the lock-step entry refuses, before any launch, a NULL history and an output range that is not the definition's: at P0 = 100
    # of 1/3 the next output is n_final(100) = 24 and an empty push returns none (host buffers stand in: nothing is dereferenced)
    buf = torch.zeros(2 * 61)
    assert OPS.stream_resample_final(100, 1, 3) == 24
    assert lib.idv_stream_resample(None, 61, 0, None, 0, 0, 100, 0, 24, 0, 1, 1, 3, buf.data_ptr(), 0, None, 0, None) == -1
    for n0, m in ((23, 0), (25, 0), (24, 1)):
        assert lib.idv_stream_resample(buf.data_ptr(), 61, 0, None, 0, 0, 100, 0, n0, m, 1, 1, 3, buf.data_ptr(), 0, buf.data_ptr(), 1,
                                       None) == -1, (n0, m)


def test_construction_guards_need_no_gpu():
    """The construction guards run before any GPU work: they raise on a machine without one."""
    for cls in (S.StreamingResampler, S.StreamingResamplerSessions):
        for bad in [(0, 16000, 1), (48000, -1, 1), (48000.0, 16000, 1), (16000, 16000, 1), (1, 641, 1), (48000, 16000, 0),
                    (48000, 16000, True)]:
            with pytest.raises(ValueError):
                cls(*bad)
        with pytest.raises(ValueError):
            cls(48000, 16000, 2, taps_mode="fast")
    for cls in (S.AtRate, S.SessionsAtRate):
        with pytest.raises(ValueError):
            cls(object(), 48000)
