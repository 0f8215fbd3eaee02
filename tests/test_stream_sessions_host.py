"""CPU tests of streaming sessions (streaming.SessionPlan, the guards of StreamingSessions.push, idv_stream_rows_check): per-slot
counts, a float64 replay of the row tables with an identity network, the guards and the library entries; no GPU needed."""
import importlib
import os
import random
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S = importlib.import_module("i-dccrn-vae_amd.streaming")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")

N_FFT, HOP, WIN = 512, 100, 400
HALF, LEFT = N_FFT // 2, (N_FFT - WIN) // 2
WIDTH = 250                                     # columns of every call's x
F = {name: j for j, name in enumerate(S.ROW_FIELDS)}
NEW_ENTRIES = ["idv_stream_row_fields", "idv_stream_rows_check", "idv_stream_frames_rows", "idv_stream_ring_rows",
               "idv_stream_ola_rows", "idv_stream_cconv_rows", "idv_stream_clstm_rows", "idv_stream_zero_rows"]


def _schedule(seed):
    """A seeded schedule for 3 slots: (calls, signals).  calls: [(x [3, WIDTH] float64 with NaN behind counts[b], counts, end)];
    signals: [(slot, samples, [(call index, count)])].  Slot 0 runs 1600 samples from call 0, slot 1 runs 257 and then 401
    samples from call 2, slot 2 runs 300 samples from call 5; an end comes with the last samples or in a later call."""
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    todo = {0: [1600], 1: [257, 401], 2: [300]}
    start = {0: 0, 1: 2, 2: 5}
    cur = {}                                    # slot -> [signal index, samples, position, calls so far]
    signals, calls = [], []
    pending_end = set()
    ci = 0
    while any(todo.values()) or cur or pending_end:
        x = torch.full((3, WIDTH), float("nan"), dtype=torch.float64)
        counts, end = [0, 0, 0], sorted(pending_end)
        pending_end = set()
        for b in range(3):
            if b in end:
                continue
            if b not in cur and todo[b] and ci >= start[b]:
                L = todo[b].pop(0)
                cur[b] = [len(signals), torch.randn(L, generator=g, dtype=torch.float64), 0]
                signals.append((b, cur[b][1], []))
            if b not in cur:
                continue
            idx, sig, pos = cur[b]
            n = min(rng.choice([0, 1, 37, 100, 250]), len(sig) - pos)
            x[b, :n] = sig[pos:pos + n]
            counts[b] = n
            signals[idx][2].append((ci, n))
            cur[b][2] = pos + n
            if pos + n == len(sig):
                del cur[b]
                (end.append(b) if rng.random() < 0.5 else pending_end.add(b))
        calls.append((x, counts, sorted(end)))
        ci += 1
    return calls, signals


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_counts_follow_an_independent_plan_per_signal(seed):
    calls, signals = _schedule(seed)
    sp = S.SessionPlan(3, N_FFT, HOP, WIN, cap=4)
    got = [sp.push(counts, end).m for _, counts, end in calls]
    assert sorted(len(sig) for _, sig, _ in signals) == [257, 300, 401, 1600]
    for slot, sig, pushes in signals:
        pl = S.StreamPlan(N_FFT, HOP, WIN, cap=4)
        total = 0
        for j, (ci, n) in enumerate(pushes):
            want = sum(c.e1 - c.e0 for c in pl.push(n))
            ends_here = slot in calls[ci][2]
            if ends_here:
                want += sum(c.e1 - c.e0 for c in pl.flush())
            assert got[ci][slot] == want, (slot, ci)
            total += want
        last = pushes[-1][0]
        if slot not in calls[last][2]:                       # the end came in a later call, without samples
            nxt = next(ci for ci in range(last + 1, len(calls)) if slot in calls[ci][2])
            want = sum(c.e1 - c.e0 for c in pl.flush())
            assert got[nxt][slot] == want
            total += want
        assert total == HOP * (len(sig) // HOP)
    assert sp.positions == [0, 0, 0]


def _replay(calls, cap):
    """float64 replay of the row tables with an identity network: per slot, framing from the ring / this call's x[b, :count]
    with the mirrors, windowed overlap-add with the carry half its parity names, envelope and emission at y_off, exactly as the
    per-slot fields say.  Returns the (y, m) of every call."""
    w = torch.hann_window(WIN, periodic=True, dtype=torch.float64)
    sp = S.SessionPlan(3, N_FFT, HOP, WIN, cap=cap)
    ccap = sp.plans[0].carry_cap
    ring = torch.zeros(3, N_FFT, dtype=torch.float64)
    carry = torch.zeros(2, 3, ccap, dtype=torch.float64)
    outs = []

    def update_ring(x, rows):
        for b in range(3):
            n_prev, count = rows[b][F["n_prev"]], rows[b][F["count"]]
            for j in range(max(0, count - N_FFT), count):
                ring[b, (n_prev + j) % N_FFT] = x[b, j]

    for x, counts, end in calls:
        plan = sp.push(counts, end)
        y = torch.zeros(3, max(plan.m), dtype=torch.float64)
        ring_due = any(counts)
        for g in plan.groups:
            if g.flush and ring_due:
                update_ring(x, plan.groups[0].rows)
                ring_due = False
            assert g.k == max(r[F["k"]] for r in g.rows)
            for b, r in enumerate(g.rows):
                n_prev, count, L_end, t0, k, par, e0, e1, p_end, cin, T_total, y_off = r
                if k == 0 and e0 == e1:
                    continue
                assert (count == 0 and L_end == n_prev) if g.flush else L_end == -1
                P = torch.arange(HALF + e0, p_end)
                v = torch.zeros(len(P), dtype=torch.float64)
                v[:cin] = carry[par, b, :cin]
                for t in range(t0, t0 + k):
                    s = HOP * t + LEFT - HALF + torch.arange(WIN)
                    s = torch.where(s < 0, -s, s)
                    if L_end >= 0:
                        s = torch.where(s >= L_end, 2 * (L_end - 1) - s, s)
                    assert int(s.max()) < n_prev + count and n_prev - int(s.min()) <= N_FFT
                    smp = torch.where(s >= n_prev, x[b, (s - n_prev).clamp(0, WIDTH - 1)], ring[b, s % N_FFT])
                    i = P - HOP * t - LEFT
                    ok = (i >= 0) & (i < WIN)
                    v[ok] += (smp * w)[i[ok]] * w[i[ok]]
                T = T_total if T_total >= 0 else 10 ** 9
                env = torch.zeros(len(P), dtype=torch.float64)
                for t in range(max(0, (int(P.min()) - LEFT - WIN) // HOP), min(T, int(P.max()) // HOP + 1)):
                    i = P - HOP * t - LEFT
                    ok = (i >= 0) & (i < WIN)
                    env[ok] += w[i[ok]] ** 2
                ne = e1 - e0
                y[b, y_off:y_off + ne] = v[:ne] / env[:ne]
                carry[1 - par, b] = 0
                carry[1 - par, b, :len(P) - ne] = v[ne:]
        if ring_due:
            update_ring(x, plan.groups[0].rows)
        for b in plan.zero:
            ring[b] = 0
            carry[:, b] = 0
        outs.append((y, plan.m))
    return outs


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_row_tables_reproduce_stft_istft_per_signal(seed):
    calls, signals = _schedule(seed)
    assert any(c == 0 for _, counts, _ in calls for c in counts)
    assert any(counts[b] > 0 for _, counts, end in calls for b in end)        # an end with the last samples
    outs = _replay(calls, cap=2)
    w = torch.hann_window(WIN, periodic=True, dtype=torch.float64)
    for y, m in outs:
        assert not torch.isnan(y).any()
        for b in range(3):
            assert not y[b, m[b]:].any()
    for slot, sig, pushes in signals:
        first = pushes[0][0]
        last = next(ci for ci in range(pushes[-1][0], len(calls)) if slot in calls[ci][2])
        got = torch.cat([outs[ci][0][slot, :outs[ci][1][slot]] for ci in range(first, last + 1)])
        ref = torch.istft(torch.stft(sig[None], N_FFT, HOP, WIN, w, return_complex=True), N_FFT, HOP, WIN, w)[0]
        assert got.shape == ref.shape, (slot, len(sig))
        assert float((got - ref).abs().max()) < 1e-9, (slot, len(sig))


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU (there is none here)."""
    is_cuda = property(lambda self: True)


def test_guards_refuse_before_anything_changes():
    with pytest.raises(ValueError, match="GPU tensor"):
        S.check_counts(torch.tensor([1, 2, 3]).as_subclass(_OnGpu), 3, 10)
    with pytest.raises(ValueError, match="2 counts for 3 slots"):
        S.check_counts([1, 2], 3, 10)
    for bad in ([1, 2, 11], [1, -1, 3]):
        with pytest.raises(ValueError, match="0 .. 10"):
            S.check_counts(bad, 3, 10)
    with pytest.raises(ValueError, match="integers"):
        S.check_counts([1, 2.0, 3], 3, 10)
    assert S.check_counts(None, 3, 10) == [10, 10, 10]
    assert S.check_counts(torch.tensor([0, 10, 3]), 3, 10) == [0, 10, 3]
    with pytest.raises(ValueError, match="0 .. 2"):
        S.check_slots([3], 3)
    assert S.check_slots((2, 0, 2), 3) == [0, 2]

    sp = S.SessionPlan(3, N_FFT, HOP, WIN)
    sp.push([100, 250, 0], [])
    sp.push([100, 6, 0], [])
    before = (sp.positions, sp.snapshot())
    assert before[0] == [200, 256, 0]
    for counts in ([50, 0, 0], [6, 0, 7]):                   # slot 0 would end at 250 / 206 samples, slot 1 at 256
        for end in ([0], [1], [2, 1]):
            with pytest.raises(ValueError, match="n_fft/2"):
                sp.push(counts, end)
            assert (sp.positions, sp.snapshot()) == before
    call = sp.push([0, 0, 0], [2])                           # ending an untouched slot: nothing
    assert call.m == [0, 0, 0] and call.groups == [] and call.zero == []
    call = sp.push([0, 1, 0], [1])                           # 257 samples: the shortest signal that can end
    assert call.m == [0, 200, 0] and call.zero == [1] and sp.positions == [200, 0, 0]


def _check(rows, n_x, k, ldy, span, Tp=None, cap=None):
    host = torch.tensor([v for r in rows for v in r], dtype=torch.int64)
    return LIB.lib().idv_stream_rows_check(LIB._P(host.data_ptr()), len(rows), N_FFT, n_x, N_FFT, WIN, HOP,
                                           N_FFT + WIN if cap is None else cap, k, k + 1 if Tp is None else Tp, ldy, span)


def test_header_declares_and_library_exports_the_rows_entries():
    names, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for n in NEW_ENTRIES:
        assert n in names and n in protos, n
        assert hasattr(lib, n), n
    assert LIB.declared_abi_version() == 9 and int(lib.idv_stream_row_fields()) == len(S.ROW_FIELDS) == 12
    with open(LIB.HEADER_PATH) as f:
        src = f.read()
    for j, name in enumerate(S.ROW_FIELDS):
        assert re.search(rf"#define IDV_ROW_{name.upper()} {j}\s", src), name


def test_rows_check_accepts_the_plan_and_refuses_each_corruption():
    einval = -1
    calls, _ = _schedule(2)
    sp = S.SessionPlan(3, N_FFT, HOP, WIN, cap=4)
    seen = []
    for _, counts, end in calls:
        plan = sp.push(counts, end)
        for g in plan.groups:
            args = (0 if g.flush else WIDTH, g.k, max(plan.m), g.span)
            assert _check(g.rows, *args) == 0
            seen.append((g, args))
    # a push group in mid-signal with a working slot, the first group of a signal (start mirror), and a flush group
    mid = next((g, a) for g, a in seen if not g.flush and any(r[F["k"]] > 0 and r[F["t0"]] > 4 for r in g.rows))
    head = next((g, a) for g, a in seen if not g.flush and any(r[F["k"]] > 0 and r[F["t0"]] == 0 for r in g.rows))
    tail = next((g, a) for g, a in seen if g.flush)

    def corrupt(ga, pick, **fields):
        g, args = ga
        b = next(b for b, r in enumerate(g.rows) if pick(r))
        rows = [list(r) for r in g.rows]
        for name, fn in fields.items():
            rows[b][F[name]] = fn(rows[b][F[name]])
        return rows, args

    working = lambda r: r[F["k"]] > 0
    cases = {
        "a frame reads past x[b, :count]": corrupt(mid, working, count=lambda v: 0),
        "a frame reads behind the ring's reach": corrupt(mid, working, n_prev=lambda v: v + 2 * N_FFT, count=lambda v: 0),
        "count past the width of x": corrupt(mid, working, count=lambda v: WIDTH + 1),
        "the start mirror has gone from the ring": corrupt(head, lambda r: working(r) and r[F["t0"]] == 0, n_prev=lambda v: N_FFT + 1),
        "carry_in over the cap": corrupt(mid, working, carry_in=lambda v: N_FFT + WIN + 1),
        "outgoing carry over the cap": corrupt(mid, working, p_end=lambda v: v + N_FFT + WIN),
        "parity": corrupt(mid, working, parity=lambda v: 2),
        "y_off past ldy": corrupt(tail, working, y_off=lambda v: v + 10 ** 6),
        "p_end short of the last frame": corrupt(mid, working, p_end=lambda v: v - 1),
        "end mirror without T_total": corrupt(tail, working, T_total=lambda v: -1),
    }
    for what, (rows, args) in cases.items():
        assert _check(rows, *args) == einval, what
    g, args = mid
    assert _check(g.rows, args[0], g.k, args[2], args[3], Tp=g.k) == einval, "k over Tp - 1"
    assert _check(g.rows, args[0], g.k - 1, args[2], args[3], Tp=g.k + 1) == einval, "k_b over k_launch"
    assert _check(g.rows, args[0], g.k, args[2], args[3] - 1) == einval, "span over span_max"


def test_scalar_entries_refuse_what_rows_check_refuses():
    """The reach conditions of idv_stream_frames and the range conditions of idv_stream_ola are the ones idv_stream_rows_check
    holds a row to: a single-row table with one of them broken is refused, and so is the scalar entry given the same values.
    Refusals only (they come before any launch, so any non-null pointer will do); the tables that pass go to the check alone."""
    einval, cap, big = -1, N_FFT + WIN, 10 ** 6
    lib = LIB.lib()
    mem = torch.zeros(4)
    ptr = mem.data_ptr()
    pl = S.StreamPlan(N_FFT, HOP, WIN)
    pl.push(700)
    (c,) = pl.push(WIDTH)                            # mid-signal: frames 6 and 7, 300 carried positions in and out
    assert (c.t0, c.k, c.e0, c.e1, c.p_end, c.carry_in) == (6, 2, 400, 600, 1156, 300)
    mid = dict(n_prev=700, count=WIDTH, L_end=-1, t0=c.t0, k=c.k, parity=c.parity, e0=c.e0, e1=c.e1, p_end=c.p_end,
               carry_in=c.carry_in, T_total=-1, y_off=0)
    head = dict(n_prev=0, count=201, L_end=-1, t0=0, k=1, parity=0, e0=0, e1=0, p_end=LEFT + WIN, carry_in=0, T_total=-1, y_off=0)
    no_frames = dict(mid, k=0, carry_in=0, p_end=HALF + c.e1)         # output without frames, as a flush chunk may be

    def table(r):
        return _check([[r[name] for name in S.ROW_FIELDS]], WIDTH, max(r["k"], 1), r["e1"] - r["e0"], big)

    def frames(r):
        return lib.idv_stream_frames(ptr, N_FFT, ptr, WIDTH, r["count"], r["n_prev"], r["L_end"], 1, N_FFT, WIN, HOP, r["t0"], r["k"],
                                     ptr, r["k"] + 1, r["k"] + 1, None)

    def ola(r):
        return lib.idv_stream_ola(ptr, r["k"] + 1, r["k"] + 1, ptr, r["carry_in"], ptr, cap, 1, N_FFT, WIN, HOP, r["t0"], r["k"],
                                  r["T_total"], r["e0"], r["e1"], r["p_end"], ptr, r["e1"] - r["e0"], r["y_off"], None)

    for r in (mid, head, no_frames):
        assert table(r) == 0
    reach = {
        "hi_read: a frame reads past the new samples": dict(mid, count=0),
        "lo_read: a frame reads behind the ring's reach": dict(mid, n_prev=700 + 2 * N_FFT, count=0),
        "the deepest start-mirror sample has not arrived": dict(head, count=200),
        "the start mirror has gone from the ring": dict(head, n_prev=N_FFT + 1, count=0),
    }
    for what, r in reach.items():
        assert table(r) == einval and frames(r) == einval, what
    ranges = {
        "p_end < half + e1": dict(no_frames, p_end=HALF + c.e1 - 1),
        "carry_in > p_end - p_start": dict(mid, carry_in=c.p_end - (HALF + c.e0) + 1),
        "carry past cap": dict(mid, p_end=HALF + c.e1 + cap + 1),
        "last frame past p_end": dict(mid, p_end=c.p_end - 1),
    }
    for what, r in ranges.items():
        assert table(r) == einval and ola(r) == einval, what
