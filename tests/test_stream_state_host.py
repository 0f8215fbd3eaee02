"""Host side of saving, loading and moving a slot's stream (streaming.SlotState, SessionPlan / ResampleSessionPlan.slot_state,
idv_stream_state_check; no GPU): the bytes round trip and its refusals, a slot's host integers against ``snapshot``, the
self-consistency guard on a plan that comes from outside, the host check of the view and slot tables, and the four new entries in
the header and in the library."""
import importlib
import json
import random
import struct

import pytest
import torch

S = importlib.import_module("i-dccrn-vae_amd.streaming")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")

N_FFT, HOP, WIN = 512, 100, 400


# ------------------------------------------------------------------------------------------------------------ 1. SlotState
def _state(n=37, kind="vae"):
    g = torch.Generator().manual_seed(n)
    layout = (N_FFT, HOP, WIN, ((1, 512), (2, 912), (16, 96), (1028, 1)), 2, 16, 96, "speech", True)
    return S.SlotState(kind, layout, (777, 5, 443, 600, 1), torch.randn(n, generator=g), seed=2 ** 40 + 3, draw_slot=2)


def _same(a, b):
    assert (a.kind, a.layout, a.plan, a.seed, a.draw_slot) == (b.kind, b.layout, b.plan, b.seed, b.draw_slot)
    assert a.data.dtype == b.data.dtype == torch.float32
    assert torch.equal(a.data.cpu().view(torch.int32), b.data.cpu().view(torch.int32))            # bits: a NaN equals itself
    assert (a.stages is None) == (b.stages is None)
    for x, y in zip(a.stages or (), b.stages or ()):
        _same(x, y)


def test_bytes_round_trip():
    st = _state()
    st.data[3] = float("nan")                         # bits, not values
    st.data[4] = -0.0
    raw = st.tobytes()
    back = S.SlotState.frombytes(raw)
    assert back.data.device.type == "cpu" and isinstance(back.layout, tuple) and isinstance(back.layout[3][0], tuple)
    assert back.data.view(torch.int32).tolist() == st.data.view(torch.int32).tolist()
    assert (back.kind, back.layout, back.plan, back.seed, back.draw_slot) == (st.kind, st.layout, st.plan, st.seed, st.draw_slot)
    assert back.tobytes() == raw and S.SlotState.frombytes(bytearray(raw)).tobytes() == raw
    _same(st.cpu(), st)
    _same(st.to("cpu"), st)
    # a state without draws, and the nested form of SessionsAtRate
    plain = S.SlotState("resampler", (160, 441, 56, ((2, 56),)), (1234, 1), torch.arange(112.0))
    _same(S.SlotState.frombytes(plain.tobytes()), plain)
    three = S.SlotState("at_rate", (44100, 16000), (), torch.empty(0), stages=[plain, _state(9, "dccrn"), plain])
    back = S.SlotState.frombytes(three.tobytes())
    _same(back, three)
    assert len(back.stages) == 3 and back.data.numel() == 0


def test_frombytes_refuses_truncated_and_foreign_bytes():
    raw = _state().tobytes()
    hlen = struct.unpack("<I", raw[12:16])[0]
    bad = {
        "empty": b"",
        "short": raw[:10],
        "magic": b"NOTSLOT\x00" + raw[8:],
        "version": raw[:8] + struct.pack("<I", 2) + raw[12:],
        "header_cut": raw[:16 + hlen - 3],
        "header_len": raw[:12] + struct.pack("<I", len(raw)) + raw[16:],
        "payload_cut": raw[:-1],
        "payload_float_cut": raw[:-4],
        "payload_long": raw + b"\x00\x00\x00\x00",
        "not_json": raw[:16] + b"\xff" * hlen + raw[16 + hlen:],
    }
    for name, b in bad.items():
        with pytest.raises(ValueError):
            S.SlotState.frombytes(b)
        assert name
    with pytest.raises(ValueError):
        S.SlotState.frombytes("a string")

    def with_header(**change):
        head = json.loads(raw[16:16 + hlen])
        head.update(change)
        for k in [k for k, v in change.items() if v is KeyError]:
            del head[k]
        h = json.dumps(head).encode()
        return raw[:12] + struct.pack("<I", len(h)) + h + raw[16 + hlen:]
    assert S.SlotState.frombytes(with_header()).plan == (777, 5, 443, 600, 1)
    for change in (dict(kind="other"), dict(floats=36), dict(floats=-1), dict(floats="37"), dict(plan=[1, 2.5]), dict(plan="x"),
                   dict(seed="7"), dict(draw_slot=True), dict(layout=5), dict(stages=[148]), dict(extra=1), dict(seed=KeyError),
                   dict(floats=None), dict(kind="at_rate")):
        with pytest.raises(ValueError):
            S.SlotState.frombytes(with_header(**change))
    # stage lengths that do not add up
    plain = S.SlotState("resampler", (160, 441, 56, ((2, 56),)), (1234, 1), torch.arange(112.0))
    three = S.SlotState("at_rate", (44100, 16000), (), torch.empty(0), stages=[plain, plain, plain]).tobytes()
    for b in (three[:-1], three + b"\x00", three[:-len(plain.tobytes())]):
        with pytest.raises(ValueError):
            S.SlotState.frombytes(b)


# ---------------------------------------------------------------------------------------------- 2. a slot's host integers
def test_slot_state_is_the_row_of_snapshot_and_set_slot_state_writes_it():
    rng = random.Random(1)
    sp = S.SessionPlan(4, N_FFT, HOP, WIN, cap=8)
    for _ in range(12):
        sp.push([rng.choice([0, 1, 37, 100, 250, 300]) for _ in range(4)], [])
        snap = sp.snapshot()
        for b in range(4):
            assert sp.slot_state(b) == snap[b] and all(type(v) is int for v in sp.slot_state(b))
            sp.check_slot_state(sp.slot_state(b))              # whatever the cut and the chunk size: a plan a stream reaches
    other = S.SessionPlan(3, N_FFT, HOP, WIN, cap=64)
    other.set_slot_state(2, sp.slot_state(1))
    assert other.snapshot()[2] == sp.snapshot()[1] and other.snapshot()[:2] == [(0, 0, 0, 0, 0)] * 2
    assert other.positions == [0, 0, sp.positions[1]]
    # the moved slot goes on as the source does
    a = sp.push([0, 163, 0, 0], [1])
    b = other.push([0, 0, 163], [2])
    strip = lambda rows: [[v for j, v in enumerate(r) if S.ROW_FIELDS[j] != "y_off"] for r in rows]
    assert a.m[1] == b.m[2] and [strip(g.rows)[1] for g in a.groups] == [strip(g.rows)[2] for g in b.groups]
    rp = S.ResampleSessionPlan(3, 160, 441)
    rp.push([100, 0, 441], [])
    rp.push([7, 0, 0], [])
    snap = rp.snapshot()
    for b in range(3):
        assert rp.slot_state(b) == (int(snap[0][b]), int(snap[1][b])) and all(type(v) is int for v in rp.slot_state(b))
    assert rp.slot_state(0) == (107, 0) and rp.slot_state(1) == (0, 0) and rp.slot_state(2) == (441, 1)
    rp2 = S.ResampleSessionPlan(2, 160, 441)
    rp2.set_slot_state(1, rp.slot_state(2))
    assert rp2.positions == [0, 441] and rp2.slot_state(1) == (441, 1)


def test_plan_guard_refuses_a_plan_no_stream_reaches():
    sp = S.SessionPlan(2, N_FFT, HOP, WIN, cap=8)
    sp.push([777, 0], [])
    n, k, emitted, carry, parity = good = sp.slot_state(0)
    assert k > 0 and carry > 0
    sp.check_slot_state(good)
    sp.check_slot_state((n, k, emitted, carry, 1 - parity))
    sp.check_slot_state((0, 0, 0, 0, 0))
    for bad in ((n, k + 1, emitted, carry, parity), (n, k - 1, emitted, carry, parity), (n, k, emitted, carry + 1, parity),
                (n, k, emitted, 0, parity), (n, k, emitted + 100, carry, parity), (n, k, emitted, carry, 2),
                (n, k, emitted, carry, -1), (-1, 0, 0, 0, 0), (n, k, emitted, carry), (n, k, emitted, carry, True),
                (float(n), k, emitted, carry, parity), "nkecp", None):
        before = sp.snapshot()
        with pytest.raises(ValueError):
            sp.set_slot_state(1, bad)
        assert sp.snapshot() == before
    # a stream far along is checked without walking its chunks
    far = S.StreamPlan(N_FFT, HOP, WIN, 2 ** 40)
    far.push(2 ** 42 + 17)
    sp.check_slot_state((far.n, far.k, far.emitted, far.carry, 1))
    rp = S.ResampleSessionPlan(2, 160, 441)
    rp.check_slot_state((0, 0))
    rp.check_slot_state((2 ** 40, 1))
    for bad in ((-1, 0), (5, 2), (5, -1), (5,), (5, 0, 0), (5.0, 0), (True, 0), None):
        with pytest.raises(ValueError):
            rp.set_slot_state(0, bad)
    assert rp.positions == [0, 0]


# --------------------------------------------------------------------------------------------------- 3. the host check
def _check(views, B, slots, per):
    v = torch.tensor([q for row in views for q in row], dtype=torch.int64)
    s = torch.tensor(slots, dtype=torch.int64)
    return LIB.lib().idv_stream_state_check(LIB._P(v.data_ptr()), len(views), B, LIB._P(s.data_ptr()), len(slots), per)


def test_state_check_accepts_a_good_table_and_refuses_each_bad_one():
    A = 0x7f0000000000                                # an address: the check looks at no memory
    good = [(A, 1028, 1, 0), (A + 64, 2, 912, 1028), (A + 128, 1, 512, 2852)]
    per = 1028 + 1824 + 512
    assert _check(good, 9, [0], per) == 0
    assert _check(good, 9, list(range(9)), per) == 0
    assert _check(good, 9, [8, 0, 3], per) == 0
    assert _check(good, 1, [0], per) == 0
    assert _check([(A + j, 1, 1, j) for j in range(64)], 4, [1], 64) == 0
    refused = {
        "overlap": (good[:1] + [(A + 64, 2, 912, 1000)] + good[2:], 9, [0], per),
        "gap": (good[:1] + [(A + 64, 2, 912, 1030), (A + 128, 1, 512, 2854)], 9, [0], per + 2),
        "short_of_per_slot": (good, 9, [0], per + 1),
        "past_per_slot": (good, 9, [0], per - 1),
        "first_offset": ([(A, 4, 1, 1)], 9, [0], 5),
        "decreasing": ([good[1], good[0], good[2]], 9, [0], per),
        "views_65": ([(A + j, 1, 1, j) for j in range(65)], 4, [1], 65),
        "views_0": ([], 4, [1], 1),
        "outer_0": ([(A, 0, 5, 0), (A, 1, 5, 0)], 4, [1], 5),
        "inner_negative": ([(A, 5, -1, 0)], 4, [1], 5),
        "address_0": ([(0, 5, 1, 0)], 4, [1], 5),
        "product_overflow": ([(A, 2 ** 62, 4, 0)], 4, [1], 0x7fffffffffffffff),
        "slot_B": (good, 9, [9], per),
        "slot_negative": (good, 9, [-1], per),
        "slot_twice": (good, 9, [3, 5, 3], per),
        "no_slots": (good, 9, [], per),
        "more_slots_than_B": (good, 2, [0, 1, 0], per),
        "B_0": (good, 0, [0], per),
        "per_slot_0": (good, 9, [0], 0),
    }
    for name, (views, B, slots, p_) in refused.items():
        assert _check(views, B, slots, p_) == -1, name
    lib = LIB.lib()
    null = LIB._P(None)
    v = torch.tensor(good, dtype=torch.int64)
    assert lib.idv_stream_state_check(null, 3, 9, LIB._P(v.data_ptr()), 1, per) == -1
    assert lib.idv_stream_state_check(LIB._P(v.data_ptr()), 3, 9, null, 1, per) == -1
    # the device entries refuse what they can see before any launch (NULL tables: nothing could be launched)
    for name in ("idv_stream_state_gather", "idv_stream_state_scatter"):
        fn = getattr(lib, name)
        assert fn(null, 3, 9, null, 1, null, per, null) == -1
        assert fn(LIB._P(8), 65, 9, LIB._P(8), 1, LIB._P(8), per, null) == -1
        assert fn(LIB._P(8), 3, 9, LIB._P(8), 10, LIB._P(8), per, null) == -1
        assert fn(LIB._P(8), 3, 9, LIB._P(8), 1, LIB._P(8), 0, null) == -1
    assert lib.idv_stream_eps_pair_rows_as(LIB._P(8), null, LIB._P(8), 2, 2, 16, 4, LIB._P(8), LIB._P(8), null, null, null) == -1
    assert lib.idv_stream_eps_pair_rows_as(LIB._P(8), LIB._P(8), LIB._P(8), 2, 2, 16, 4, LIB._P(8), LIB._P(8), LIB._P(8), null, null) == -1


# ------------------------------------------------------------------------------------------------------- 4. the entries
def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    want = {
        "idv_stream_state_check": ("int", ["ptr", "int", "int", "ptr", "int", "long long"]),
        "idv_stream_state_gather": ("int", ["ptr", "int", "int", "ptr", "int", "ptr", "long long", "ptr"]),
        "idv_stream_state_scatter": ("int", ["ptr", "int", "int", "ptr", "int", "ptr", "long long", "ptr"]),
        "idv_stream_eps_pair_rows_as": ("int", ["ptr", "ptr", "ptr", "int", "int", "int", "int", "ptr", "ptr", "ptr", "ptr", "ptr"]),
    }
    for name, proto in want.items():
        assert name in declared and hasattr(lib, name), name
        assert protos[name] == proto, name
    # the draws entry is its sibling with one more table in front of rows; the sibling stays as it was
    old = protos["idv_stream_eps_pair_rows"][1]
    assert protos["idv_stream_eps_pair_rows_as"][1] == old[:1] + ["ptr"] + old[1:]
    assert old == ["ptr", "ptr", "int", "int", "int", "int", "ptr", "ptr", "ptr", "ptr", "ptr"]
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9                 # additive entries


def test_vae_tables_carry_the_draw_slots_behind_the_seeds():
    sp = S.SessionPlan(3, N_FFT, HOP, WIN, cap=8)
    call = sp.push([300, 0, 250], [])
    seeds = [5, 6, 7]
    flat = S.vae_session_tables(call, 2, seeds)
    assert S.vae_session_tables(call, 2, seeds, []) == flat                 # nobody moved: the copy a call made before
    assert S.vae_session_tables(call, 2, seeds, [2, 1, 0]) == flat + [2, 1, 0]
    assert flat[-3:] == seeds
