"""Clip assembly on the MI355X (csrc/assemble.hip through dataset.assemble.assemble / activity, SignalPool.stats / usable and
DynamicMixtures(clips=True)) against the float64 host definition of tests/assemble_ref.py.  Rows of at most 12000 samples; the
references are computed once per module.  Every signal is PCM16 / 32768, so every sum of squares is an exact double whatever the order
of summation; decisions are compared as integers under the condition, asserted here from the reference alone, that every smoothed
probability stands at least 1e-9 from energy_thresh and every activity at least 1e-9 from min_activity."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import assemble_ref as R  # noqa: E402
import mix_ref  # noqa: E402
import reverb_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
MARGIN = 1e-9
SAMPLES = [1, 3, 799, 800, 801, 1601, 4097]
PIECE_LENS = [1, 2, 3, 5, 63, 64, 65, 257]
GAPS = [0, 1, 3, 4]
MIN_ACTIVITY = 0.6


def _asm():
    return importlib.import_module("i-dccrn-vae_amd.dataset.assemble")


def _mix():
    return importlib.import_module("i-dccrn-vae_amd.dataset.mix")


def _rv():
    return importlib.import_module("i-dccrn-vae_amd.dataset.reverb")


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _data(n, key, scale=1.0):
    """n PCM16 samples (no negative zero among them)."""
    return R.pcm16(np.random.default_rng(20000 + key).standard_normal(n) / 4 * scale) + np.float32(0.0)


def edge_candidates(samples):
    """Candidate rows as lists of (data, dst), chosen where the kernel can go wrong; a multiple of 4 of them."""
    out = [[(_data(samples, samples), 0)]]                                     # one piece covering the row
    for ph in range(4):                                                        # every piece length and gap, from four phases
        pos, pc, j = 0, [], ph
        while pos < samples and len(pc) < 64:
            n = min(PIECE_LENS[(3 * j + ph) % 8], samples - pos)
            pc.append((_data(n, 1000 * ph + j + samples, [1.0, 1.0, 3e-3, 0.05][(j + ph) % 4]), pos))
            pos += n + GAPS[(j + ph) % 4]
            j += 1
        out.append(pc)
    pc, pos = [], 0                                                            # 64 pieces (fewer where the row is full before)
    for j in range(64):
        n = min(1 + j % 3, samples - pos)
        if n < 1:
            break
        pc.append((_data(n, 5000 + j + samples), pos))
        pos += n + GAPS[j % 4]
    out.append(pc)
    for e in (799, 800, 801):                                                  # a piece ending one sample either side of a window edge
        e = min(e, samples)
        pc = [(_data(e, 6000 + e + samples), 0)]
        if e + 1 < samples:
            pc.append((_data(samples - e - 1, 6500 + e + samples, 0.01), e + 1))
        out.append(pc)
    pc = [(_data(min(700, samples), 7000 + samples), 0)]                       # a window wholly inside a pause
    if samples > 1700:
        pc.append((_data(samples - 1700, 7500 + samples), 1700))
    out.append(pc)
    out.append([(_data(max(1, samples // 2), 8000 + samples), 0)])             # a candidate that ends short of the row
    if samples > 3:
        out.append([(_data(samples - 3, 8500 + samples, 0.02), 3)])            # a pause in front
    while len(out) % 4:
        out.append([(_data(samples, 9000 + len(out) + samples, 10.0 ** -len(out)), 0)])
    return out


def place(cands, tries, shift=0, reverse=False):
    """Candidates as lists of (data, dst) -> (members, Clips, candidates [b][t] as the reference takes them).  Every piece is a member
    of its own with ``(i + shift) % 4`` NaN samples in front and ``(7 i) % 3`` behind, NaN members between them: the pool is NaN outside the
    named pieces and the sources fall on every residue mod 4.  ``reverse``: the members in the opposite order."""
    ASM = _asm()
    flat = [(r, j) for r, pc in enumerate(cands) for j in range(len(pc))]
    order = list(reversed(range(len(flat)))) if reverse else list(range(len(flat)))
    members, where = [], {}
    for i in order:
        r, j = flat[i]
        lead = (i + shift) % 4
        members.append(np.full(1 + (i + shift) % 2, NAN, dtype=np.float32))
        where[(r, j)] = (len(members), lead)
        members.append(np.concatenate([np.full(lead, NAN, dtype=np.float32), cands[r][j][0], np.full((7 * i) % 3, NAN, dtype=np.float32)]))
    c = ASM.Clips([], [], [], [], [], [], tries)
    for r, pc in enumerate(cands):
        c.first.append(len(c.member))
        c.count.append(len(pc))
        for j, (x, dst) in enumerate(pc):
            m, lead = where[(r, j)]
            c.member.append(m), c.start.append(lead), c.length.append(len(x)), c.dst.append(dst)
    return members, c, c.candidates()


def run(cands, tries, samples, min_activity=MIN_ACTIVITY, **kw):
    """-> (reference dict, rows, info) for one assemble call."""
    ASM, M = _asm(), _mix()
    members, clips, cc = place(cands, tries, **kw)
    pool = M.SignalPool(members)
    rows, info = ASM.assemble(pool, clips, samples, min_activity, stats=True)
    return R.assemble(members, cc, samples, min_activity), rows, info


@pytest.fixture(scope="module", params=SAMPLES)
def edge(request):
    samples = request.param
    cands = edge_candidates(samples)
    return samples, cands, {tries: run(cands, tries, samples) for tries in (1, 4)}


def test_edge_cases_are_what_they_claim():
    lens, gaps, residues = set(), set(), set()
    for samples in SAMPLES:
        cands = edge_candidates(samples)
        assert len(cands) % 4 == 0 and len(cands) >= 12
        for pc in cands:
            assert 1 <= len(pc) <= 64
            ends = [d + len(x) for x, d in pc]
            assert all(a <= b for a, (_, b) in zip(ends, pc[1:])) and ends[-1] <= samples and pc[0][1] >= 0
            lens |= {len(x) for x, _ in pc}
            gaps |= {d - e for e, (_, d) in zip(ends, pc[1:])}
        _, clips, _ = place(cands, 4)
        residues |= {s % 4 for s in clips.start}
    assert lens >= set(PIECE_LENS) and gaps >= set(GAPS) and residues == {0, 1, 2, 3}
    c = edge_candidates(4097)
    assert any(len(pc) == 64 for pc in c) and any(len(pc) == 1 and len(pc[0][0]) == 4097 for pc in c)
    assert {pc[0][1] + len(pc[0][0]) for pc in c[6:9]} == {799, 800, 801}
    assert c[9][0][1] + len(c[9][0][0]) <= 800 and c[9][1][1] >= 1600                           # window 1 lies in the pause
    assert any(pc[-1][1] + len(pc[-1][0]) < 4097 for pc in c)


def test_statistics_and_rows_are_bit_exact(edge):
    """1. of the issue: max|x| and sum x^2 of every window and every written row equal the reference bit for bit; the pool holds NaN
    everywhere outside the named pieces and no output holds one."""
    samples, cands, got = edge
    for tries, (ref, rows, info) in got.items():
        B = len(cands) // tries
        nw = -(-samples // R.WIN)
        assert rows.shape == (B, samples) and rows.dtype == torch.float32 and info["window_stats"].shape == (B, tries, nw, 2)
        for t in (rows, info["window_stats"], info["activity"], info["peak"], info["sum2"]):
            assert torch.isfinite(t).all(), (samples, tries)
        assert np.array_equal(_bits(rows), _bits(ref["rows"])), (samples, tries)
        W = info["window_stats"].cpu().numpy()
        for b in range(B):
            for t in range(tries):
                a = ref["acts"][b][t]
                assert np.array_equal(_bits(W[b, t]), _bits(a["window_stats"])), (samples, tries, b, t)
                assert float(info["peak"][b, t]) == a["peak"] and float(info["sum2"][b, t]) == a["sum2"]


def test_decisions_equal_the_reference(edge):
    """2. of the issue: active-window counts, chosen and accepted as integers, under the margins asserted first."""
    samples, cands, got = edge
    for tries, (ref, rows, info) in got.items():
        assert ref["margin"] >= MARGIN, (samples, tries, ref["margin"])
        B = len(cands) // tries
        assert info["chosen"].dtype == info["accepted"].dtype == info["active"].dtype == info["windows"].dtype == torch.int32
        assert info["activity"].dtype == torch.float64 and info["activity"].shape == (B, tries)
        assert info["active"].tolist() == [[a["active"] for a in row] for row in ref["acts"]], (samples, tries)
        assert info["windows"].tolist() == [[a["windows"] for a in row] for row in ref["acts"]]
        assert info["activity"].tolist() == [[a["activity"] for a in row] for row in ref["acts"]]
        assert info["chosen"].tolist() == ref["chosen"] and info["accepted"].tolist() == ref["accepted"], (samples, tries)
    if samples == 4097:
        acc = got[1][0]["accepted"]
        assert 0 < sum(acc) < len(acc)                                          # candidates on both sides of the gate


@pytest.fixture(scope="module")
def big():
    """65 rows of 4 candidates of 4097 samples: the edge candidates, turned by one from row to row."""
    cands = edge_candidates(4097)
    rows = [[cands[(b + 5 * t) % len(cands)] for t in range(4)] for b in range(65)]
    flat = [c for row in rows for c in row]
    return rows, run(flat, 4, 4097)


def test_rows_do_not_depend_on_the_batch(big):
    """3. of the issue: row b of a batch of 65 against the same candidate list assembled alone (B = 1), in a batch of 3, and with the
    pieces elsewhere in the pool (another order of the members, other alignments): every output bit for bit."""
    rows, (ref, out, info) = big
    assert ref["margin"] >= MARGIN and out.shape == (65, 4097)
    assert np.array_equal(_bits(out), _bits(ref["rows"])) and info["chosen"].tolist() == ref["chosen"]
    keys = ("activity", "active", "windows", "peak", "sum2", "window_stats", "chosen", "accepted")

    def same(b0, b1, **kw):
        _, o, i = run([c for row in rows[b0:b1] for c in row], 4, 4097, **kw)
        assert np.array_equal(_bits(o), _bits(out[b0:b1])), (b0, b1, kw)
        for k in keys:
            assert np.array_equal(_bits(i[k]), _bits(info[k][b0:b1])), (b0, b1, kw, k)

    for b in (0, 7, 64):
        same(b, b + 1)
    same(30, 33)
    same(62, 65, shift=1, reverse=True)
    same(0, 65, shift=3, reverse=True)


def _loud_for(windows, key):
    """One piece that covers the first ``windows`` windows of a row; the release keeps one more window active."""
    return [(_data(800 * windows, 30000 + key), 0)]


def test_choice():
    """4. of the issue, rows of 5 windows: a loud piece over w windows gives w + 1 active ones."""
    cases = {"candidate 0 fails and 2 passes": ([1, 2, 3, 4], 0.7, 2, 1),
             "all fail: the most active wins": ([1, 1, 2, 1], 0.7, 2, 0),
             "a tie goes to the lowest index": ([1, 2, 2, 1], 0.7, 1, 0)}
    cands = [_loud_for(w, 10 * r + t) for r, (ws, _, _, _) in enumerate(cases.values()) for t, w in enumerate(ws)]
    ref, rows, info = run(cands, 4, 4000, 0.7)
    assert ref["margin"] >= MARGIN
    assert [[a["active"] for a in row] for row in ref["acts"]] == [[w + 1 for w in ws] for ws, _, _, _ in cases.values()]
    assert info["active"].tolist() == [[w + 1 for w in ws] for ws, _, _, _ in cases.values()]
    assert info["chosen"].tolist() == ref["chosen"] == [c for _, _, c, _ in cases.values()]
    assert info["accepted"].tolist() == ref["accepted"] == [a for _, _, _, a in cases.values()]
    assert np.array_equal(_bits(rows), _bits(ref["rows"]))
    # tries = 1: the one candidate is taken whatever its activity
    ref, rows, info = run(cands[:3], 1, 4000, 0.7)
    assert info["chosen"].tolist() == [0, 0, 0] and info["accepted"].tolist() == ref["accepted"] == [0, 0, 1]


def test_activity_of_a_padded_batch():
    """5. of the issue: every row judged over its own length, NaN behind it, at an odd row pitch."""
    ASM = _asm()
    lens = [1, 799, 800, 801, 12000]
    rows = [R.speech_like(n, k) for k, n in enumerate(lens)]
    want = [R.activity(r) for r in rows]
    assert min(a["margin"] for a in want) >= MARGIN
    x = torch.full((5, 12003), NAN)
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(r)
    x = x.cuda()[:, :12000]
    act, active, windows = ASM.activity(x, lengths=lens, stats=True)
    assert act.dtype == torch.float64 and act.is_cuda and active.dtype == windows.dtype == torch.int32
    assert active.tolist() == [a["active"] for a in want] and windows.tolist() == [1, 1, 1, 2, 15]
    assert act.tolist() == [a["activity"] for a in want] and 0 < want[4]["active"] < 15
    assert np.array_equal(_bits(ASM.activity(x, lengths=lens)), _bits(act))
    for b, n in enumerate(lens):                                               # a row alone, and whole rows without lengths
        one = ASM.activity(x[b:b + 1, :n].contiguous())
        assert np.array_equal(_bits(one), _bits(act[b:b + 1])), n
    full = ASM.activity(torch.from_numpy(np.stack([rows[4], R.speech_like(12000, 9)])).cuda())
    assert full.tolist() == [want[4]["activity"], R.activity(R.speech_like(12000, 9))["activity"]]


def test_pool_statistics_and_usable():
    """6. of the issue: peaks bit for bit, a member with one sample of 1.0 excluded at clip = 0.99."""
    M = _mix()
    members = [R.speech_like(n, 40 + k) for k, n in enumerate((1601, 5, 12000, 800, 3333))]
    members[2] = members[2].copy()
    members[2][7777] = 1.0
    members.append(np.full(64, np.float32(32440 / 32768)))                       # 0.98999: the loudest usable
    pool = M.SignalPool(members)
    st = pool.stats()
    want = [R.activity(m) for m in members]
    assert min(a["margin"] for a in want) >= MARGIN
    assert st is pool.stats() and all(st[k].dtype == torch.float64 and st[k].is_cuda and st[k].shape == (6,) for k in ("peak", "rms", "activity"))
    assert np.array_equal(_bits(st["peak"]), _bits(np.array([a["peak"] for a in want])))
    assert st["activity"].tolist() == [a["activity"] for a in want]
    assert np.allclose(st["rms"].cpu().numpy(), [a["rms"] for a in want], rtol=4 * 2.0 ** -53, atol=0)       # an exact sum, a division, a root
    assert st["peak"][2].item() == 1.0 and pool.usable() == [0, 1, 3, 4, 5] == pool.usable(0.99) and pool.usable(1.0) == list(range(6))
    assert 5 not in pool.usable(0.98)


@pytest.fixture(scope="module")
def pools():
    RV, M = _rv(), _mix()
    clean = [R.speech_like(n, 60 + k) for k, n in enumerate((1900, 701, 5000, 1234, 2600, 333))]
    clean[3] = clean[3].copy()
    clean[3][100] = -1.0                                                        # a clipped recording: never drawn
    noise = [_data(n, 70 + k, 0.3) for k, n in enumerate((4800, 257, 9001))]
    rirs = [reverb_ref.rir_row(K, 80 + k) for k, K in enumerate((300, 17))]
    return clean, noise, rirs, M.SignalPool(clean), M.SignalPool(noise), RV.RirPool(rirs)


def test_dynamic_mixtures_with_clips(pools):
    """7. of the issue.  Every step against its float64 definition at the tolerance its own tests use: the assembled rows bit for bit;
    the reverberant rows within ulp32 + 2 K 2^-53 S (tests/test_gpu_reverb.py); the mixture of the device's float32 input rows within
    4 n 2^-53 relative in the gains and one float32 ulp in the outputs (tests/test_gpu_mix.py)."""
    ASM, RV, M = _asm(), _rv(), _mix()
    clean, noise, rirs, cp, npool, rp = pools
    B, n, seed = 4, 4096, 21
    kw = dict(samples=n, seed=seed, tries=3, gap=100, clean_activity=0.6, noise_activity=0.0)
    dry = M.DynamicMixtures(cp, npool, B, clips=True, **kw)
    wet = M.DynamicMixtures(cp, npool, B, clips=True, rir_pool=rp, p_reverb=0.5, **kw)
    early = M.DynamicMixtures(cp, npool, B, clips=True, rir_pool=rp, p_reverb=0.5, target="early", early_ms=1.0, **kw)
    assert dry.usable == ([0, 1, 2, 4, 5], [0, 1, 2])
    gain_tol = 4 * n * 2.0 ** -53
    seen, short, joined = set(), 0, 0
    for k in (0, 1, 2):
        d = dry.draw(k)
        got = dry.batch(k, info=True)
        inf = got[3]
        assert inf["clean_clips"] == ASM.draw_clips(k, seed, cp.lengths, B, n, 3, 100, dry.usable[0], "clean")
        assert inf["noise_clips"] == ASM.draw_clips(k, seed, npool.lengths, B, n, 3, 100, dry.usable[1], "noise")
        assert 3 not in inf["clean_clips"].member
        rc = R.assemble(clean, inf["clean_clips"].candidates(), n, 0.6)
        rn = R.assemble(noise, inf["noise_clips"].candidates(), n, 0.0)
        assert rc["margin"] >= MARGIN and rn["margin"] >= MARGIN
        assert inf["clean_chosen"].tolist() == rc["chosen"] and inf["clean_accepted"].tolist() == rc["accepted"]
        assert inf["noise_chosen"].tolist() == rn["chosen"] and inf["noise_accepted"].tolist() == rn["accepted"] == [1] * B
        rows_c, _ = ASM.assemble(cp, inf["clean_clips"], n, 0.6)
        rows_n, _ = ASM.assemble(npool, inf["noise_clips"], n, 0.0)
        assert np.array_equal(_bits(rows_c), _bits(rc["rows"])) and np.array_equal(_bits(rows_n), _bits(rn["rows"]))

        def check_mix(out, clean_in, tag):
            sig = [t.cpu().numpy() for t in out[:3]]
            for b in range(B):
                r = mix_ref.mix(clean_in[b], rn["rows"][b], 0, d.snr_db[b], d.level_db[b])
                for key in ("g_clean", "g_noise"):
                    assert abs(float(out[3][key][b]) - r[key]) <= gain_tol * abs(r[key]), (tag, k, b, key)
                for s, key in enumerate(("noisy", "clean_out", "noise_out")):
                    err = np.abs(sig[s][b].astype(np.float64) - r[key].astype(np.float64))
                    assert (err <= np.maximum(mix_ref.ulp32(sig[s][b]), mix_ref.ulp32(r[key]))).all(), (tag, k, b, key)

        check_mix(got, rc["rows"], "dry")
        for b in range(B):                                                     # no zero tail unless the candidate ended short
            pc = inf["clean_clips"].pieces(b, rc["chosen"][b])
            end = pc[-1][3] + pc[-1][2]
            short += end < n
            joined += len(pc) > 1
            assert got[1][b, pc[-1][3]:end].any() and not got[1][b, end:].any()
        # with a RirPool: the rows draw_reverb names are convolved whole, the others are the dry feed's
        w = wet.batch(k, info=True)
        ids = RV.draw_reverb(k, seed, len(rp), B, 0.5)
        assert w[3]["rir_id"] == ids and w[3]["clean_clips"] == inf["clean_clips"]
        seen |= {r >= 0 for r in ids}
        conv = RV.reverb_rows(rows_c, rp, ids)
        for b, r in enumerate(ids):
            if r < 0:
                assert np.array_equal(_bits(conv[b]), _bits(rows_c[b] + 0.0))
                continue
            ref, S = reverb_ref.reverb(rc["rows"][b], rirs[r])
            y = conv[b].cpu().numpy()
            assert (np.abs(y.astype(np.float64) - ref) <= reverb_ref.bound(len(rirs[r]), S, y, ref)).all(), (k, b)
        check_mix(w, conv.cpu().numpy(), "wet")
        direct = M.snr_mix(conv, rows_n, d.snr_db, d.level_db)
        for s in range(3):
            assert np.array_equal(_bits(w[s]), _bits(direct[s])), (k, s)
        # target="early": float32(g_clean x the row under the early taps), mixture and noise unchanged
        e = early.batch(k, info=True)
        few = RV.reverb_rows(rows_c, rp, ids, taps=rp.early_taps(1.0))
        exp = (e[3]["g_clean"].cpu().numpy()[:, None] * few.cpu().numpy().astype(np.float64)).astype(np.float32)
        assert np.array_equal(_bits(e[1]), _bits(exp)) and np.array_equal(_bits(e[0]), _bits(w[0])) and np.array_equal(_bits(e[2]), _bits(w[2]))
        assert len(dry.batch(k)) == 3 and all(t.shape == (B, n) and t.dtype == torch.float32 and t.is_cuda for t in got[:3])
    assert seen == {True, False} and joined >= 6 and short < 3 * B
    # batch 2 drawn first equals batch 2 drawn after 0 and 1
    fresh = M.DynamicMixtures(cp, npool, B, clips=True, **kw).batch(2)
    for s in range(3):
        assert np.array_equal(_bits(fresh[s]), _bits(got[s]))


def test_without_clips_nothing_changes(pools):
    M = _mix()
    clean, noise, _, _, _, _ = pools
    cp, npool = M.SignalPool(clean), M.SignalPool(noise)
    for kw in ({}, dict(clips=False, tries=2, gap=7, clean_activity=0.9)):
        dm = M.DynamicMixtures(cp, npool, 4, samples=4096, seed=11, **kw)
        got = dm.batch(1, info=True)
        want = M.mix_draw(cp, npool, M.draw_batch(1, 11, cp.lengths, npool.lengths, 4, 4096), 4096)
        for s in range(3):
            assert np.array_equal(_bits(got[s]), _bits(want[s]))
        assert set(got[3]) == set(want[3])
    assert "_stats" not in cp.__dict__ and "_stats" not in npool.__dict__       # the feed without clips never asks for pool statistics


def test_mix_draw_takes_noise_rows(pools):
    """mix_draw(noise=): row b of the tensor, read from offset 0 with length ``samples``, in place of the noise the draw names."""
    M = _mix()
    _, _, _, cp, npool, _ = pools
    n = 1500
    d = M.draw_batch(0, 3, cp.lengths, npool.lengths, 5, n)
    nz = torch.from_numpy(np.stack([_data(n, 90 + b, 0.2) for b in range(5)])).cuda()
    got = M.mix_draw(cp, npool, d, n, noise=nz)
    rows = torch.zeros(5, n)
    for b, (c, s, m) in enumerate(zip(d.clean_id, d.clean_start, d.lens)):
        rows[b, :m] = cp.member(c)[s:s + m].cpu()
    want = M.snr_mix(rows.cuda(), nz, d.snr_db, d.level_db, lengths=d.lens)
    both = M.mix_draw(cp, npool, d, n, clean=rows.cuda(), noise=nz)
    for s in range(3):
        assert np.array_equal(_bits(got[s]), _bits(want[s])) and np.array_equal(_bits(both[s]), _bits(want[s]))
    for bad, what in ((nz[:4], "\\[5, 1500\\]"), (nz[:, :-1], "\\[5, 1500\\]"), (nz.double(), "float32"), (nz[0], "\\[B, L\\]")):
        with pytest.raises(ValueError, match=what):
            M.mix_draw(cp, npool, d, n, noise=bad)
