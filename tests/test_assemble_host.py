"""CPU tests of clip assembly: draw_clips, the host-side guards of dataset/assemble.py and the known answers of the
host reference tests/assemble_ref.py (the yardstick of tests/test_gpu_assemble.py); no GPU and no library load."""
import importlib
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import assemble_ref as R  # noqa: E402

ASM = importlib.import_module("i-dccrn-vae_amd.dataset.assemble")
MIX = importlib.import_module("i-dccrn-vae_amd.dataset.mix")
RV = importlib.import_module("i-dccrn-vae_amd.dataset.reverb")

LENGTHS = [70000, 64000, 500, 200000, 31000, 1, 47999]


def _host_pool(lengths, peaks=None):
    """A SignalPool that owns no device buffer: enough for every guard that runs before device work."""
    pool = MIX.SignalPool.__new__(MIX.SignalPool)
    pool.lengths = list(lengths)
    pool.offsets = [int(v) for v in np.concatenate([[0], np.cumsum(lengths)[:-1]])]
    pool.data = torch.zeros(sum(lengths))
    pool.device = pool.data.device
    if peaks is not None:
        pool._stats = {"peak": torch.tensor(peaks, dtype=torch.float64)}
    return pool


def test_draw_clips_is_a_function_of_seed_batch_and_stream():
    args = dict(seed=9, lengths=LENGTHS, batch=6, samples=64000)
    alone = ASM.draw_clips(5, **args)
    for k in range(5):
        ASM.draw_clips(k, **args)
    assert ASM.draw_clips(5, **args) == alone
    assert alone != ASM.draw_clips(4, **args) and alone != ASM.draw_clips(5, **dict(args, seed=10))
    assert alone != ASM.draw_clips(5, stream="noise", **args) and alone == ASM.draw_clips(5, stream="clean", **args)
    # the joining rule restated in the reference, from the same generator
    rng = random.Random("clips:clean:9:5")
    want = [R.join(rng, LENGTHS, list(range(len(LENGTHS))), 64000, 3200) for _ in range(6 * 4)]
    assert [alone.pieces(b, t) for b in range(6) for t in range(4)] == want
    assert alone.candidates()[2][3] == want[2 * 4 + 3] and alone.tries == 4 and len(alone.first) == len(alone.count) == 24


@pytest.mark.parametrize("samples,gap,tries", [(64000, 3200, 4), (4097, 0, 1), (800, 1, 16), (1, 3, 2), (100000, 4, 3)])
def test_pieces_are_sorted_disjoint_inside_their_members_and_fill_the_row(samples, gap, tries):
    multi = 0
    for k in range(4):
        c = ASM.draw_clips(k, 3, LENGTHS, 5, samples, tries=tries, gap=gap)
        assert ASM.check_clips(c, LENGTHS, samples) == 5
        assert all(isinstance(v, int) for f in c[:6] for v in f)
        for b in range(5):
            for t in range(tries):
                pc = c.pieces(b, t)
                assert 1 <= len(pc) <= 64
                multi += len(pc) > 1
                end = 0
                for j, (m, s, n, d) in enumerate(pc):
                    assert 0 <= s and n >= 1 and s + n <= LENGTHS[m]
                    assert d == (0 if j == 0 else end + gap)                  # end to end, exactly the gap between them
                    end = d + n
                    if LENGTHS[m] > samples - d:
                        assert n == samples - d                               # a longer recording: exactly what remains
                    else:
                        assert (s, n) == (0, LENGTHS[m])                      # a shorter one: whole
                assert end <= samples and (end == samples or len(pc) == 64 or end + gap >= samples)
    assert multi or samples == 1


def test_a_pool_of_one_sample_members_stops_at_64_pieces():
    c = ASM.draw_clips(0, 1, [1, 1, 1], 2, 1000, tries=3, gap=2)
    assert c.count == [64] * 6 and c.first == [64 * r for r in range(6)] and c.length == [1] * 384
    assert [d for d in c.dst[:64]] == [3 * j for j in range(64)] and ASM.check_clips(c, [1, 1, 1], 1000) == 2
    row = R.build_row([np.ones(1, dtype=np.float32)] * 3, c.pieces(1, 2), 1000)
    assert row.sum() == 64 and not row[190:].any()                           # the candidate ends short of the row


def test_usable_is_honoured():
    for k in range(6):
        c = ASM.draw_clips(k, 2, LENGTHS, 8, 64000, usable=[2, 4, 5])
        assert set(c.member) <= {2, 4, 5}
    seen = set()
    for k in range(6):
        seen |= set(ASM.draw_clips(k, 2, LENGTHS, 8, 64000, usable=[4, 2, 5]).member)
    assert seen == {2, 4, 5}
    assert set(ASM.draw_clips(0, 2, LENGTHS, 8, 64000, usable=[3]).member) == {3}
    pool = _host_pool([10, 20, 30], peaks=[0.5, 1.0, 0.99])
    assert pool.usable() == [0, 2] and pool.usable(1.0) == [0, 1, 2] and pool.usable(0.5) == [0] and pool.usable() == [0, 2]
    with pytest.raises(ValueError, match="no usable member"):
        pool.usable(0.25)
    for clip in (0.0, 1.5, float("nan"), "1", True):
        with pytest.raises(ValueError, match="clip"):
            pool.usable(clip)


def test_draw_batch_and_draw_reverb_are_unchanged():
    """The values the parent commit returns for a fixed (seed, k), before and after the new generator has been used."""
    def both():
        return MIX.draw_batch(5, 77, [70000, 64000, 500, 200000], [1, 16000, 480000], 3, 64000), RV.draw_reverb(5, 77, 9, 8, 0.5)
    before = both()
    ASM.draw_clips(5, 77, [70000, 64000, 500, 200000], 3, 64000)
    ASM.draw_clips(5, 77, [1, 16000, 480000], 3, 64000, stream="noise")
    assert both() == before
    d, ids = before
    assert d == MIX.Draw(clean_id=[0, 3, 0], clean_start=[3068, 26759, 1871], lens=[64000, 64000, 64000], noise_id=[2, 0, 0],
                         noise_offset=[300572, 0, 0], snr_db=[12.57686916404224, 17.535637622276354, 14.725757827397732],
                         level_db=[-35.0, -33.0, -24.0])
    assert ids == [5, 0, -1, -1, 4, 0, -1, 6]


def test_draw_clips_guards():
    ok = dict(k=0, seed=1, lengths=LENGTHS, batch=4, samples=1000)
    ASM.draw_clips(**ok)
    for kw, what in ((dict(k=-1), "k"), (dict(k=1.0), "k"), (dict(seed=True), "seed"), (dict(batch=0), "batch"), (dict(batch=65536), "batch"),
                     (dict(samples=0), "samples"), (dict(samples=(1 << 27) + 1), "samples"), (dict(tries=0), "tries"), (dict(tries=17), "tries"),
                     (dict(tries=2.0), "tries"), (dict(gap=-1), "gap"), (dict(gap=1.5), "gap"), (dict(stream=3), "stream"),
                     (dict(lengths=[]), "lengths"), (dict(lengths=[5, 0]), "lengths"), (dict(lengths=[1.5]), "lengths"), (dict(lengths="ab"), "lengths"),
                     (dict(usable=[]), "no usable member"), (dict(usable=[7]), "usable"), (dict(usable=[-1]), "usable"), (dict(usable=[0.0]), "usable"),
                     (dict(usable=3), "usable"), (dict(usable="01"), "usable")):
        with pytest.raises(ValueError, match="draw_clips: .*" + what):
            ASM.draw_clips(**dict(ok, **kw))


def test_assemble_guards_raise_before_device_work():
    lengths = [100, 50, 7]
    pool = _host_pool(lengths)
    good = ASM.Clips(member=[0, 1, 2, 1], start=[10, 0, 0, 5], length=[60, 50, 7, 45], dst=[0, 64, 114, 0], first=[0, 3], count=[3, 1], tries=2)
    assert ASM.check_clips(good, lengths, 121) == 1
    bad = [(dict(member=[0, 1, 3, 1]), "member 3"), (dict(member=[0, -1, 2, 1]), "member -1"), (dict(member=[0, 1, 2]), "equal lengths"),
           (dict(start=[10, 0, 0]), "equal lengths"), (dict(count=[3]), "equal lengths"), (dict(dst=[0, 64, 114, 0, 0]), "equal lengths"),
           (dict(member=(0, 1, 2, 1)), "python list"), (dict(start=[10, 0, 0.0, 5]), "python list"), (dict(length=[60, 50, True, 45]), "python list"),
           (dict(first=np.array([0, 3])), "python list"), (dict(tries=0), "tries"), (dict(tries=17), "tries"), (dict(tries=3), "multiple of tries"),
           (dict(start=[41, 0, 0, 5]), "piece 0: samples \\[41, 101\\)"), (dict(start=[10, 0, 0, 6]), "piece 3"), (dict(start=[-1, 0, 0, 5]), "piece 0"),
           (dict(length=[60, 0, 7, 45]), "piece 1"), (dict(length=[60, 51, 7, 45]), "piece 1"),
           (dict(dst=[0, 59, 114, 0]), "piece 1 of candidate 0 starts at 59"), (dict(dst=[50, 0, 114, 0]), "sorted by dst"),
           (dict(dst=[0, 64, 113, 0]), "do not overlap"), (dict(dst=[0, 64, 115, 0]), "covers \\[115, 122\\)"), (dict(dst=[-1, 64, 114, 0]), "before the end"),
           (dict(first=[0, 4]), "candidate 1"), (dict(first=[-1, 3]), "candidate 0"), (dict(count=[3, 2]), "candidate 1"), (dict(count=[-1, 1]), "candidate 0"),
           (dict(member=[], start=[], length=[], dst=[], first=[0, 0], count=[0, 0]), "at least one piece")]
    for kw, what in bad:
        with pytest.raises(ValueError, match="assemble: .*" + what):
            ASM.assemble(pool, good._replace(**kw), 121)
    many = ASM.Clips([0] * 65, [0] * 65, [1] * 65, list(range(65)), [0], [65], 1)
    with pytest.raises(ValueError, match="at most 64 per candidate"):
        ASM.assemble(pool, many, 121)
    rows = ASM.Clips([0] * 65536, [0] * 65536, [1] * 65536, [0] * 65536, list(range(65536)), [1] * 65536, 1)
    with pytest.raises(ValueError, match="65535"):
        ASM.assemble(pool, rows, 121)
    for kw, what in ((dict(samples=120), "covers"), (dict(samples=0), "samples"), (dict(samples=121.0), "samples"), (dict(min_activity=float("nan")), "min_activity"),
                     (dict(min_activity="0"), "min_activity"), (dict(energy_thresh=None), "energy_thresh"), (dict(target_db=float("inf")), "target_db"),
                     (dict(fs=22050), "22050"), (dict(fs=44100), "44100"), (dict(fs=0), "fs"), (dict(fs=16000.0), "fs"), (dict(clips=None), "Clips"),
                     (dict(pool=[np.zeros(4)]), "SignalPool")):
        with pytest.raises(ValueError, match="assemble: .*" + what):
            ASM.assemble(**dict(dict(pool=pool, clips=good, samples=121), **kw))
    # all value guards passed: a pool in host memory is refused before any launch
    with pytest.raises(ValueError, match="no host fallback"):
        ASM.assemble(pool, good, 121)


def test_the_window_guard_says_which_and_why():
    assert [ASM.window_of(fs) for fs in (8000, 16000, 24000, 32000, 48000)] == [400, 800, 1200, 1600, 2400]
    with pytest.raises(ValueError, match="fs = 22050: 50 ms are no whole number of samples"):
        ASM.window_of(22050)
    with pytest.raises(ValueError, match="fs = 44100: its 50 ms window of 2205 samples is no multiple of 4.*quads of 4 samples"):
        ASM.window_of(44100)
    with pytest.raises(ValueError, match="fs = 11020.*551 samples"):
        ASM.window_of(11020)


def test_activity_guards():
    x = torch.zeros(3, 2000)
    for xx, kw, what in ((x[0], {}, "\\[B, L\\]"), (x.double(), {}, "float32"), ("x", {}, "\\[B, L\\]"), (x[:0], {}, "at least one row"),
                         (x[:, :0], {}, "2\\^27"), (x, dict(lengths=[2000, 10]), "2 lengths"), (x, dict(lengths=[2001, 1, 1]), "exceeds"),
                         (x, dict(lengths=[2000, 0, 1]), "positive"), (x, dict(lengths=torch.tensor([1.0, 2.0, 3.0])), "integer"),
                         (x, dict(fs=44100), "44100"), (x, dict(energy_thresh=float("nan")), "energy_thresh"), (x, dict(target_db="a"), "target_db"),
                         (x, {}, "no host fallback"), (x, dict(lengths=[1, 799, 2000], stats=True), "no host fallback")):
        with pytest.raises(ValueError, match=what):
            ASM.activity(xx, **kw)
    with pytest.raises(ValueError, match="pool_stats: .*SignalPool"):
        ASM.pool_stats([x])


def test_dynamic_mixtures_guards():
    cp, npool = _host_pool([5000, 300], peaks=[0.5, 0.5]), _host_pool([777], peaks=[0.25])
    ok = dict(clean_pool=cp, noise_pool=npool, batch=4, samples=1600, clips=True)
    dm = MIX.DynamicMixtures(**ok)
    assert dm.usable == ([0, 1], [0]) and dm.gate == (0.6, 0.0) and (dm.tries, dm.gap, dm.fs) == (4, 3200, 16000)
    for kw, what in ((dict(clips=1), "clips"), (dict(tries=0), "tries"), (dict(tries=17), "tries"), (dict(gap=-1), "gap"), (dict(fs=44100), "44100"),
                     (dict(clean_activity=float("nan")), "clean_activity"), (dict(noise_activity="x"), "noise_activity"),
                     (dict(batch=16384), "candidate rows"), (dict(clip=0.4), "no usable member"),
                     (dict(noise_pool=_host_pool([9], peaks=[1.0])), "no usable member")):
        with pytest.raises(ValueError, match=what):
            MIX.DynamicMixtures(**dict(ok, **kw))
    # without clips none of the new keywords is looked at
    plain = MIX.DynamicMixtures(cp, npool, 4, samples=1600, tries=99, gap=-5, fs=1)
    assert plain.clips is False and not hasattr(plain, "usable")


def test_reference_known_answers():
    fs, win = 16000, R.WIN
    assert win == 800 == ASM.window_of(fs) and R.MAX_PIECES == ASM.MAX_PIECES and R.EPS == 2.0 ** -52
    z = R.activity(np.zeros(16000))
    assert (z["active"], z["windows"], z["activity"]) == (0, 20, 0.0) and z["s"].max() < 1e-25
    t = np.arange(16000)
    sine = np.sin(2 * np.pi * 1000.0 * t / fs)                           # 16 samples per period: 50 whole periods per window
    full = R.activity(sine)
    assert (full["active"], full["windows"], full["activity"]) == (20, 20, 1.0)
    # by hand: rms = sqrt(1/2), so k^2 = 2 T^2 and every window holds k^2 * 400 = 800 * 10^-2.5
    p = 1 / (1 + np.exp(1 - 0.2 * 20 * np.log10(800 * 10 ** -2.5)))
    assert abs(p - 0.6485) < 1e-4 and abs(full["s"][0] - 0.8 * p) < 1e-12 and np.abs(full["s"][1:] - p).max() < 1e-12
    # the sine in the first half only: rms = 1/2, a loud window holds 1600 * 10^-2.5, p = 0.8601.  Windows 0 .. 9 are active (s_0 =
    # 0.8 p, then p), window 10 is silent but the release keeps 0.95 p = 0.817 > 0.13, window 11 sees 0.95 * p(silence) = 0: 11 of 20
    half = np.where(t < 8000, sine, 0.0)
    h = R.activity(half)
    p = 1 / (1 + np.exp(1 - 0.2 * 20 * np.log10(1600 * 10 ** -2.5)))
    assert abs(p - 0.8601) < 1e-4 and abs(h["s"][0] - 0.8 * p) < 1e-12 and abs(h["s"][10] - 0.95 * p) < 1e-12 and h["s"][11:].max() < 1e-25
    assert (h["active"], h["windows"], h["activity"]) == (11, 20, 0.55) and h["margin"] > 0.1
    # a short last window counts as a window; one sample is one window
    assert R.activity(sine[:801])["windows"] == 2 and R.activity(sine[:800])["windows"] == 1 and R.activity(sine[3:4])["windows"] == 1
    # one sample normalised to -25 dB holds 10^-2.5: db = -50, p = 1 / (1 + e^11), never active
    one = R.activity(sine[3:4])
    assert one["active"] == 0 and abs(one["s"][0] - 0.8 / (1 + np.exp(11.0))) < 1e-15
    # choice: the first that passes; else the most active, the lowest index on a tie
    acts = [dict(activity=a / 20, active=a) for a in (3, 12, 13, 12)]
    assert R.choose(acts, 0.6) == (2, 1) and R.choose(acts, 0.55) == (1, 1) and R.choose(acts, 0.65) == (2, 0) and R.choose(acts, 0.0) == (0, 1)
    assert R.choose([dict(activity=0.5, active=10)] * 3, 0.5) == (0, 0)
    # a row built from pieces: +0 in the pauses and behind the last piece
    members = [np.arange(1, 11, dtype=np.float32), -np.arange(1, 4, dtype=np.float32)]
    row = R.build_row(members, [(0, 2, 3, 1), (1, 0, 3, 6)], 12)
    assert row.tolist() == [0, 3, 4, 5, 0, 0, -1, -2, -3, 0, 0, 0] and not np.signbit(row[[0, 4, 5, 9, 10, 11]]).any()
