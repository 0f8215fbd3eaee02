"""Float64 numpy definition of clip assembly: the yardstick of tests/test_gpu_assemble.py, tests/test_assemble_host.py
and profiles/tools/measure_assemble.py.  No GPU, no package import.

It restates two pieces of the DNS-Challenge synthesizer (parity with that package is unpinned: it is not installed here):

``build_audio``, the joining rule (:func:`join`): recordings are drawn and laid end to end with ``gap`` samples of pause between them
until the clip holds ``samples`` samples; a recording longer than what remains gives a segment of exactly the remaining length, at a
drawn start.  Here a candidate also ends after 64 pieces.

``activitydetector`` (:func:`activity`), EPS = 2^-52, win = 50 ms (800 samples at 16 kHz), for a row x of n samples:

    k = 10^(target_db / 20) / (sqrt(sum x^2 / n) + EPS)                      the row normalised to target_db, pauses included
    db_j = 20 log10(k^2 sum_{window j} x^2 + EPS)                             the last window may be short
    p_j = 1 / (1 + exp(-(a + b db_j))),  a = -1, b = 0.2
    s_j = 0.8 p_j + 0.2 p_(j-1)  where p_j > p_(j-1),  else  0.05 p_j + 0.95 p_(j-1);   p_(-1) = 0
    activity = #{j: s_j > energy_thresh} / ceil(n / win)

Two deliberate differences from the synthesizer: it draws clips in a host loop until one passes ``clean_activity_threshold``; here a
bounded number of candidates (``tries``) is drawn per row and :func:`choose` takes the first whose activity exceeds ``min_activity``,
or, when none does, the one with the most active windows (the lowest index on a tie), flagged ``accepted = 0``.  And it tests every
drawn file for clipped samples; here clipped recordings (peak above ``clip``) are excluded once per pool, before anything is drawn.
"""
import numpy as np

EPS = 2.0 ** -52
WIN = 800
MAX_PIECES = 64
A, B = -1.0, 0.2
ATTACK, RELEASE = 0.8, 0.05
ENERGY_THRESH, TARGET_DB = 0.13, -25.0


def join(rng, lengths, ids, samples, gap):
    """One candidate row: ``rng`` a ``random.Random``, ``ids`` the usable members of a pool with ``lengths`` -> the list of pieces
    (member, start, length, dst)."""
    out, pos = [], 0
    while pos < samples and len(out) < MAX_PIECES:
        m = ids[rng.randrange(len(ids))]
        n, rem = lengths[m], samples - pos
        if n > rem:
            out.append((m, rng.randrange(n - rem + 1), rem, pos))
            pos += rem + gap
        else:
            out.append((m, 0, n, pos))
            pos += n + gap
    return out


def build_row(members, pieces, samples):
    """``pieces`` (member, start, length, dst) of one candidate -> the float32 row: the pieces copied, +0 elsewhere."""
    row = np.zeros(samples, dtype=np.float32)
    for m, s, n, d in pieces:
        row[d:d + n] = np.asarray(members[m], dtype=np.float32)[s:s + n]
    return row


def window_stats(x, win=WIN):
    """[ceil(n / win), 2] float64: max|x| and the sum of the squares of every window."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([[np.abs(x[s:s + win]).max(), np.sum(x[s:s + win] ** 2)] for s in range(0, len(x), win)]).reshape(-1, 2)


def activity(x, win=WIN, energy_thresh=ENERGY_THRESH, target_db=TARGET_DB):
    """One row -> dict: ``active`` (windows), ``windows``, ``activity``, ``s`` (the smoothed probabilities), ``margin`` (the least
    |s_j - energy_thresh|), ``peak``, ``sum2``, ``rms``."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    W = window_stats(x, win)
    sum2 = float(np.sum(x * x))
    k = 10.0 ** (target_db / 20.0) / (np.sqrt(sum2 / n) + EPS)
    p = 1.0 / (1.0 + np.exp(-(A + B * (20.0 * np.log10(k * k * W[:, 1] + EPS)))))
    prev = np.concatenate([[0.0], p[:-1]])
    s = np.where(p > prev, ATTACK * p + (1.0 - ATTACK) * prev, RELEASE * p + (1.0 - RELEASE) * prev)
    active = int((s > energy_thresh).sum())
    return dict(active=active, windows=len(W), activity=active / len(W), s=s, margin=float(np.abs(s - energy_thresh).min()),
                peak=float(np.abs(x).max()), sum2=sum2, rms=float(np.sqrt(sum2 / n)), window_stats=W)


def choose(acts, min_activity):
    """The results of :func:`activity` for the candidates of one row -> (chosen, accepted)."""
    for t, a in enumerate(acts):
        if a["activity"] > min_activity:
            return t, 1
    best = 0
    for t, a in enumerate(acts):
        if a["active"] > acts[best]["active"]:
            best = t
    return best, 0


def assemble(members, candidates, samples, min_activity=0.0, win=WIN, energy_thresh=ENERGY_THRESH, target_db=TARGET_DB):
    """``candidates[b][t]``: the piece list of candidate t of row b -> dict: ``rows`` float32 [B, samples], ``chosen``, ``accepted``,
    ``acts[b][t]`` (what :func:`activity` returns) and ``margin``: the least distance of any s_j from energy_thresh and of any
    activity from min_activity, the condition under which decisions are compared as integers."""
    rows, chosen, accepted, acts, margin = [], [], [], [], np.inf
    for cands in candidates:
        built = [build_row(members, pc, samples) for pc in cands]
        a = [activity(r, win, energy_thresh, target_db) for r in built]
        c, ok = choose(a, min_activity)
        margin = min([margin] + [x["margin"] for x in a] + [abs(x["activity"] - min_activity) for x in a])
        rows.append(built[c]), chosen.append(c), accepted.append(ok), acts.append(a)
    return dict(rows=np.stack(rows), chosen=chosen, accepted=accepted, acts=acts, margin=float(margin))


def pcm16(x):
    """round(0.8 * 32767 * clip(x, -1, 1)) / 32768 as float32: values a 16-bit file holds."""
    return (np.round(0.8 * 32767 * np.clip(x, -1.0, 1.0)) / 32768).astype(np.float32)


def speech_like(n, k, win=WIN):
    """A PCM16 recording whose level steps through loud, faint and silent stretches of a few windows each (+ 0.0: no negative zero)."""
    rng = np.random.default_rng(12000 + k)
    env = np.array([1.0, 1.0, 3e-3, 1.0, 0.0, 0.3])[(np.arange(n) // (2 * win) + k) % 6]
    return pcm16(rng.standard_normal(n) / 4 * env) + np.float32(0.0)
