"""Float64 numpy definition of silence trimming: the yardstick of tests/test_gpu_trim.py and of
profiles/tools/measure_trim.py.  No GPU, no package import.

It restates ``librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length)`` of librosa 0.10 for one row of n >= 1 samples:

  frames      the row padded by frame_length // 2 zeros on both sides (``rms(center=True, pad_mode="constant")``); frame t covers
              padded samples [t hop, t hop + frame_length); T = 1 + n // hop of them
  frame_power P[t] = mean of the squares over frame t
  frame_db    db[t] = 10 log10(max(1e-10, P[t])) - 10 log10(max(1e-10, max_t P[t]))        (``amplitude_to_db`` with amin = 1e-5 on the
              rms).  The package differs in two ways that this float64 restatement leaves open: ``feature.rms`` forms the squares and
              their mean in float32 by default (P about 1e-7 relative, some 5e-7 dB, away from the float64 P), and it takes the
              square root of P and squares it again
  trim        t0 / t1 the first / last frame with db[t] > -top_db:  (t0 hop, min(n, (t1 + 1) hop)); no such frame: (0, 0)

So a row of zeros, or one wholly below 1e-10 in power, has db = 0 everywhere and is returned untrimmed as (0, n).
"""
import numpy as np

FRAME, HOP, AMIN_POWER = 2048, 512, 1e-10

# the lengths of the GPU tests: every block and frame edge of (2048, 512) and the first lengths past one, two and four frames
LENGTHS = [1, 2, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 12000, 16000, 16385]


def n_frames(n, hop=HOP):
    return 1 + n // hop


def frame_power(y, frame=FRAME, hop=HOP):
    y = np.asarray(y, dtype=np.float64)
    yp = np.pad(y, frame // 2)
    return np.array([np.mean(yp[t * hop:t * hop + frame] ** 2) for t in range(n_frames(len(y), hop))])


def frame_db(y, frame=FRAME, hop=HOP):
    P = frame_power(y, frame, hop)
    return 10.0 * np.log10(np.maximum(AMIN_POWER, P)) - 10.0 * np.log10(np.maximum(AMIN_POWER, P.max()))


def trim(y, top_db=30.0, frame=FRAME, hop=HOP):
    """-> (start, end) of the non-silent span of one row."""
    nz = np.flatnonzero(frame_db(y, frame, hop) > -top_db)
    if nz.size == 0:
        return 0, 0
    return int(nz[0] * hop), min(len(y), int((nz[-1] + 1) * hop))


def margin_db(y, top_db, frame=FRAME, hop=HOP):
    """The distance in dB of the frame nearest to the threshold: a comparison in another double log10 can only differ below it."""
    return float(np.abs(frame_db(y, frame, hop) + top_db).min())


def fade(n, seed):
    """PCM16 noise (values k / 32768 as float32) under an envelope that rises 70 dB over the first 40 % of the row and falls 70 dB
    over its last 30 %."""
    r = np.random.default_rng(1000 + seed)
    t = np.arange(n) / max(n, 1)
    env_db = np.minimum(0, np.minimum((t - 0.4) / 0.4 * 70, (0.7 - t) / 0.3 * 70))
    x = 0.25 * r.standard_normal(n) * 10 ** (env_db / 20)
    return (np.round(x * 32768).clip(-32768, 32767) / 32768).astype(np.float32)


def cases(seeds=None):
    """One fade() row per entry of LENGTHS, seed = the entry's index unless ``seeds`` names another one for it."""
    seeds = seeds or {}
    return [fade(n, seeds.get(k, k)) for k, n in enumerate(LENGTHS)]
