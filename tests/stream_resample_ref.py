"""A float64 numpy restatement of the streaming resampler's state machine: a history of H samples, n_final, flush.

    y[n] = up * sum_j x[j] h[half + n*down - j*up],  max(0, ceil((n*down - half)/up)) <= j <= min(L - 1, floor((n*down + half)/up))

which is scipy.signal.resample_poly(x, up, down) with its default filter.  A push keeps nothing but the last H samples and the
position, so whatever it returns it has formed from those alone."""
import numpy as np


def taps(up, down):
    """scipy's default filter for a reduced ratio, float64: kaiser(5.0)-windowed sinc of 20 max(up, down) + 1 taps, sum 1."""
    m = max(up, down)
    half = 10 * m
    t = np.arange(-half, half + 1, dtype=np.float64)
    h = np.kaiser(2 * half + 1, 5.0) * np.sinc(t / m) / m
    return h / h.sum()


class RefResampler:
    def __init__(self, up, down, h=None):
        self.up, self.down = up, down
        self.half = 10 * max(up, down)
        self.H = 2 * self.half // up + 1
        self.h = taps(up, down) if h is None else np.asarray(h, dtype=np.float64)
        self.reset()

    def reset(self):
        self.n = 0
        self.hist = np.zeros(self.H)

    def n_final(self, P):
        return max(0, -((self.half - P * self.up) // self.down))

    def n_out(self, L):
        return -((-L * self.up) // self.down)

    def _outputs(self, n0, n1, x):
        up, down, half, H, P0 = self.up, self.down, self.half, self.H, self.n
        P1 = P0 + len(x)
        buf = np.concatenate([self.hist, x])                 # buf[H + d]: sample P0 + d
        y = np.zeros(n1 - n0)
        t = np.arange(2 * half // up + 1)                    # an output has at most this many terms
        for a in range(n0, n1, 1 << 15):                     # blocks of outputs, to bound the index matrices
            n = np.arange(a, min(a + (1 << 15), n1), dtype=np.int64)
            c = n * down + half
            jlo = np.maximum(0, -((2 * half - c) // up))
            jhi = np.minimum(P1 - 1, c // up)
            assert (jlo >= P0 - H).all(), "an output reads further back than the history"
            j = jlo[:, None] + t[None, :]
            ok = j <= jhi[:, None]
            j = np.where(ok, j, jlo[:, None])
            terms = np.where(ok, buf[H + j - P0] * self.h[c[:, None] - j * up], 0.0)
            y[a - n0:a - n0 + len(n)] = up * terms.sum(axis=1)
        return y

    def push(self, x):
        x = np.asarray(x, dtype=np.float64)
        n0, n1 = self.n_final(self.n), self.n_final(self.n + len(x))
        y = self._outputs(n0, n1, x)
        self.hist = np.concatenate([self.hist, x])[-self.H:]
        self.n += len(x)
        return y

    def flush(self):
        y = self._outputs(self.n_final(self.n), self.n_out(self.n), np.zeros(0))
        self.reset()
        return y


def chunkings(L, down, seed):
    """The cuts of a signal of L samples the tests use: whole, 1-sample, 37, ``down`` and random with empty pushes."""
    rng = np.random.RandomState(seed)
    rand, left = [], L
    while left:
        n = min(left, int(rng.choice([0, 0, 1, 2, 13, 37, 100, 441, 777])))
        rand.append(n)
        left -= n
    cut = lambda s: [s] * (L // s) + ([L % s] if L % s else [])
    return {"whole": [L], "one": [1] * L, "37": cut(37), "down": cut(down), "random": rand}


def run(rs, x, sizes):
    """Pushes of the given sizes, then the flush -> (whole output, samples per call)."""
    outs, pos = [], 0
    for s in sizes:
        outs.append(rs.push(x[pos:pos + s]))
        pos += s
    assert pos == len(x)
    outs.append(rs.flush())
    return np.concatenate(outs), [len(o) for o in outs]
