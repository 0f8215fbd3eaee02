"""The fixed order of summation of the row-signal kernels (csrc/rows.hpp), restated in numpy float64 and nothing else.

A row is cut into windows; sample i of a window belongs to quad i // 4, quad q to lane q % 64; a lane adds its quads in increasing q,
the four terms of a quad in increasing i; the 64 lanes meet in an xor butterfly; a row adds its windows k = t, t + 256, ... in thread
t, and the 256 threads meet in a tree.  Every step below is one IEEE double addition, as on the device.

What can be pinned bit for bit this way are sums of squares of float32 INPUT samples: the square of a float32 is exact in double, so
whether the compiler contracts ``s += d * d`` into an fma or not does not change a bit.  Maxima are exact in any order.  A sum such as
sum y0^2 of the mixer, whose squares are rounded (or not, under an fma), is outside this module's reach.
"""
import numpy as np

LANES = 64
THREADS = 256


def butterfly(v, op=np.add):
    """The 64 lanes' values after v = op(v, v[lane ^ o]) for o = 32 .. 1; every lane ends with the same value."""
    v = np.asarray(v, dtype=np.float64).copy()
    idx = np.arange(LANES)
    o = LANES // 2
    while o:
        v = op(v, v[idx ^ o])
        o //= 2
    return v


def window_sum_sq(x) -> np.float64:
    """The sum of the squares of the float32 samples of one window in the device's order.  A sample that does not exist (the ragged
    last quad, a lane without a quad in the last round) enters as +0, which leaves a non-negative partial as it is."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    sq = np.zeros(-(-max(len(x), 1) // (4 * LANES)) * 4 * LANES, dtype=np.float64)
    sq[:len(x)] = x.astype(np.float64) ** 2                 # exact
    lanes = np.zeros(LANES, dtype=np.float64)
    for quads in sq.reshape(-1, LANES, 4):                   # round r: quad q = 64 r + lane
        for i in range(4):
            lanes = lanes + quads[:, i]
    return butterfly(lanes)[0]


def tree256(values, op=np.add):
    """The 256 threads' values folded as sh[t] = op(sh[t], sh[t + o]) for t < o, o = 128 .. 1 -> sh[0]."""
    v = np.array(values).copy()
    assert v.shape == (THREADS,)
    o = THREADS // 2
    while o:
        v[:o] = op(v[:o], v[o:2 * o])
        o //= 2
    return v[0]


def row_sum(window_values) -> np.float64:
    """A row's sum of its windows' values: thread t adds the windows k = t, t + 256, ... in this order from +0, then the tree."""
    w = np.asarray(window_values, dtype=np.float64)
    acc = np.zeros(THREADS, dtype=np.float64)
    for k0 in range(0, len(w), THREADS):
        part = w[k0:k0 + THREADS]
        acc[:len(part)] = acc[:len(part)] + part
    return tree256(acc)
