"""tests/rows_ref.py, the numpy restatement of the summation order of csrc/rows.hpp, against math.fsum (no GPU).  It is the yardstick
of tests/test_gpu_rows_order.py, so it is held to what any correct order of double additions must give."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rows_ref as RR  # noqa: E402

LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1027, 2400]


def _float_row(n, key):
    return (0.1 * np.random.default_rng(100 + key).standard_normal(n)).astype(np.float32)


def _pcm16_row(n, key):
    return (np.random.default_rng(200 + key).integers(-32768, 32768, n) / 32768.0).astype(np.float32)


def _row_total(x, win):
    return RR.row_sum([RR.window_sum_sq(x[k:k + win]) for k in range(0, len(x), win)])


def test_emulator_equals_fsum_within_n_ulps():
    """A sum of n non-negative doubles in any order errs by at most (n - 1) 2^-53 relative; the squares themselves are exact."""
    for key, n in enumerate(LENGTHS):
        x = _float_row(n, key)
        want = math.fsum(float(v) * float(v) for v in x)
        for win in (4, 256, 1024):
            got = float(_row_total(x, win))
            assert abs(got - want) <= n * 2.0 ** -53 * want, (n, win, got, want)
        got = float(RR.window_sum_sq(x))
        assert abs(got - want) <= n * 2.0 ** -53 * want, (n, got, want)


def test_emulator_is_exact_on_pcm16_rows():
    """Samples k / 32768: every partial sum is an integer below 2^53 times 2^-30, so every order gives the same double."""
    for key, n in enumerate(LENGTHS):
        x = _pcm16_row(n, key)
        want = math.fsum(float(v) * float(v) for v in x)
        assert float(RR.window_sum_sq(x)) == want
        for win in (4, 1024):
            assert float(_row_total(x, win)) == want, (n, win)


def test_the_order_is_the_documented_one():
    """Where the order shows: 2^54 (ulp 4) and three ones.  Lane 0 holds quad 0 and adds it in increasing i: behind the big term
    every 1 is rounded away, in front of it the ones add up to 3 first and round up to 4.  Quad 64 (sample 256 on) belongs to lane 0
    again; quad 1 belongs to lane 1, whose 3 meets lane 0 whole in the butterfly."""
    big = np.float32(2.0 ** 27)
    b2 = 2.0 ** 54
    x = np.array([big, 1, 1, 1], dtype=np.float32)
    assert float(RR.window_sum_sq(x)) == b2
    assert float(RR.window_sum_sq(x[::-1].copy())) == b2 + 4.0
    y = np.zeros(260, dtype=np.float32)
    y[0], y[256:259] = big, 1.0
    assert float(RR.window_sum_sq(y)) == b2
    y[256:259], y[4:7] = 0.0, 1.0
    assert float(RR.window_sum_sq(y)) == b2 + 4.0


def test_tree_and_row_sum():
    v = np.arange(256, dtype=np.float64)
    assert RR.tree256(v) == v.sum() and RR.tree256(v, np.maximum) == 255 and RR.tree256(-v, np.minimum) == -255
    assert RR.tree256(np.arange(256, dtype=np.int32), np.minimum) == 0
    # thread 0 adds windows 0, 256, 512 in this order before the tree: (2^53 + 1) + 1 loses both ones
    w = np.zeros(600)
    w[0], w[256], w[512] = 2.0 ** 53, 1.0, 1.0
    assert RR.row_sum(w) == 2.0 ** 53
    w[0], w[512] = 1.0, 2.0 ** 53
    assert RR.row_sum(w) == 2.0 ** 53 + 2.0
    assert RR.row_sum([]) == 0.0 and RR.row_sum([3.0]) == 3.0
