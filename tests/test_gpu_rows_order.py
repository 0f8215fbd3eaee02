"""The order of summation of the row-signal kernels on the MI355X (csrc/rows.hpp through ops.mix_gains, ops.asm_activity and
ops.trim_bounds) against its numpy restatement tests/rows_ref.py: every assertion is bit equality.  Seeded float32 0.1 N(0, 1) rows,
whose sums of squares depend on the order (PCM16 rows would not); lengths around the quad, the lane's second quad (sample 257 on) and
the ragged last quad of a second window, and one row whose 600 windows make a thread add several before the tree."""
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

import rows_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1027]
SHAPES = [(LENGTHS, 1024), ([2400], 4)]                           # (row lengths, win)
NAN = float("nan")


def _ops():
    return importlib.import_module("i-dccrn-vae_amd.ops")


def _row(n, key):
    return (0.1 * np.random.default_rng(4000 + key).standard_normal(n)).astype(np.float32)


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    return a.view(np.int64)


def _padded(rows):
    """The rows in one NaN-padded batch at the pitch of the longest: an odd pitch puts the rows at every alignment."""
    x = torch.full((len(rows), max(len(r) for r in rows)), NAN)
    for b, r in enumerate(rows):
        x[b, :len(r)] = torch.from_numpy(r)
    return x.cuda()


@pytest.fixture(scope="module")
def expected():
    """Per shape: the rows and, from the emulator, (max|x|, sum x^2) per window and per row."""
    out = []
    for s, (lens, win) in enumerate(SHAPES):
        sets = []
        for base in (0, 100):                                     # 0: clean / the assembled rows, 100: noise
            rows = [_row(n, base + 10 * s + b) for b, n in enumerate(lens)]
            wins = [np.array([[np.abs(r[k:k + win]).max(), RR.window_sum_sq(r[k:k + win])] for k in range(0, len(r), win)],
                             dtype=np.float64) for r in rows]
            tot = np.array([[w[:, 0].max(), RR.row_sum(w[:, 1])] for w in wins], dtype=np.float64)
            sets.append((rows, wins, tot))
        out.append((lens, win, sets))
    return out


def test_mix_gains_statistics(expected):
    """W[b][k] = max|c|, sum c^2, max|v|, sum v^2 of every window and sum_c2, max_c, sum_v2, max_v of every row."""
    ops = _ops()
    F = ops.MIX_FIELD
    for lens, win, ((c, cw, ct), (v, vw, vt)) in expected:
        B, L = len(lens), max(lens)
        table = torch.tensor([lens, lens, [0] * B], dtype=torch.int32).cuda()
        rows = ops.MixRows(_padded(c), None, _padded(v), None, table, B, L, L)
        par = torch.tensor([[5.0, -25.0]] * B, dtype=torch.float64).cuda()
        rec, W = ops.mix_gains(rows, par, False, -25.0, 0.99, win, -50.0)
        rec, W = rec.cpu().numpy(), W.cpu().numpy()
        assert W.shape == (B, -(-L // win), ops.MIX_WIN_FIELDS)
        for b in range(B):
            nw = len(cw[b])
            assert np.array_equal(_bits(W[b, :nw, 0:2]), _bits(cw[b])), (lens[b], win, "clean windows")
            assert np.array_equal(_bits(W[b, :nw, 2:4]), _bits(vw[b])), (lens[b], win, "noise windows")
            got = [rec[b, F[k]] for k in ("max_c", "sum_c2", "max_v", "sum_v2")]
            assert np.array_equal(_bits(got), _bits(np.concatenate([ct[b], vt[b]]))), (lens[b], win, got, ct[b], vt[b])


def test_asm_activity_statistics(expected):
    """window_stats and rowstat of single-piece rows read in place from a pool, the rows 0, 1, 2, 3 floats past a 16-byte boundary."""
    ops = _ops()
    for lens, win, ((x, xw, xt), _) in expected:
        parts, src, pos = [], [], 0
        for b, r in enumerate(x):
            lead = (b % 4 - pos) % 4
            parts += [np.full(lead, NAN, dtype=np.float32), r]
            src.append(pos + lead)
            pos += lead + len(r)
        pool = torch.from_numpy(np.concatenate(parts)).cuda()
        R = len(lens)
        assert pool.data_ptr() % 16 == 0 and [s % 4 for s in src] == [b % 4 for b in range(R)]
        tab = ops.asm_tables(pool, src, lens, [0] * R, list(range(R)), [1] * R, R, 1, max(lens))
        a = ops.asm_activity(tab, tab.len, win, -25.0, 0.13, 0.0)
        W, rowstat = a["window_stats"].cpu().numpy(), a["rowstat"].cpu().numpy()
        assert W.shape == (R, -(-max(lens) // win), ops.ASM_WIN_FIELDS)
        for b in range(R):
            assert np.array_equal(_bits(W[b, :len(xw[b])]), _bits(xw[b])), (lens[b], win, "windows")
            assert np.array_equal(_bits(rowstat[b]), _bits(xt[b])), (lens[b], win, rowstat[b], xt[b])


@pytest.mark.parametrize("hop,frame", [(4, 8), (256, 512)])
def test_trim_frame_powers(expected, hop, frame):
    """power[b][t] = (E[t - r/2] + ... + E[t + r/2 - 1]) / frame, added in increasing block index from +0 over the blocks inside the
    row, E[k] the block's sum of squares in the order of a window; zeros from frame 1 + n // hop on."""
    ops = _ops()
    lens, _, ((x, _, _), _) = expected[0]
    _, P = ops.trim_bounds(_padded(x), 30.0, frame, hop, ops.Lengths(lens, "cuda"), power=True)
    P = P.cpu().numpy()
    assert P.shape == (len(lens), 1 + max(lens) // hop) and P.dtype == np.float64
    r = frame // hop
    for b, n in enumerate(lens):
        E = [RR.window_sum_sq(x[b][k:k + hop]) for k in range(0, n, hop)]
        want = np.zeros(P.shape[1])
        for t in range(1 + n // hop):
            s = np.float64(0.0)
            for k in range(max(t - r // 2, 0), min(t - r // 2 + r, len(E))):
                s = s + E[k]
            want[t] = s / np.float64(frame)
        assert np.array_equal(_bits(P[b]), _bits(want)), (n, hop, frame)
