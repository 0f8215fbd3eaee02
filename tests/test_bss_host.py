"""CPU tests of the BSS-eval SDR / SIR / SAR metric with two sources: the host reference tests/bss_ref.py (it is the yardstick of
tests/test_gpu_bss.py, so its cases must be ones for which the float64 definition itself is unambiguous) and the host-side guards of
inference.compute_bss / score_list; no GPU needed."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bss_ref as R  # noqa: E402
import sdr_ref as S  # noqa: E402

INF = importlib.import_module("i-dccrn-vae_amd.inference")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")


@pytest.fixture(scope="module")
def table():
    """Both float64 solvers on every case, once."""
    out = []
    for index, (L, K, kind) in enumerate(R.CASES):
        s, v, y = R.case_signals(index)
        out.append(dict(L=L, K=K, s=s, v=v, y=y, lu=R.bss(s, v, y, K), lev=R.bss(s, v, y, K, solver="levinson")))
    return out


def test_cases_name_the_shapes_of_the_issue():
    want = {16: [24, 31, 32, 33, 257], 64: [96, 127, 128, 129, 257, 4001], 512: [768, 1023, 1024, 1025, 4082, 16385]}
    got = {}
    for L, K, kind in R.CASES:
        assert kind in ("white", "lowpass") and L >= 1.5 * K
        got.setdefault(K, []).append(L)
    assert got == want
    assert {R.case_snr(k) for k in range(len(R.CASES))} == {0, 20, 60}                                   # the artifacts are never left out
    assert {R.GAINS[R.case_snr(k)] for k in range(len(R.CASES))} == {0.0, 0.1, 1.0}                      # none, -20 dB, 0 dB
    a, b = R.case_signals(5), R.case_signals(5)
    assert all(x.dtype == np.float32 and np.array_equal(x, y) for x, y in zip(a, b))                     # seeded
    assert R.CHANNEL is S.CHANNEL and R.reference is S.reference and R.lag_sums is S.lag_sums


def test_reference_is_unambiguous_on_every_case(table):
    """LU and block Levinson agree within 1e-9 dB on SIR and SAR and cond(G) <= 1e8: what keeps the GPU test honest."""
    for c in table:
        lu, lev = c["lu"], c["lev"]
        cond = R.condition(lu["lags"])
        print(c["K"], c["L"], f"cond {cond:.2g}", lu["sdr"], lu["sir"], lu["sar"], abs(lu["sir"] - lev["sir"]), abs(lu["sar"] - lev["sar"]))
        assert cond <= 1e8
        for name in ("sir", "sar"):
            assert math.isfinite(lu[name]) and abs(lu[name] - lev[name]) <= 1e-9, (c["L"], c["K"], name, lu[name], lev[name])
        assert lu["interf_energy"] > 0 and lu["artif_energy"] > 0 and lu["projection_energy"] > 0
        assert R.residual(lu["filters"], lu["lags"]) < 1e-13 and R.residual(lev["filters"], lev["lags"]) < 1e-13
        assert 0 < lu["sir"] < 60 and 0 < lu["sar"] < 60                                                 # values, not rounding levels


def test_sdr_is_the_one_source_sdr_to_the_last_bit(table):
    for c in table:
        one = S.sdr(c["s"], c["y"], c["K"])
        for got in (c["lu"], c["lev"]):
            assert got["sdr"] == one["sdr"] and got["target_energy"] == one["target_energy"] and got["error_energy"] == one["error_energy"]
            assert np.array_equal(got["filter"], one["filter"])


def test_joint_matrix_is_the_gram_matrix_of_the_convolution_matrices():
    """G built from the lags equals A'A of the explicit (L + K - 1) x 2K convolution matrix within 1e-12 of x_ss[0], at K = 16."""
    K = 16
    for index, (L, Kc, kind) in enumerate(R.CASES):
        if Kc != K:
            continue
        s, v, y = (a.astype(np.float64) for a in R.case_signals(index))
        A = np.zeros((L + K - 1, 2 * K))
        for k in range(K):
            A[k:k + L, k] = s
            A[k:k + L, K + k] = v
        lg = R.lags(s, v, y, K)
        G = R.joint_matrix(lg)
        assert np.array_equal(G, G.T)
        assert np.abs(G - A.T @ A).max() <= 1e-12 * lg["ss"][0]
        ypad = np.concatenate([y, np.zeros(K - 1)])
        assert np.abs(np.concatenate([lg["ds"], lg["dv"]]) - A.T @ ypad).max() <= 1e-12 * lg["ss"][0]
        # the projection of the definition is the least-squares fit on both sources
        got = R.bss(s, v, y, K)
        fit = A @ np.linalg.lstsq(A, ypad, rcond=None)[0]
        assert abs(got["projection_energy"] - np.sum(fit * fit)) <= 1e-9 * got["projection_energy"]


def test_special_rows():
    L, K = 600, 64
    s, v = R.reference(L, "lowpass", seed=3), R.reference(L, "white", seed=4)
    y = R.mixture(s, v, 20, 1.0, seed=5)
    z = np.zeros(L, dtype=np.float32)
    nan3 = lambda r: all(math.isnan(r[n]) for n in ("sdr", "sir", "sar"))
    only_sdr = lambda r, w: (r["sdr"] == w and math.isnan(r["sir"]) and math.isnan(r["sar"]) and np.isnan(r["filters"]).all()
                             and all(math.isnan(r[n]) for n in ("interf_energy", "projection_energy", "artif_energy")))
    assert nan3(R.bss(z, v, y, K))                                                                       # a silent reference
    assert only_sdr(R.bss(s, z, y, K), S.sdr(s, y, K)["sdr"])                                            # a silent interferer
    q = R.bss(s, v, z, K)                                                                                # a silent estimate: zero numerators
    assert q["sdr"] == q["sir"] == q["sar"] == -np.inf
    for n in (1, K - 1, K):                                                                              # L <= K: G is singular
        assert only_sdr(R.bss(s[:n], v[:n], y[:n], K), S.sdr(s[:n], y[:n], K)["sdr"])
        if n > 1:
            lg = R.lags(s[:n].astype(np.float64), v[:n].astype(np.float64), y[:n].astype(np.float64), K)
            assert np.linalg.matrix_rank(R.joint_matrix(lg)) < 2 * K
    assert math.isfinite(R.bss(s[:K + 1], v[:K + 1], y[:K + 1], K)["sar"])                               # valid, if overfitted
    two = (2 * s).astype(np.float32)                                                                     # v = 2 s: a pivot that is not positive
    for solver in ("lu", "levinson"):
        assert only_sdr(R.bss(s, two, y, K, solver=solver), S.sdr(s, y, K)["sdr"])
    # an exactly filtered copy of the target alone (the reference ends in silence, so the cut takes nothing away)
    s2 = s.copy()
    s2[-16:] = 0
    d = np.zeros(L)
    d[3:] = 0.5 * s2[:-3]
    r = R.bss(s2, v, d, K)
    assert all(r[n] == np.inf or r[n] > 200 for n in ("sdr", "sir", "sar"))
    assert abs(r["filters"][0, 3] - 0.5) < 1e-9 and np.abs(r["filters"][1]).max() < 1e-9
    with pytest.raises(ValueError):
        R.bss(s, v[:-1], y, K)
    with pytest.raises(ValueError):
        R.bss(s, v, y, K, solver="cholesky")


def test_rationale_of_the_issue():
    """Two estimates with one SDR: leakage of the other source against white artifacts of the same energy."""
    L, K = 8000, 64
    s, v = R.reference(L, "lowpass", seed=21), R.reference(L, "white", seed=22)
    leak = 0.1 * v.astype(np.float64)
    nz = np.random.default_rng(23).standard_normal(L)
    nz *= np.sqrt(np.sum(leak * leak) / np.sum(nz * nz))
    a, b = R.bss(s, v, (s + leak).astype(np.float32), K), R.bss(s, v, (s + nz).astype(np.float32), K)
    assert abs(a["sdr"] - b["sdr"]) < 0.5 and b["sir"] - a["sir"] > 10 and a["sar"] - b["sar"] > 10


def test_filt_len_guards():
    e = torch.zeros(2, 2000)
    for bad in (0, 8, 24, 520, 1024, True, 512.0, -16, None, "512"):
        with pytest.raises(ValueError, match="filt_len"):
            INF.compute_bss(e, e, e, filt_len=bad)
    for good in (16, 64, 496, 512):
        with pytest.raises(LIB.IdvError, match="no CPU fallback"):           # every value guard passed
            INF.compute_bss(e, e, e, filt_len=good)


def test_guards_raise_before_gpu_work():
    e, r, v = torch.zeros(3, 2000), torch.zeros(3, 2000), torch.zeros(3, 2000)
    ok = [2000, 1500, 300]
    fn = INF.compute_bss
    with pytest.raises(ValueError, match="must be tensors"):
        fn(e.numpy(), r, v)
    with pytest.raises(ValueError, match="must be tensors"):
        fn(e, r, v.numpy())
    with pytest.raises(ValueError, match="expected"):
        fn(e[None], r[None], v[None])
    with pytest.raises(ValueError, match="batch size"):
        fn(e, r[:2], v, lengths=ok)
    with pytest.raises(ValueError, match="batch size"):
        fn(e, r, v[:2], lengths=ok)
    with pytest.raises(ValueError, match="differ"):
        fn(e, r[:, :1999], v)
    with pytest.raises(ValueError, match="differ"):
        fn(e, r, v[:, :1999])
    with pytest.raises(ValueError, match="empty"):
        fn(e[:, :0], r[:, :0], v[:, :0])
    with pytest.raises(ValueError, match="2 lengths for a batch of 3"):
        fn(e, r, v, lengths=ok[:2])
    with pytest.raises(ValueError, match="exceeds"):
        fn(e, r, v, lengths=[2001, 1500, 300])
    with pytest.raises(ValueError, match="exceeds"):
        fn(e, r, v[:, :1999], lengths=ok)                                    # beyond the shortest row of the three
    with pytest.raises(ValueError, match="positive"):
        fn(e, r, v, lengths=[2000, 0, 300])
    with pytest.raises(ValueError, match="integers"):
        fn(e, r, v, lengths=[2000.0, 1500, 300])
    # all value guards passed: the CPU tensors are refused before any launch
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        fn(e, r, v, lengths=ok)
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        fn(e[0], r[0], v[0], details=True)
    doc = fn.__doc__
    assert "ESTIMATE FIRST" in doc and "bss_eval_sources" in doc and "roles swapped" in doc and "OVERFITTED" in doc
    assert "pinned only where it is installed" in doc


def test_score_list_knows_the_names():
    sig = [torch.zeros(400), torch.zeros(300)]
    assert INF.BSS_METRICS == ("sir", "sar") and '"sir"' in INF.score_list.__doc__ and "interferers" in INF.score_list.__doc__
    for name in ("sir", "sar"):
        with pytest.raises(ValueError, match="interferers"):
            INF.score_list(sig, sig, metrics=("sdr", name))
    with pytest.raises(ValueError, match="1 interferers for 2 estimates"):
        INF.score_list(sig, sig, metrics=("sir",), interferers=sig[:1])
    with pytest.raises(ValueError, match="metric 'pesq'"):
        INF.score_list(sig, sig, metrics=("sir", "pesq"), interferers=sig)
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):
        INF.score_list(sig, sig, metrics=("sir", "sar"), interferers=sig)
    with pytest.raises(LIB.IdvError, match="no CPU fallback"):               # a call that was valid before
        INF.score_list(sig, sig, metrics=("sdr",))


def test_bss_ref_matches_mir_eval():
    """The pin for a machine that has the package: the reference restates bss_eval_sources for two sources, read for source 0."""
    mir_eval = pytest.importorskip("mir_eval")
    for index, (L, K, kind) in enumerate(R.CASES):
        if K != 512:
            continue                                                         # the package's own filter length
        s, v, y = (a.astype(np.float64) for a in R.case_signals(index))
        # the second estimate is the interferer itself: it has no part in source 0's figures
        sdr, sir, sar, _ = mir_eval.separation.bss_eval_sources(np.stack([s, v]), np.stack([y, v]), compute_permutation=False)
        got = R.bss(s, v, y, K)
        assert abs(got["sdr"] - sdr[0]) < 1e-6 and abs(got["sir"] - sir[0]) < 1e-6 and abs(got["sar"] - sar[0]) < 1e-6, (L, got, sdr, sir, sar)
