"""Throughput of BSS-eval SDR / SIR / SAR scoring with the noise as second source (512-tap filters) of a set of utterances of different
lengths: inference.score_list with interferers= against the float64 host definition of the tests, and against the enhancement of the
same folder.

    python profiles/tools/measure_bss.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--host-count 32]
                                         [--no-enhance] [--kernels-only] [--kernel-stats DB] [--out profiles/bss/measure.json]

``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz; the targets are the "speech" of tests/stoi_ref.py, the
interferers white noise at half their scale, the estimates the mixtures of tests/bss_ref.py (the target through its 9-tap channel, the
interferer through the 6-tap path at -20 dB, white artifacts at 20 dB).
  score_list:  ``score_list(estimates, references, metrics=("sdr", "sir", "sar"), interferers=...)``; one untimed pass first, then
               ``--passes`` timed ones (HIP events around the pass and a host clock ended by a synchronise); beside it
               ``score_list(metrics=("sdr",))`` alone, what the two more columns cost;
  host:        ``bss_ref.bss(..., 512)`` in float64, one process, one thread, on the first ``--host-count`` utterances (0: all);
  enhance:     ``enhance_list`` of measure_ragged.py (full-width DCCRN-CL, fp32) on the same lengths, in the same run, for the share of
               an evaluation loop that the metric takes;
  kernels:     the device times of the passes come from a kernel trace taken in a run of its own,
               ``rocprofv3 --kernel-trace --stats -d DIR -o bss -- python profiles/tools/measure_bss.py --kernels-only``
               (two passes of score_list and nothing else), whose ``bss_results.db`` goes in with ``--kernel-stats``: time per pass
               and mean time per kernel and, for the MFMA passes, the achieved f64 TFLOP/s over the useful work
               (12 K n flop per row for the six lag sets, 6 K (n + K - 1) for p1 and pall).
One JSON line per mode on stdout; ``--out`` writes them into one JSON file keyed by mode.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import random
import sqlite3
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")               # the host definition runs on one thread

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bss_ref as R  # noqa: E402
import measure_ragged as MR  # noqa: E402
import stoi_ref as S  # noqa: E402

SR, K = 16000, 512
TRACED_PASSES = 2                                            # what --kernels-only runs
METRICS = ("sdr", "sir", "sar")
KERNELS = ("sdr_corr_kernel", "sdr_solve_kernel", "sdr_proj_kernel", "sdr_final_kernel", "bss_corr_kernel", "bss_solve_kernel",
           "bss_proj_kernel", "bss_final_kernel")


def kernel_stats(path, lens):
    """The sdr_* and bss_* dispatches of a rocprofv3 kernel trace database (its ``kernels`` view) -> {kernel: calls, ms_per_pass,
    mean_us[, f64_tflops]}."""
    flop = {"sdr_corr_kernel": sum(4.0 * K * n for n in lens), "sdr_proj_kernel": sum(2.0 * K * (n + K - 1) for n in lens),
            "bss_corr_kernel": sum(12.0 * K * n for n in lens), "bss_proj_kernel": sum(6.0 * K * (n + K - 1) for n in lens)}
    out = {}
    db = sqlite3.connect(path)
    for name, calls, total_ns in db.execute('select name, count(*), sum("end" - start) from kernels group by name'):
        short = next((k for k in KERNELS if k in name), None)
        if short is None:
            continue
        rec = {"calls": calls, "ms_per_pass": round(total_ns / 1e6 / TRACED_PASSES, 3), "mean_us": round(total_ns / calls / 1e3, 1)}
        if short in flop:
            rec["f64_tflops"] = round(TRACED_PASSES * flop[short] / (total_ns * 1e-9) / 1e12, 1)
        out[short] = rec
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-count", type=int, default=32)
    ap.add_argument("--no-enhance", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_bss.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    clean = [S.speech(n, seed=k).astype(np.float32) for k, n in enumerate(lens)]
    scale = [float(np.sqrt(np.mean(x.astype(np.float64) ** 2))) for x in clean]
    noise = [(0.5 * g * np.random.default_rng(4000 + k).standard_normal(n)).astype(np.float32) for k, (n, g) in enumerate(zip(lens, scale))]
    noisy = [R.mixture(s, v, 20, 0.1, seed=k) for k, (s, v) in enumerate(zip(clean, noise))]
    refs = [torch.from_numpy(x).cuda() for x in clean]
    nses = [torch.from_numpy(x).cuda() for x in noise]
    ests = [torch.from_numpy(y).cuda() for y in noisy]
    if a.kernels_only:
        import importlib
        sys.path.insert(0, HERE)
        inf = importlib.import_module("i-dccrn-vae_amd.inference")
        for _ in range(TRACED_PASSES):
            inf.score_list(ests, refs, metrics=METRICS, interferers=nses)
        torch.cuda.synchronize()
        return
    model, inf = MR.build(HERE)
    audio_s = sum(lens) / SR
    base = {"count": a.count, "audio_s": round(audio_s, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed, "filt_len": K}
    results = {}

    def record(key, rec, dev, wall, n):
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, device_s_per_pass=[round(v, 4) for v in dev], wall_s_per_pass=[round(v, 4) for v in wall],
                   utt_per_s=round(n / w, 1), audio_s_per_s=round(audio_s / w, 1), utt_per_s_device=round(n / d, 1))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return w

    got = {}
    dev, wall = MR.timed(lambda: got.update(inf.score_list(ests, refs, metrics=METRICS, interferers=nses)), a.passes)
    w_bss = record("score_list_sdr_sir_sar", {"metric": "bss_scoring", "mode": "score_list", "metrics": list(METRICS)}, dev, wall, a.count)
    dev, wall = MR.timed(lambda: inf.score_list(ests, refs, metrics=("sdr",)), a.passes)
    w_sdr = record("score_list_sdr", {"metric": "bss_scoring", "mode": "score_list", "metrics": ["sdr"]}, dev, wall, a.count)

    n_host = a.count if a.host_count <= 0 else min(a.count, a.host_count)
    t0 = time.perf_counter()
    host = [R.bss(clean[k], noise[k], noisy[k], K) for k in range(n_host)]
    t_host = time.perf_counter() - t0
    dev_max = {m: max(abs(float(got[m][k]) - host[k][m]) for k in range(n_host)) for m in METRICS}
    rec = dict(base, metric="bss_scoring", mode="host_float64", utterances=n_host, wall_s=round(t_host, 3),
               utt_per_s=round(n_host / t_host, 2), audio_s_per_s=round(sum(lens[:n_host]) / SR / t_host, 1),
               max_abs_dev_db_of_score_list={m: float(f"{v:.3g}") for m, v in dev_max.items()},
               value_range_db={m: [round(min(h[m] for h in host), 2), round(max(h[m] for h in host), 2)] for m in METRICS},
               speedup=round((a.count / w_bss) / (n_host / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host_float64"] = rec

    if not a.no_enhance:
        dev, wall = MR.timed(lambda: inf.enhance_list(functools.partial(inf.enhance_supervised, model), ests, MR.HOP), a.passes)
        w_enh = record("enhance_list", {"metric": "ragged_enhance", "mode": "list"}, dev, wall, a.count)
        rec = dict(base, metric="bss_scoring", mode="share", bss_over_enhance=round(w_bss / w_enh, 3), sdr_over_enhance=round(w_sdr / w_enh, 3),
                   bss_over_sdr=round(w_bss / w_sdr, 2))
        print(json.dumps(rec), flush=True)
        results["share"] = rec
    if a.kernel_stats:
        rec = dict(base, metric="bss_scoring", mode="kernels", traced_passes=TRACED_PASSES, kernels=kernel_stats(a.kernel_stats, lens))
        print(json.dumps(rec), flush=True)
        results["kernels"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
