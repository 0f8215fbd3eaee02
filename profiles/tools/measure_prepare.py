"""Throughput of corpus preparation on the device: inference.resample_list and dataset.stats.cal_mean_std on a set of utterances of
different lengths, against the float64 host definitions of tests/prepare_ref.py.

    python profiles/tools/measure_prepare.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--reps 25]
                                             [--host-count 16] [--out profiles/prepare/measure.json]

``--count`` seeded lengths uniform in [--min-s, --max-s] seconds (the set of measure_stoi.py / measure_ragged.py), 0.05 N(0, 1) + 0.5.
  resample_list:  the same durations at 48 kHz and at 44.1 kHz -> 16 kHz; one untimed pass first, then ``--passes`` timed ones (HIP
                  events around the pass and a host clock ended by a synchronise); a pass goes over the set ``--reps`` times, so
                  that a timed window is a tenth of a second and not a few milliseconds, and reports the time of one;
  cal_mean_std:   n_fft / win / hop = 512 / 400 / 100 on the 16 kHz tensors already on the device, ``result()`` included;
  host:           ``scipy.signal.resample_poly`` in float64 and the two-pass float64 moments of prepare_ref, one process, one thread,
                  on the first ``--host-count`` utterances (0: all of them), with the largest deviation of the device's tables from
                  the host's on those utterances.
One JSON line per mode on stdout; ``--out`` writes them into one JSON file keyed by mode.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import random
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")               # the host definitions run on one thread

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_ragged as MR  # noqa: E402
import prepare_ref as R  # noqa: E402

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--host-count", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_prepare.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    inf = importlib.import_module("i-dccrn-vae_amd.inference")
    stats = importlib.import_module("i-dccrn-vae_amd.dataset.stats")
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    audio_s = sum(lens) / SR
    base = {"count": a.count, "audio_s": round(audio_s, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed}
    results = {}

    def timed(fn):
        def many():
            for _ in range(a.reps):
                out = fn()
            return out
        keep = []
        dev, wall = MR.timed(lambda: keep.append(many()), a.passes)
        return [v / a.reps for v in dev], [v / a.reps for v in wall], keep[-1]

    def record(key, rec, dev, wall, n):
        rec["reps_per_pass"] = a.reps
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, device_s_per_pass=[round(v, 5) for v in dev], wall_s_per_pass=[round(v, 5) for v in wall],
                   utt_per_s=round(n / w, 1), audio_s_per_s=round(audio_s / w, 1), utt_per_s_device=round(n / d, 1))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return w

    n_host = a.count if a.host_count <= 0 else min(a.count, a.host_count)
    host_in = {}
    for fs in (48000, 44100):
        x = [R.dc_signal(n * fs // SR, k) for k, n in enumerate(lens)]
        host_in[fs] = x[:n_host]
        sig = [torch.from_numpy(v).cuda() for v in x]
        dev, wall, got = timed(lambda: inf.resample_list(sig, fs, SR))
        w = record(f"resample_list_{fs}", {"metric": "prepare", "mode": "resample_list", "fs_in": fs, "fs_out": SR}, dev, wall, a.count)
        up, down = R.ratio(SR, fs)
        R.resample(host_in[fs][0][:1000], up, down)          # scipy's import and first call stay out of the host's time
        t0 = time.perf_counter()
        want = [R.resample(v, up, down) for v in host_in[fs]]
        t_host = time.perf_counter() - t0
        err = max(float(np.abs(got[k].cpu().numpy() - want[k]).max()) for k in range(n_host))
        rec = dict(base, metric="prepare", mode="host_resample_poly_float64", fs_in=fs, fs_out=SR, utterances=n_host,
                   wall_s=round(t_host, 3), utt_per_s=round(n_host / t_host, 2), max_abs_dev_of_resample_list=float(f"{err:.3g}"),
                   speedup=round((a.count / w) / (n_host / t_host), 1))
        print(json.dumps(rec), flush=True)
        results[f"host_resample_{fs}"] = rec
        del sig, got

    x16 = [R.dc_signal(n, k) for k, n in enumerate(lens)]
    sig = [torch.from_numpy(v).cuda() for v in x16]
    dev, wall, _ = timed(lambda: stats.cal_mean_std(sig, R.NFFT, R.WIN, R.HOP, SR).result())
    w = record("cal_mean_std", {"metric": "prepare", "mode": "cal_mean_std", "n_fft": R.NFFT, "win": R.WIN, "hop": R.HOP,
                                "frames": sum(1 + n // R.HOP for n in lens)}, dev, wall, a.count)
    t0 = time.perf_counter()
    mean, std, frames = R.moments(x16[:n_host], "constant")
    t_host = time.perf_counter() - t0
    part = stats.cal_mean_std(sig[:n_host], R.NFFT, R.WIN, R.HOP, SR).result()
    rec = dict(base, metric="prepare", mode="host_moments_float64", utterances=n_host, frames=frames, wall_s=round(t_host, 3),
               utt_per_s=round(n_host / t_host, 2), max_abs_dev_mean=float(f"{np.abs(part[0] - mean).max():.3g}"),
               max_abs_dev_std=float(f"{np.abs(part[1] - std).max():.3g}"), speedup=round((a.count / w) / (n_host / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host_moments"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
