"""Throughput of ESTOI scoring of a set of utterances of different lengths: inference.score_list against the float64 host
reference of the tests, and against the enhancement of the same folder.

    python profiles/tools/measure_stoi.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--host-count 32]
                                          [--no-enhance] [--out profiles/stoi/measure.json]

``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz; the signals are the "speech" of tests/stoi_ref.py (a
harmonic carrier with pauses, so the silent-frame removal has work to do) and estimates at 0 dB SNR.
  score_list:  ``score_list(estimates, references, metrics=("estoi",))`` and the default ``("sisdr", "estoi")``; one untimed pass
               first, then ``--passes`` timed ones (HIP events around the pass and a host clock ended by a synchronise);
  host:        ``stoi_ref.stoi(..., extended=True)`` in float64, one process, one thread, on the first ``--host-count`` utterances
               (0: all of them) -- what a user without the package's GPU port runs per file;
  enhance:     ``enhance_list`` of measure_ragged.py (full-width DCCRN-CL, fp32) on the same lengths, for the share of an evaluation
               loop that scoring takes.
One JSON line per mode on stdout; ``--out`` writes them into one JSON file keyed by mode.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import random
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")               # the host reference runs on one thread

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_ragged as MR  # noqa: E402
import stoi_ref as R  # noqa: E402

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-count", type=int, default=32)
    ap.add_argument("--no-enhance", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_stoi.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    model, inf = MR.build(HERE)
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    clean = [R.speech(n, seed=k).astype(np.float32) for k, n in enumerate(lens)]
    noisy = [R.noisy(x.astype(np.float64), 0, seed=1000 + k).astype(np.float32) for k, x in enumerate(clean)]
    refs = [torch.from_numpy(x).cuda() for x in clean]
    ests = [torch.from_numpy(y).cuda() for y in noisy]
    audio_s = sum(lens) / SR
    base = {"count": a.count, "audio_s": round(audio_s, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed}
    results = {}

    def record(key, rec, dev, wall, n):
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, device_s_per_pass=[round(v, 4) for v in dev], wall_s_per_pass=[round(v, 4) for v in wall],
                   utt_per_s=round(n / w, 1), audio_s_per_s=round(audio_s / w, 1), utt_per_s_device=round(n / d, 1))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return w

    got = {}
    dev, wall = MR.timed(lambda: got.update(inf.score_list(ests, refs, metrics=("estoi",))), a.passes)
    w_estoi = record("score_list_estoi", {"metric": "stoi_scoring", "mode": "score_list", "metrics": ["estoi"]}, dev, wall, a.count)
    dev, wall = MR.timed(lambda: inf.score_list(ests, refs), a.passes)
    w_both = record("score_list_default", {"metric": "stoi_scoring", "mode": "score_list", "metrics": ["sisdr", "estoi"]}, dev, wall,
                    a.count)

    n_host = a.count if a.host_count <= 0 else min(a.count, a.host_count)
    t0 = time.perf_counter()
    host = [R.stoi(clean[k], noisy[k], SR, True)[0] for k in range(n_host)]
    t_host = time.perf_counter() - t0
    dev_max = max(abs(float(got["estoi"][k]) - host[k]) for k in range(n_host))
    rec = dict(base, metric="stoi_scoring", mode="host_float64", utterances=n_host, wall_s=round(t_host, 3),
               utt_per_s=round(n_host / t_host, 2), audio_s_per_s=round(sum(lens[:n_host]) / SR / t_host, 1),
               max_abs_dev_of_score_list=float(f"{dev_max:.3g}"),
               speedup_estoi=round((a.count / w_estoi) / (n_host / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host_float64"] = rec

    if not a.no_enhance:
        dev, wall = MR.timed(lambda: inf.enhance_list(functools.partial(inf.enhance_supervised, model), ests, MR.HOP), a.passes)
        w_enh = record("enhance_list", {"metric": "ragged_enhance", "mode": "list"}, dev, wall, a.count)
        rec = dict(base, metric="stoi_scoring", mode="share", estoi_over_enhance=round(w_estoi / w_enh, 3),
                   sisdr_estoi_over_enhance=round(w_both / w_enh, 3))
        print(json.dumps(rec), flush=True)
        results["share"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
