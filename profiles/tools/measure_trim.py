"""Throughput of silence trimming on the device: inference.trim_list, the bounds-only path (inference.trim_bounds_list, what the segment
index uses) and the two kernels alone on batches padded beforehand, against the float64 host definition of tests/trim_ref.py.

    python profiles/tools/measure_trim.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--reps 250] [--kernel-reps 10000]
                                          [--host-count 0] [--out profiles/trim/measure.json]

``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz (the set of measure_prepare.py), PCM16 noise under the fade
of trim_ref.fade, so that ends are really cut.
  trim_list / trim_bounds_list:  one untimed pass first, then ``--passes`` timed ones (HIP events around the pass and a host clock ended
                  by a synchronise); a pass goes over the set ``--reps`` times, so that a timed window is half a second or more, and
                  reports the time of one.  The padding copies and the fetch of the bounds are part of the pass.
  bounds_kernels: idv_trim_bounds alone on the batches trim_list forms, padded before the clock starts; a pass goes over them
                  ``--kernel-reps`` times.  bytes = 4 x the samples of the rows, each read once; the rate is bytes over the device time
                  of the pass and is quoted against the 8 TB/s of HBM3E.  It is a rate of the whole call sequence (two launches per
                  batch), not of one kernel, and the set (87 MB at the defaults) fits the 256 MiB Infinity Cache, which repeated
                  passes read from.
  host:           tests/trim_ref.trim, one process, one thread, on the first ``--host-count`` utterances (0: all of them); its bounds
                  must equal the device's.
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

os.environ.setdefault("OMP_NUM_THREADS", "1")               # the host definition runs on one thread

import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_ragged as MR  # noqa: E402
import trim_ref as R  # noqa: E402

SR = 16000
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=250)
    ap.add_argument("--kernel-reps", type=int, default=10000)
    ap.add_argument("--host-count", type=int, default=0)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--top-db", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_trim.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    inf = importlib.import_module("i-dccrn-vae_amd.inference")
    ops = importlib.import_module("i-dccrn-vae_amd.ops")
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    audio_s = sum(lens) / SR
    base = {"count": a.count, "audio_s": round(audio_s, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed, "top_db": a.top_db,
            "max_batch": a.max_batch}
    results = {}

    def timed(fn, reps):
        def many():
            for _ in range(reps):
                out = fn()
            return out
        keep = []
        dev, wall = MR.timed(lambda: keep.append(many()), a.passes)
        return [v / reps for v in dev], [v / reps for v in wall], keep[-1]

    def record(key, rec, dev, wall, reps):
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, reps_per_pass=reps, device_s_per_pass=[round(v, 6) for v in dev], wall_s_per_pass=[round(v, 6) for v in wall],
                   utt_per_s=round(a.count / w, 1), audio_s_per_s=round(audio_s / w, 1), utt_per_s_device=round(a.count / d, 1))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return d, w

    host_x = [R.fade(n, k) for k, n in enumerate(lens)]
    sig = [torch.from_numpy(v).cuda() for v in host_x]
    dev, wall, (got, bounds) = timed(lambda: inf.trim_list(sig, a.top_db, a.max_batch), a.reps)
    kept = sum(int(g.shape[0]) for g in got)
    _, w_list = record("trim_list", {"metric": "trim", "mode": "trim_list", "samples_kept_share": round(kept / sum(lens), 4)}, dev, wall, a.reps)
    dev, wall, bounds2 = timed(lambda: inf.trim_bounds_list(sig, a.top_db, a.max_batch), a.reps)
    assert bounds2 == bounds
    _, w_bounds = record("trim_bounds_list", {"metric": "trim", "mode": "trim_bounds_list"}, dev, wall, a.reps)

    batches = []
    for batch in inf._trim_batches(lens, a.max_batch):
        blens = [lens[k] for k in batch]
        batches.append((inf._trim_pad([sig[k] for k in batch], "cuda"), ops.Lengths(blens, "cuda")))
    dev, wall, _ = timed(lambda: [ops.trim_bounds(x, a.top_db, R.FRAME, R.HOP, ln) for x, ln in batches], a.kernel_reps)
    d = sorted(dev)[len(dev) // 2]
    nbytes = 4 * sum(lens)
    record("bounds_kernels", {"metric": "trim", "mode": "bounds_kernels", "launches_per_pass": 2 * len(batches), "bytes_read": nbytes,
                              "read_bytes_per_s": round(nbytes / d, 0), "share_of_8TBps": round(nbytes / d / HBM_BYTES_PER_S, 4)}, dev, wall, a.kernel_reps)

    n_host = a.count if a.host_count <= 0 else min(a.count, a.host_count)
    R.trim(host_x[0][:4096], a.top_db)                       # numpy's first call stays out of the host's time
    t0 = time.perf_counter()
    want = [R.trim(v, a.top_db) for v in host_x[:n_host]]
    t_host = time.perf_counter() - t0
    rec = dict(base, metric="trim", mode="host_trim_ref_float64", utterances=n_host, wall_s=round(t_host, 3),
               utt_per_s=round(n_host / t_host, 2), bounds_equal_device=want == bounds[:n_host],
               speedup_trim_list=round((a.count / w_list) / (n_host / t_host), 1),
               speedup_bounds_only=round((a.count / w_bounds) / (n_host / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host_trim_ref"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
