"""Throughput of mixture synthesis on the device (dataset/mix.py, csrc/mix.hip) against the float64 host definition of tests/mix_ref.py
and against a train step.

    python profiles/tools/measure_mix.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--reps 800] [--host-count 0]
                                         [--train-workload dccrn_cl_train] [--train-batch 32] [--out profiles/mix/measure.json]

``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz (the set of measure_trim.py), 0.1 N(0, 1) clean rows, noise
rows of 3 s read cyclically from seeded offsets, SNRs uniform in [-5, 20] dB, levels in [-35, -15] dB.
  snr_mix_plain / snr_mix_segmental:  ``snr_mix`` on batches of ``--max-batch`` utterances sorted by length, padded before the clock
                  starts; one untimed pass first, then ``--passes`` timed ones (HIP events around the pass and a host clock ended by a
                  synchronise); a pass goes over the set ``--reps`` times, so that a timed window is half a second or more, and reports
                  the time of one.  The uploads of the per-row tables are part of the pass.  bytes = 4 x 5 x the samples of the rows: the algorithm's MINIMUM of five row transfers (clean and
                  noise read once, three outputs written once) -- the kernels read both inputs three times (two statistics passes and the
                  write), which the rate does not count; it is quoted against the 8 TB/s of HBM3E and is a rate of the whole call sequence
                  (five launches per batch), with a set that largely fits the 256 MiB Infinity Cache.
  dynamic:        ``DynamicMixtures.batch(k)`` at the training shape B = 64 x 64000 from pools of the same recordings, fresh k each time.
  host:           tests/mix_ref.mix, one process, one thread, on the first ``--host-count`` utterances (0: all of them).
  train_share:    the device time of one ``DynamicMixtures`` batch of ``--train-batch`` rows over the device time of one fp32 step of
                  bench.py's ``--train-workload`` at the same batch, measured in this run.
One JSON line per mode on stdout; ``--out`` writes them into one JSON file keyed by mode.  Fails without a GPU: there is no fallback.
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

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_ragged as MR  # noqa: E402
import mix_ref as R  # noqa: E402

SR = 16000
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--noise-s", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=800)
    ap.add_argument("--host-count", type=int, default=0)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--train-workload", default="dccrn_cl_train")
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--train-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_mix.py measures on the GPU; there is nothing to report without one")
    torch.set_num_threads(1)
    M = importlib.import_module("i-dccrn-vae_amd.dataset.mix")
    rng = random.Random(a.seed)
    lens = sorted(rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count))
    m = int(a.noise_s * SR)
    offs = [rng.randrange(m) for _ in lens]
    snrs = [rng.uniform(-5.0, 20.0) for _ in lens]
    levels = [float(rng.randrange(-35, -15)) for _ in lens]
    audio_s = sum(lens) / SR
    base = {"count": a.count, "audio_s": round(audio_s, 1), "lengths_s": [a.min_s, a.max_s], "noise_s": a.noise_s, "seed": a.seed,
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

    def record(key, rec, dev, wall, reps, count):
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, reps_per_pass=reps, device_s_per_pass=[round(v, 6) for v in dev], wall_s_per_pass=[round(v, 6) for v in wall],
                   utt_per_s=round(count / w, 1), utt_per_s_device=round(count / d, 1))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return d, w

    host_c = [(0.1 * np.random.default_rng(1000 + k).standard_normal(n)).astype(np.float32) for k, n in enumerate(lens)]
    host_v = [(0.1 * np.random.default_rng(5000 + k).standard_normal(m)).astype(np.float32) for k in range(len(lens))]
    batches = []
    for g0 in range(0, a.count, a.max_batch):
        sl = slice(g0, g0 + a.max_batch)
        c = torch.zeros(len(lens[sl]), max(lens[sl]))
        for b, r in enumerate(host_c[sl]):
            c[b, :len(r)] = torch.from_numpy(r)
        batches.append((c.cuda(), torch.from_numpy(np.stack(host_v[sl])).cuda(), sl))
    nbytes = 4 * 5 * sum(lens)
    first = {}
    for seg in (False, True):
        fn = lambda: [M.snr_mix(c, v, snrs[sl], levels[sl], lengths=lens[sl], noise_offsets=offs[sl], segmental=seg) for c, v, sl in batches]
        dev, wall, out = timed(fn, a.reps)
        first[seg] = out[0]
        d = sorted(dev)[len(dev) // 2]
        key = "snr_mix_segmental" if seg else "snr_mix_plain"
        record(key, {"metric": "mix", "mode": key, "launches_per_pass": 5 * len(batches), "min_bytes_moved": nbytes,
                     "min_bytes_label": "five row transfers: two inputs read once, three outputs written once",
                     "min_bytes_per_s": round(nbytes / d, 0), "share_of_8TBps": round(nbytes / d / HBM_BYTES_PER_S, 4)}, dev, wall, a.reps,
               a.count)
    w_plain = sorted(results["snr_mix_plain"]["wall_s_per_pass"])[a.passes // 2]

    cp, npool = M.SignalPool(host_c, "cuda"), M.SignalPool(host_v, "cuda")
    counter = [0]

    def dyn(dm):
        counter[0] += 1
        return dm.batch(counter[0])
    dm64 = M.DynamicMixtures(cp, npool, 64, samples=64000, seed=a.seed)
    dev, wall, _ = timed(lambda: dyn(dm64), a.reps * 2)
    record("dynamic", {"metric": "mix", "mode": "dynamic_mixtures", "batch": 64, "samples": 64000}, dev, wall, a.reps * 2, 64)

    n_host = a.count if a.host_count <= 0 else min(a.count, a.host_count)
    R.mix(host_c[0][:4096], host_v[0], 0, 5.0)                # numpy's first call stays out of the host's time
    t0 = time.perf_counter()
    want = [R.mix(host_c[k], host_v[k], offs[k], snrs[k], levels[k]) for k in range(n_host)]
    t_host = time.perf_counter() - t0
    nb = min(n_host, a.max_batch)
    got = first[False][3]
    g_dev, clip_dev = got["g_clean"][:nb].cpu().numpy(), got["clipped"][:nb].tolist()
    rec = dict(base, metric="mix", mode="host_mix_ref_float64", utterances=n_host, wall_s=round(t_host, 3), utt_per_s=round(n_host / t_host, 2),
               worst_relative_gain_difference=float(max(abs(g_dev[k] - want[k]["g_clean"]) / want[k]["g_clean"] for k in range(nb))),
               clipped_equal_device=clip_dev == [r["clipped"] for r in want[:nb]],
               speedup_snr_mix=round((a.count / w_plain) / (n_host / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host_mix_ref"] = rec

    bench = importlib.import_module("bench")
    dmb = M.DynamicMixtures(cp, npool, a.train_batch, samples=bench.LEN, seed=a.seed)
    dev, _, _ = timed(lambda: dyn(dmb), a.reps * 2)
    d_mix = sorted(dev)[len(dev) // 2]
    step, _, what = bench.build_workload(a.train_workload, a.train_batch, "cuda", 0)
    dev, _, _ = timed(step, a.train_steps)
    d_step = sorted(dev)[len(dev) // 2]
    rec = {"metric": "mix", "mode": "train_share", "workload": a.train_workload, "precision": "fp32", "batch": a.train_batch,
           "samples": bench.LEN, "what": what["workload"], "mix_device_s": round(d_mix, 6), "step_device_s": round(d_step, 6),
           "mix_share_of_step": round(d_mix / d_step, 5)}
    print(json.dumps(rec), flush=True)
    results["train_share"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
