"""Throughput of reverberation on the device (dataset/reverb.py, csrc/reverb.hip) against scipy.signal.fftconvolve on the host and
against a train step.

    python profiles/tools/measure_reverb.py [--count 256] [--min-s 1] [--max-s 10] [--rirs 32] [--passes 3] [--window-s 0.5]
                                            [--host-count 0] [--train-workload dccrn_cl_train] [--train-batch 32]
                                            [--out profiles/reverb/measure.json]

``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz (the set of measure_trim.py), 0.1 N(0, 1) rows; a seeded
pool of ``--rirs`` impulse responses of 0.2 .. 1.0 s (tests/reverb_ref.rir_row), one drawn per utterance.
  reverb:       ``reverb`` on batches of ``--max-batch`` utterances sorted by length, padded before the clock starts; one untimed pass
                first, then ``--passes`` timed ones (HIP events around the pass and a host clock ended by a synchronise); a pass goes
                over the set as many times as make the timed window ``--window-s`` seconds or more and reports the time of one.  The
                uploads of the per-row tables are part of the pass.  flops: 2 per multiply-add of the definition, sum_i min(i + 1, K)
                of them per row, that is n K LESS the triangle of terms that reach in front of the row (which the kernel skips); the
                zero operands of the first and last tap block and of the last tile of a row are not counted either, so the rate is the
                useful one, below what the matrix unit executes.
  kernel:       the same call at B = 64 x 64000 with 16000 taps per row, one shape, lengths and taps full.
  host:         scipy.signal.fftconvolve in float64, one process, one thread, on the first ``--host-count`` utterances (0: all).
  dynamic_p50 / dynamic_p100:  ``DynamicMixtures.batch(k)`` with the pool at p_reverb = 0.5 and 1.0, B = 64 x 64000, fresh k each
                time; dynamic_dry: the same without a pool.
  train_share:  the device time of one ``DynamicMixtures`` batch of ``--train-batch`` rows (p_reverb = 0.5) over the device time of one
                fp32 step of bench.py's ``--train-workload`` at the same batch, measured in this run.
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

os.environ.setdefault("OMP_NUM_THREADS", "1")               # the host comparator runs on one thread

import numpy as np
import scipy.signal
import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_ragged as MR  # noqa: E402
import reverb_ref as R  # noqa: E402

SR = 16000


def macs(n: int, K: int) -> int:
    """sum_{i < n} min(i + 1, K): the multiply-adds of the definition for a row of n samples under K taps."""
    m = min(n, K)
    return m * (m + 1) // 2 + (n - m) * K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--rirs", type=int, default=32)
    ap.add_argument("--rir-min-s", type=float, default=0.2)
    ap.add_argument("--rir-max-s", type=float, default=1.0)
    ap.add_argument("--noise-s", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--host-count", type=int, default=0)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--train-workload", default="dccrn_cl_train")
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--train-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_reverb.py measures on the GPU; there is nothing to report without one")
    torch.set_num_threads(1)
    M = importlib.import_module("i-dccrn-vae_amd.dataset.mix")
    RV = importlib.import_module("i-dccrn-vae_amd.dataset.reverb")
    rng = random.Random(a.seed)
    lens = sorted(rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count))
    rir_lens = [rng.randint(int(a.rir_min_s * SR), int(a.rir_max_s * SR)) for _ in range(a.rirs)]
    pick = [rng.randrange(a.rirs) for _ in lens]
    base = {"count": a.count, "audio_s": round(sum(lens) / SR, 1), "lengths_s": [a.min_s, a.max_s], "rirs": a.rirs,
            "rir_lengths_s": [a.rir_min_s, a.rir_max_s], "seed": a.seed, "max_batch": a.max_batch}
    results = {}

    def timed(fn):
        """-> (device seconds, wall seconds) per call of fn for every pass, the repetitions of a pass, the last result."""
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps = max(1, int(np.ceil(a.window_s / max(time.perf_counter() - t0, 1e-6))))
        keep = []

        def many():
            for _ in range(reps):
                out = fn()
            keep.append(out)
        dev, wall = MR.timed(many, a.passes)
        return [v / reps for v in dev], [v / reps for v in wall], reps, keep[-1]

    def record(key, rec, dev, wall, reps, count, flops=None):
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, reps_per_pass=reps, device_s_per_pass=[round(v, 6) for v in dev], wall_s_per_pass=[round(v, 6) for v in wall],
                   utt_per_s=round(count / w, 1), utt_per_s_device=round(count / d, 1))
        if flops is not None:
            rec.update(flops=flops, flops_label="2 sum_i min(i + 1, K) per row: 2 n K less the skipped triangle",
                       f64_tflops_device=round(flops / d / 1e12, 2), f64_tflops_wall=round(flops / w / 1e12, 2))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return d, w

    host_x = [(0.1 * np.random.default_rng(1000 + k).standard_normal(n)).astype(np.float32) for k, n in enumerate(lens)]
    host_h = [R.rir_row(K, 2000 + k) for k, K in enumerate(rir_lens)]
    batches = []
    for g0 in range(0, a.count, a.max_batch):
        sl = slice(g0, g0 + a.max_batch)
        x = torch.zeros(len(lens[sl]), max(lens[sl]))
        hk = [rir_lens[j] for j in pick[sl]]
        h = torch.zeros(len(hk), max(hk))
        for b, (r, j) in enumerate(zip(host_x[sl], pick[sl])):
            x[b, :len(r)] = torch.from_numpy(r)
            h[b, :rir_lens[j]] = torch.from_numpy(host_h[j])
        batches.append((x.cuda(), h.cuda(), lens[sl], hk))
    flops = 2 * sum(macs(n, rir_lens[j]) for n, j in zip(lens, pick))
    dev, wall, reps, out = timed(lambda: [RV.reverb(x, h, lengths=ln, rir_lengths=hk) for x, h, ln, hk in batches])
    first = out[0][:8].cpu().numpy()
    _, w_rev = record("reverb", {"metric": "reverb", "mode": "reverb", "launches_per_pass": len(batches),
                                 "flops_nominal_2nK": 2 * sum(n * rir_lens[j] for n, j in zip(lens, pick))}, dev, wall, reps, a.count, flops)

    xk, hk = 0.1 * torch.randn(64, 64000, device="cuda"), torch.from_numpy(np.stack([R.rir_row(16000, 3000 + b) for b in range(64)])).cuda()
    dev, wall, reps, _ = timed(lambda: RV.reverb(xk, hk))
    record("kernel", {"metric": "reverb", "mode": "kernel", "batch": 64, "samples": 64000, "taps": 16000}, dev, wall, reps, 64,
           2 * 64 * macs(64000, 16000))

    n_host = a.count if a.host_count <= 0 else min(a.count, a.host_count)
    scipy.signal.fftconvolve(host_x[0][:4096].astype(np.float64), host_h[0].astype(np.float64))          # the first call stays out of the time
    t0 = time.perf_counter()
    want = [scipy.signal.fftconvolve(host_x[k].astype(np.float64), host_h[pick[k]].astype(np.float64), "full")[:lens[k]] for k in range(n_host)]
    t_host = time.perf_counter() - t0
    diff = max(float(np.abs(first[b, :lens[b]] - want[b]).max() / np.abs(want[b]).max()) for b in range(min(8, n_host)))
    rec = dict(base, metric="reverb", mode="host_fftconvolve_float64", utterances=n_host, wall_s=round(t_host, 3),
               utt_per_s=round(n_host / t_host, 2), worst_difference_over_peak_first_rows=diff,
               speedup_reverb=round((a.count / w_rev) / (n_host / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host"] = rec

    host_v = [(0.1 * np.random.default_rng(5000 + k).standard_normal(int(a.noise_s * SR))).astype(np.float32) for k in range(64)]
    cp, npool, rp = M.SignalPool(host_x, "cuda"), M.SignalPool(host_v, "cuda"), RV.RirPool(host_h, "cuda")
    counter = [0]

    def dyn(dm):
        counter[0] += 1
        return dm.batch(counter[0])
    for key, kw in (("dynamic_dry", {}), ("dynamic_p50", dict(rir_pool=rp, p_reverb=0.5)), ("dynamic_p100", dict(rir_pool=rp, p_reverb=1.0))):
        dm = M.DynamicMixtures(cp, npool, 64, samples=64000, seed=a.seed, **kw)
        dev, wall, reps, _ = timed(lambda: dyn(dm))
        record(key, {"metric": "reverb", "mode": key, "batch": 64, "samples": 64000, "p_reverb": kw.get("p_reverb")}, dev, wall, reps, 64)

    bench = importlib.import_module("bench")
    dmb = M.DynamicMixtures(cp, npool, a.train_batch, samples=bench.LEN, seed=a.seed, rir_pool=rp, p_reverb=0.5)
    dev, _, _, _ = timed(lambda: dyn(dmb))
    d_mix = sorted(dev)[len(dev) // 2]
    step, _, what = bench.build_workload(a.train_workload, a.train_batch, "cuda", 0)
    dev, _ = MR.timed(lambda: [step() for _ in range(a.train_steps)], a.passes)
    d_step = sorted(dev)[len(dev) // 2] / a.train_steps
    rec = {"metric": "reverb", "mode": "train_share", "workload": a.train_workload, "precision": "fp32", "batch": a.train_batch,
           "samples": bench.LEN, "p_reverb": 0.5, "what": what["workload"], "mix_device_s": round(d_mix, 6), "step_device_s": round(d_step, 6),
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
