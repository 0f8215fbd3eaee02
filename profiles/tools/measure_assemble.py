"""Throughput of clip assembly on the device (dataset/assemble.py, csrc/assemble.hip) against the float64 host definition of
tests/assemble_ref.py and against a train step.

    python profiles/tools/measure_assemble.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--reps 100] [--host-rows 8]
                                              [--train-workload dccrn_cl_train] [--train-batch 32] [--out profiles/assemble/measure.json]

A clean pool of ``--count`` seeded PCM16 recordings of [--min-s, --max-s] seconds at 16 kHz whose level steps through loud, faint and
silent stretches (tests/assemble_ref.py ``speech_like``), a noise pool of as many 0.1 N(0, 1) recordings of the same lengths, three
impulse responses of 4000, 8000 and 16000 taps.  Every mode runs one untimed pass first, then ``--passes`` timed ones (HIP events
around the pass and a host clock ended by a synchronise); a pass repeats the call ``--reps`` times and reports the time of one.
  dynamic_plain / dynamic_clips / dynamic_clips_rir:  ``DynamicMixtures.batch(k)`` at B = 64 x 64000, fresh k each time: the parent's
                  path (``clips=False``), ``clips=True``, and ``clips=True`` with the impulse responses at ``p_reverb = 0.5``.
  assemble:       ``assemble`` alone on the clean clips of one batch (tables uploaded in the call), tries = 4.
  activity:       ``activity`` alone on a [64, 64000] batch.
  kernels:        the three kernels alone, from events, the tables already on the device.  min bytes = 4 x the samples of (tries
                  candidates read once by the window pass + the chosen row read and written once by the write), pauses counted as
                  samples; quoted against the 8 TB/s of HBM3E; the pool largely fits the 256 MiB Infinity Cache.
  host:           tests/assemble_ref.assemble, one process, one thread, on ``--host-rows`` rows of 4 candidates.
  train_share:    the device time of one ``DynamicMixtures(clips=True)`` batch of ``--train-batch`` rows over the device time of one
                  fp32 step of bench.py's ``--train-workload`` at the same batch, measured in this run.
  accepted:       the share of rows with ``accepted = 0`` at ``clean_activity = 0.6`` over ``--gate-batches`` batches of 64.
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

import assemble_ref as R  # noqa: E402
import measure_ragged as MR  # noqa: E402
import reverb_ref  # noqa: E402

SR = 16000
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--gate-batches", type=int, default=50)
    ap.add_argument("--train-workload", default="dccrn_cl_train")
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--train-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_assemble.py measures on the GPU; there is nothing to report without one")
    torch.set_num_threads(1)
    M = importlib.import_module("i-dccrn-vae_amd.dataset.mix")
    RV = importlib.import_module("i-dccrn-vae_amd.dataset.reverb")
    ASM = importlib.import_module("i-dccrn-vae_amd.dataset.assemble")
    ops = importlib.import_module("i-dccrn-vae_amd.ops")
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    clean = [R.speech_like(n, k) for k, n in enumerate(lens)]
    noise = [(0.1 * np.random.default_rng(5000 + k).standard_normal(n)).astype(np.float32) for k, n in enumerate(lens)]
    cp, npool = M.SignalPool(clean, "cuda"), M.SignalPool(noise, "cuda")
    rp = RV.RirPool([reverb_ref.rir_row(K, 80 + k) for k, K in enumerate((4000, 8000, 16000))], "cuda")
    B, n, tries = 64, 64000, 4
    base = {"count": a.count, "audio_s": round(sum(lens) / SR, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed, "batch": B, "samples": n,
            "tries": tries, "gap": 3200}
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
        rec = dict(base, metric="assemble", mode=key, **rec)
        rec.update(reps_per_pass=reps, device_s_per_pass=[round(v, 6) for v in dev], wall_s_per_pass=[round(v, 6) for v in wall],
                   utt_per_s=round(count / w, 1), utt_per_s_device=round(count / d, 1))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return d, w

    counter = [0]

    def dyn(dm):
        counter[0] += 1
        return dm.batch(counter[0])

    feeds = {"dynamic_plain": M.DynamicMixtures(cp, npool, B, samples=n, seed=a.seed),
             "dynamic_clips": M.DynamicMixtures(cp, npool, B, samples=n, seed=a.seed, clips=True),
             "dynamic_clips_rir": M.DynamicMixtures(cp, npool, B, samples=n, seed=a.seed, clips=True, rir_pool=rp, p_reverb=0.5)}
    for key, dm in feeds.items():
        reps = max(1, a.reps // 10) if key.endswith("rir") else a.reps
        dev, wall, _ = timed(lambda: dyn(dm), reps)
        record(key, {"usable_clean": len(dm.usable[0]) if dm.clips else None}, dev, wall, reps, B)

    clips = ASM.draw_clips(1, a.seed, cp.lengths, B, n, tries, 3200, cp.usable(), "clean")
    dev, wall, out = timed(lambda: ASM.assemble(cp, clips, n, 0.6), a.reps)
    record("assemble", {"pieces": len(clips.member)}, dev, wall, a.reps, B)
    rows_dev, info_dev = out

    x = rows_dev.clone()
    dev, wall, _ = timed(lambda: ASM.activity(x), a.reps)
    record("activity", {}, dev, wall, a.reps, B)

    src = [cp.offsets[m] + s for m, s in zip(clips.member, clips.start)]
    tab = ops.asm_tables(cp.data, src, clips.length, clips.dst, clips.first, clips.count, B, tries, n)

    def kernels():
        r = ops.asm_activity(tab, None, 800, -25.0, 0.13, 0.6)
        return ops.asm_write(tab, r["chosen"])
    dev, wall, _ = timed(kernels, a.reps)
    nbytes = 4 * B * n * (tries + 2)
    d = sorted(dev)[len(dev) // 2]
    record("kernels", {"launches_per_call": 3, "min_bytes_moved": nbytes,
                       "min_bytes_label": "tries candidates read once, the chosen row read and written once",
                       "min_bytes_per_s": round(nbytes / d, 0), "share_of_8TBps": round(nbytes / d / HBM_BYTES_PER_S, 4)}, dev, wall, a.reps, B)

    hb = min(B, a.host_rows)
    cands = clips.candidates()[:hb]
    R.assemble(clean, cands[:1], n, 0.6)                      # numpy's first call stays out of the host's time
    t0 = time.perf_counter()
    want = R.assemble(clean, cands, n, 0.6)
    t_host = time.perf_counter() - t0
    w_asm = sorted(results["assemble"]["wall_s_per_pass"])[a.passes // 2]
    rec = dict(base, metric="assemble", mode="host_assemble_ref_float64", rows=hb, wall_s=round(t_host, 3), utt_per_s=round(hb / t_host, 2),
               rows_equal_device=bool(np.array_equal(rows_dev[:hb].cpu().numpy().view(np.int32), want["rows"].view(np.int32))),
               chosen_equal_device=info_dev["chosen"][:hb].tolist() == want["chosen"], margin=want["margin"],
               speedup_assemble=round((B / w_asm) / (hb / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host_assemble_ref"] = rec

    gate = feeds["dynamic_clips"]
    rejected = torch.zeros((), dtype=torch.int64, device="cuda")
    for k in range(a.gate_batches):
        rejected += B - gate.batch(1000 + k, info=True)[3]["clean_accepted"].sum()
    rec = dict(base, metric="assemble", mode="accepted", clean_activity=0.6, batches=a.gate_batches, rows=a.gate_batches * B,
               rows_not_accepted=int(rejected.item()), share_not_accepted=round(int(rejected.item()) / (a.gate_batches * B), 5),
               pool_activity_mean=round(float(cp.stats()["activity"].mean()), 4))
    print(json.dumps(rec), flush=True)
    results["accepted"] = rec

    bench = importlib.import_module("bench")
    dmb = M.DynamicMixtures(cp, npool, a.train_batch, samples=bench.LEN, seed=a.seed, clips=True)
    dev, _, _ = timed(lambda: dyn(dmb), a.reps)
    d_asm = sorted(dev)[len(dev) // 2]
    step, _, what = bench.build_workload(a.train_workload, a.train_batch, "cuda", 0)
    dev, _, _ = timed(step, a.train_steps)
    d_step = sorted(dev)[len(dev) // 2]
    rec = {"metric": "assemble", "mode": "train_share", "workload": a.train_workload, "precision": "fp32", "batch": a.train_batch,
           "samples": bench.LEN, "what": what["workload"], "clips_batch_device_s": round(d_asm, 6), "step_device_s": round(d_step, 6),
           "clips_share_of_step": round(d_asm / d_step, 5)}
    print(json.dumps(rec), flush=True)
    results["train_share"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
