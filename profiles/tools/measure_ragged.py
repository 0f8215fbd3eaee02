"""Throughput of enhancing a set of utterances of different lengths: the B = 1 loop against inference.enhance_list.

    python profiles/tools/measure_ragged.py [--modes loop,list] [--count 256] [--min-s 1] [--max-s 10] [--passes 3]
                                            [--root DIR] [--out profiles/ragged/measure.json]

Full-width DCCRN-CL, fp32, synthetic weights, ``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz.
  loop: ``enhance_supervised(model, x[None])`` one utterance at a time -- all the package offered before ``lengths=`` existed;
        uses nothing newer, so ``--root DIR`` (another checkout of this repository with its library built, e.g. the parent
        commit) measures the baseline a user had.
  list: ``enhance_list(functools.partial(enhance_supervised, model), signals, hop)`` with the default planner.
One untimed pass over the whole set first (every shape builds its DFT plan and warms the allocator), then ``--passes`` timed
passes: HIP events around the pass and a host clock ended by a synchronise.  Both modes keep the default ``check=True`` (one
synchronising ``ops.coop_check()`` per call / per batch), as a user would run them.  One JSON line per mode on stdout; ``--out``
merges the lines into a JSON file keyed by mode (``loop_parent`` when ``--root`` is given).
"""
from __future__ import annotations

import argparse
import functools
import importlib
import json
import os
import random
import sys
import time

import torch

NFFT, HOP, WIN, SR = 512, 100, 400, 16000


def build(root):
    sys.path.insert(0, root)
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    inf = importlib.import_module("i-dccrn-vae_amd.inference")
    from oracle import idccrn_oracle as O
    np_ = O.net_params(True, 32)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, [0, 1, 2, 3, 4, 5], "mask", False, None, None)
    m.load_state_dict(O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 7))
    return m.cuda(), inf


def timed(fn, passes):
    fn()                                            # warm-up: every shape once
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1) / 1e3)
    return dev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="loop,list")
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--root", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.abspath(a.root) if a.root else here
    if not torch.cuda.is_available():
        raise SystemExit("measure_ragged.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    model, inf = build(root)
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    g = torch.Generator().manual_seed(a.seed)
    signals = [(torch.randn(n, generator=g) * 0.1).cuda() for n in lens]
    audio_s = sum(lens) / SR
    results = {}
    for mode in [v for v in a.modes.split(",") if v]:
        rec = {"metric": "ragged_enhance", "mode": mode, "count": a.count, "audio_s": round(audio_s, 1), "precision": "fp32",
               "lengths_s": [a.min_s, a.max_s], "seed": a.seed}
        if mode == "loop":
            fn = lambda: [inf.enhance_supervised(model, s[None]) for s in signals]
            key = "loop_parent" if a.root else "loop"
        elif mode == "list":
            fn = lambda: inf.enhance_list(functools.partial(inf.enhance_supervised, model), signals, HOP)
            batches = inf.plan_ragged_batches(lens, HOP)
            T = [1 + n // HOP for n in lens]
            cols = sum(len(b) * max(T[k] for k in b) for b in batches)
            rec.update(batches=len(batches), batch_sizes=[len(b) for b in batches], padding_share=round(1 - sum(T) / cols, 4))
            key = "list"
        else:
            raise SystemExit(f"unknown mode {mode!r}")
        dev, wall = timed(fn, a.passes)
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(device_s_per_pass=[round(v, 4) for v in dev], wall_s_per_pass=[round(v, 4) for v in wall],
                   utt_per_s=round(a.count / w, 1), audio_s_per_s=round(audio_s / w, 1), utt_per_s_device=round(a.count / d, 1))
        if a.root:
            rec["root"] = os.path.relpath(root, here)
        print(json.dumps(rec), flush=True)
        results[key] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        merged = json.load(open(a.out)) if os.path.exists(a.out) else {}
        merged.update(results)
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
