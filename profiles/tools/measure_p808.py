"""What the P808_MOS column costs (dnsmos.P808, csrc/p808.hip): inference.dnsmos_list with and without ``p808=`` on the recordings of
measure_dnsmos.py, the throughput of P808 alone, the deviation from the float64 definition on the fixtures, and a kernel trace.

    python profiles/tools/measure_p808.py [--count 256] [--min-s 1] [--max-s 10] [--passes 5] [--out profiles/p808/measure.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o p808 -- python profiles/tools/measure_p808.py --mode kernels
    python profiles/tools/measure_p808.py --merge-trace DIR/.../p808_kernel_trace.csv [--out ...]

  list (default): ``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz, the signals of tests/dnsmos_ref.py.
      dnsmos_list:  one untimed pass of each form, then ``--passes`` timed pairs (without, with, alternating, so that a drift of the
                    clocks meets both alike); the medians and their quotient.
      p808_alone:   P808.score on the same recordings in batches of 64: segments/s.
      deviation:    max |device - float64| per segment on the fixtures of tests/golden/p808_expected.npz.
  kernels: P808 on ``--chunk`` segments three times and nothing else, to be run under a kernel trace of its own.
  --merge-trace: reads that trace; per kernel of a pass (the first pass, which carries the code-object load, left out) the mean time.
Fails without a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import random
import re
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dnsmos_ref as R  # noqa: E402

SR = 16000
GOLDEN = os.path.join(HERE, "tests", "golden")
PASSES_TRACED = 3


def merge_trace(path, chunk):
    rows = [r for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    mine = [r for r in rows if any(s in r["Kernel_Name"] for s in ("p808_", "conv3x3_", "gmax_kernel")) and "pack" not in r["Kernel_Name"]]
    if not mine or len(mine) % PASSES_TRACED:
        raise SystemExit(f"{path}: {len(mine)} launches are no whole number of {PASSES_TRACED} passes")
    per = len(mine) // PASSES_TRACED
    out, total = [], 0.0
    for k in range(per):
        t = [(int(mine[q * per + k]["End_Timestamp"]) - int(mine[q * per + k]["Start_Timestamp"])) / 1e3 for q in range(1, PASSES_TRACED)]
        name = re.search(r"(\w+_kernel(?:<[^>]*>)?)", mine[per + k]["Kernel_Name"]).group(1)
        out.append({"kernel": name, "us_mean": round(sum(t) / len(t), 1)})
        total += sum(t) / len(t)
    return {"segments": chunk, "launches_per_pass": per, "us_per_pass": round(total, 1), "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("list", "kernels"), default="list")
    ap.add_argument("--merge-trace", default=None)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "p808", "measure.json"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    if a.merge_trace:
        res["kernels"] = merge_trace(a.merge_trace, a.chunk)
        print(json.dumps(res["kernels"]), flush=True)
        return save()
    if not torch.cuda.is_available():
        raise SystemExit("measure_p808.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    D = importlib.import_module("i-dccrn-vae_amd.dnsmos")
    p808 = D.P808.from_npz(os.path.join(GOLDEN, "p808_weights.npz"))
    if a.mode == "kernels":
        segs = torch.from_numpy(np.stack([R.signal("speechlike", 144160, k) for k in range(a.chunk)])).cuda()
        for _ in range(PASSES_TRACED):
            p808.raw(segs)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "kernels", "segments": a.chunk}), flush=True)
        return

    import measure_ragged as MR
    inf = importlib.import_module("i-dccrn-vae_amd.inference")
    model = D.DNSMOS(R.load_weights(os.path.join(GOLDEN, "dnsmos_weights.npz"), os.path.join(GOLDEN, "dnsmos_frontend.npz")))
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    sigs = [torch.from_numpy(R.signal(("speechlike", "tone", "noise")[k % 3], n, k)).cuda() for k, n in enumerate(lens)]
    nseg = sum(D.plan_segments(lens)[1])
    base = {"count": a.count, "audio_s": round(sum(lens) / SR, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed, "segments": nseg}

    forms = {"without": lambda: inf.dnsmos_list(sigs, model), "with_p808": lambda: inf.dnsmos_list(sigs, model, p808=p808)}
    wall = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.passes):
        for k, fn in forms.items():
            _, w = MR.timed(fn, 1)
            wall[k] += w
    med = {k: sorted(v)[len(v) // 2] for k, v in wall.items()}
    res["dnsmos_list"] = dict(base, wall_s_per_pass={k: [round(x, 4) for x in v] for k, v in wall.items()},
                              median_s={k: round(v, 4) for k, v in med.items()},
                              with_over_without=round(med["with_p808"] / med["without"], 3),
                              utt_per_s={k: round(a.count / v, 1) for k, v in med.items()})
    print(json.dumps(res["dnsmos_list"]), flush=True)

    def alone():
        order = sorted(range(a.count), key=lambda k: -lens[k])
        for b0 in range(0, a.count, 64):
            batch = order[b0:b0 + 64]
            x = torch.zeros(len(batch), lens[batch[0]], device="cuda")
            for r, k in enumerate(batch):
                x[r, :lens[k]] = sigs[k]
            p808.score(x, [lens[k] for k in batch])
    _, w = MR.timed(alone, a.passes)
    wa = sorted(w)[len(w) // 2]
    res["p808_alone"] = dict(base, wall_s_per_pass=[round(x, 4) for x in w], segments_per_s=round(nseg / wa, 1),
                             utt_per_s=round(a.count / wa, 1))
    print(json.dumps(res["p808_alone"]), flush=True)

    exp = np.load(os.path.join(GOLDEN, "p808_expected.npz"))
    kinds = (("tone", 144160), ("speechlike", 176000))
    x = torch.full((2, 176000), float("nan"), device="cuda")
    for b, (k, n) in enumerate(kinds):
        x[b, :n] = torch.from_numpy(R.signal(k, n)).cuda()
    raw = p808.score(x, [n for _, n in kinds], per_segment=True)["segments_p808"].cpu().numpy().astype(np.float64)
    want = np.concatenate([exp[f"{k}.raw64"] for k, _ in kinds])
    floor = max(np.abs(exp[f"{k}.raw32"] - exp[f"{k}.raw64"]).max() for k, _ in kinds)
    res["deviation"] = {"float32_host_max_abs": float(f"{floor:.3g}"), "bound": float(f"{4 * floor:.3g}"),
                        "device_max_abs": float(f"{np.abs(raw - want).max():.3g}")}
    print(json.dumps(res["deviation"]), flush=True)
    res["when"] = time.strftime("%Y-%m-%d")
    save()


if __name__ == "__main__":
    main()
