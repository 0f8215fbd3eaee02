"""Throughput of DNSMOS P.835 scoring of a set of recordings of different lengths (inference.dnsmos_list, csrc/dnsmos.hip), the conv
kernels' share of the fp32 matrix peak per layer, and the deviation from the float64 definition on the fixtures.

    python profiles/tools/measure_dnsmos.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--host-segments 2] [--no-enhance]
                                            [--out profiles/dnsmos/measure.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o dnsmos -- python profiles/tools/measure_dnsmos.py --mode kernels
    python profiles/tools/measure_dnsmos.py --merge-trace DIR/.../dnsmos_kernel_trace.csv [--out ...]

  list (default): ``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz, the signals of tests/dnsmos_ref.py.
      dnsmos_list:   one untimed pass, then ``--passes`` timed ones (HIP events and a host clock ended by a synchronise): utt/s and
                     segments/s (a clip shorter than 9.01 s is continued with itself, so a folder of short clips has several
                     segments per clip).
      first_layer:   the first two layers on one chunk of segments with the 1 -> 128 layer fused into the staging of the 128 -> 64
                     layer (what the library runs) and as a kernel of its own (idv_conv3x3_c1_fwd, then idv_conv3x3_fwd).
      host_float32:  the float32 torch-CPU evaluation of the definition (dnsmos_ref.network_float32) on ``--host-segments``
                     segments with the host threads torch uses here.
      enhance_list:  measure_ragged.py's full-width DCCRN-CL on the same lengths, for the share of an evaluation loop.
      deviation:     max |device - float64| per raw value on the fixtures of tests/golden/dnsmos_expected.npz, both sets of weights.
  kernels: the network on ``--chunk`` segments a few times and nothing else, to be run under a kernel trace of its own.
  --merge-trace: reads that trace; the six conv3x3_kernel launches of a pass are the layers 128->64 (with the first layer), 64->64,
      64->32+pool, 32->32+pool, 32->32+pool, 32->64 in that order; writes per layer the mean time, the FLOP (2 * 9 * Cin * Cout per
      output pixel before pooling, plus 2 * 9 * 128 for the fused first layer) and the fraction of the 157.3 TFLOP/s fp32 matrix peak.
Fails without a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import csv
import functools
import importlib
import json
import os
import random
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
PEAK = 157.3e12
GOLDEN = os.path.join(HERE, "tests", "golden")
# (name, H, W, Cin, Cout, extra FLOP per pixel)
LAYERS = (("c1+128->64", 900, 161, 128, 64, 2 * 9 * 128), ("64->64", 900, 161, 64, 64, 0), ("64->32+pool", 900, 161, 64, 32, 0),
          ("32->32+pool", 450, 80, 32, 32, 0), ("32->32+pool (2)", 225, 40, 32, 32, 0), ("32->64", 112, 20, 32, 64, 0))


def weights(sfx=""):
    return R.load_weights(os.path.join(GOLDEN, f"dnsmos_weights{sfx}.npz"), os.path.join(GOLDEN, f"dnsmos_frontend{sfx}.npz"))


def network_only(D, chunk, reps):
    m = D.DNSMOS(weights())
    feat = m.features(torch.from_numpy(np.stack([R.signal("speechlike", 144160, k) for k in range(chunk)])).cuda())
    raw = torch.empty(chunk, 3, dtype=torch.float32, device="cuda")
    m._network(feat, raw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        m._network(feat, raw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def first_layer(D, chunk, reps):
    """The first two layers through the C ABI: the 1 -> 128 layer inside the staging of the 128 -> 64 layer (what the library runs)
    against the two launches with the 128-channel map in memory."""
    L = importlib.import_module("i-dccrn-vae_amd._lib")
    m = D.DNSMOS(weights())
    pk = m.packs("cuda")
    feat = m.features(torch.from_numpy(np.stack([R.signal("speechlike", 144160, k) for k in range(chunk)])).cuda())
    wp, bias = pk.conv[0][:2]
    y = torch.empty(chunk, 900, 161, 64, device="cuda")
    mid = torch.empty(chunk, 900, 161, 128, device="cuda")
    st = L.stream_ptr()
    dims = (L.i(chunk), L.i(900), L.i(161))

    def fused():
        L.call("idv_conv3x3_c1_fused_fwd", L.p(feat), L.p(pk.w1), L.p(pk.b1), L.i(128), L.p(wp), L.p(bias), *dims, L.i(64), L.i(0), L.p(y), st)

    def separate():
        L.call("idv_conv3x3_c1_fwd", L.p(feat), L.p(pk.w1), L.p(pk.b1), *dims, L.i(128), L.p(mid), st)
        L.call("idv_conv3x3_fwd", L.p(mid), L.p(wp), L.p(bias), *dims, L.i(128), L.i(64), L.i(0), L.p(y), st)

    out = {"segments": chunk}
    for name, fn in (("fused", fused), ("separate", separate)):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(e0.elapsed_time(e1) * 1e3 / reps, 1)
    out["separate_over_fused"] = round(out["separate_us"] / out["fused_us"], 3)
    return out


def merge_trace(path, chunk):
    rows = [r for r in csv.DictReader(open(path)) if "conv3x3_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if not rows or len(rows) % len(LAYERS):
        raise SystemExit(f"{path}: {len(rows)} conv3x3_kernel launches are no whole number of passes")
    passes = len(rows) // len(LAYERS)
    out = {}
    for k, (name, H, W, ci, co, extra) in enumerate(LAYERS):
        t = [(int(rows[q * len(LAYERS) + k]["End_Timestamp"]) - int(rows[q * len(LAYERS) + k]["Start_Timestamp"])) / 1e3
             for q in range(1 if passes > 1 else 0, passes)]               # the first pass carries the code-object load
        us = sum(t) / len(t)
        flop = chunk * H * W * (2 * 9 * ci * co + extra)
        out[name] = {"us_mean": round(us, 1), "us_min": round(min(t), 1), "calls": len(t), "gflop": round(flop / 1e9, 2),
                     "tflops": round(flop / us / 1e6, 1), "fraction_of_fp32_matrix_peak": round(flop / (us * 1e-6) / PEAK, 3)}
    return {"segments": chunk, "peak_tflops": PEAK / 1e12, "layers": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("list", "kernels"), default="list")
    ap.add_argument("--merge-trace", default=None)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--host-segments", type=int, default=2)
    ap.add_argument("--no-enhance", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dnsmos", "measure.json"))
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
        raise SystemExit("measure_dnsmos.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    D = importlib.import_module("i-dccrn-vae_amd.dnsmos")
    if a.mode == "kernels":
        print(json.dumps({"mode": "kernels", "segments": a.chunk, "s_per_pass": network_only(D, a.chunk, 4)}), flush=True)
        return

    import measure_ragged as MR
    inf = importlib.import_module("i-dccrn-vae_amd.inference")
    model = D.DNSMOS(weights())
    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    sigs = [torch.from_numpy(R.signal(("speechlike", "tone", "noise")[k % 3], n, k)).cuda() for k, n in enumerate(lens)]
    nseg = sum(D.plan_segments(lens)[1])
    base = {"count": a.count, "audio_s": round(sum(lens) / SR, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed, "segments": nseg}

    dev, wall = MR.timed(lambda: inf.dnsmos_list(sigs, model), a.passes)
    w = sorted(wall)[len(wall) // 2]
    res["dnsmos_list"] = dict(base, metric="dnsmos", mode="dnsmos_list", device_s_per_pass=[round(v, 4) for v in dev],
                              wall_s_per_pass=[round(v, 4) for v in wall], utt_per_s=round(a.count / w, 1),
                              segments_per_s=round(nseg / w, 1), tflops_conv=round(nseg * 38.8e9 / w / 1e12, 1))
    print(json.dumps(res["dnsmos_list"]), flush=True)

    res["first_layer"] = first_layer(D, a.chunk, 4)
    print(json.dumps(res["first_layer"]), flush=True)

    t = weights()
    seg = R.signal("speechlike", 144160)
    R.network_float32(seg, t)
    t0 = time.perf_counter()
    for k in range(a.host_segments):
        R.network_float32(R.signal("speechlike", 144160, k), t)
    th = (time.perf_counter() - t0) / max(1, a.host_segments)
    res["host_float32"] = {"segments": a.host_segments, "threads": torch.get_num_threads(), "s_per_segment": round(th, 3),
                           "segments_per_s": round(1 / th, 2), "speedup_of_dnsmos_list": round((nseg / w) * th, 1)}
    print(json.dumps(res["host_float32"]), flush=True)

    exp = np.load(os.path.join(GOLDEN, "dnsmos_expected.npz"))
    res["deviation"] = {}
    for sfx in ("", "_personalized"):
        m = D.DNSMOS(weights(sfx), personalized=bool(sfx))
        kinds = (("tone", 144160), ("speechlike", 176000))
        x = torch.full((2, 176000), float("nan"), device="cuda")
        for b, (k, n) in enumerate(kinds):
            x[b, :n] = torch.from_numpy(R.signal(k, n)).cuda()
        raw = m.score(x, [n for _, n in kinds], per_segment=True)["segments_raw"].cpu().numpy().astype(np.float64)
        want = np.concatenate([exp[f"{k}{sfx}.raw64"] for k, _ in kinds])
        floor = max(np.abs(exp[f"{k}{sfx}.raw32"] - exp[f"{k}{sfx}.raw64"]).max() for k, _ in kinds)
        res["deviation"]["weights" + sfx] = {"float32_host_max_abs": float(f"{floor:.3g}"), "bound": float(f"{4 * floor:.3g}"),
                                             "device_max_abs": float(f"{np.abs(raw - want).max():.3g}")}
    print(json.dumps(res["deviation"]), flush=True)

    if not a.no_enhance:
        enh, _ = MR.build(HERE)
        dev, wall = MR.timed(lambda: inf.enhance_list(functools.partial(inf.enhance_supervised, enh), sigs, MR.HOP), a.passes)
        we = sorted(wall)[len(wall) // 2]
        res["enhance_list"] = dict(base, metric="ragged_enhance", mode="list", wall_s_per_pass=[round(v, 4) for v in wall],
                                   utt_per_s=round(a.count / we, 1))
        res["share"] = {"dnsmos_over_enhance": round(w / we, 2)}
        print(json.dumps(res["enhance_list"]), flush=True)
        print(json.dumps(res["share"]), flush=True)
    save()


if __name__ == "__main__":
    main()
