"""Throughput of the image-source room simulator on the device (dataset/rir.py, csrc/ism.hip) against its float64 numpy definition
on one host thread, and the cost of a training batch that draws from such a pool.

    python profiles/tools/measure_ism.py [--rooms 256] [--seed 0] [--passes 3] [--host-rooms 0] [--out profiles/ism/measure.json]

``--rooms`` rooms of ``draw_rooms(0, seed, rooms)`` at ``taps = round(t60 fs)``, fs = 16000.
  pool:     ``RirPool.shoebox`` on the whole set, one launch: one untimed pass first, then ``--passes`` timed ones (HIP events around
            the pass and a host clock ended by a synchronise; the upload of the room records, the packing of the rows and the
            download of the peaks are part of the pass).  images: the sum of the images every tile owns, from the kernel's work
            buffer (the image set of the definition, exactly).  lane_pairs: 64 times the images summed into every tile, the (sample,
            image) pairs the lanes went through; pairs_nominal: 81 per image, the pairs of the definition for an image whose window
            lies inside the response.
  kernel:   ``shoebox_rir`` alone on the same rooms (no packing, no peaks).
  host:     tests/ism_ref.rir in float64, one process, one thread, on the first ``--host-rooms`` rooms (0: all), with the images
            of those rooms from the same device counts.
  dynamic_p50 / dynamic_dry:  ``DynamicMixtures.batch(k)`` at B = 64 x 64000 with that pool at p_reverb = 0.5, fresh k each time,
            and without a pool.
One JSON line per mode on stdout; ``--out`` writes them into one JSON file keyed by mode.  Fails without a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")               # the host comparator runs on one thread

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ism_ref as R  # noqa: E402
import measure_ragged as MR  # noqa: E402

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-rooms", type=int, default=0)
    ap.add_argument("--noise-s", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_ism.py measures on the GPU; there is nothing to report without one")
    torch.set_num_threads(1)
    M = importlib.import_module("i-dccrn-vae_amd.dataset.mix")
    RV = importlib.import_module("i-dccrn-vae_amd.dataset.reverb")
    RI = importlib.import_module("i-dccrn-vae_amd.dataset.rir")
    OPS = importlib.import_module("i-dccrn-vae_amd.ops")
    rooms = RI.draw_rooms(0, a.seed, a.rooms)
    taps = [int(round(t * SR)) for t in rooms.t60]
    args = (rooms.room, rooms.source, rooms.mic, rooms.beta, taps)
    base = {"rooms": a.rooms, "seed": a.seed, "taps": [min(taps), max(taps)], "response_s": round(sum(taps) / SR, 1)}
    results = {}

    geom, tp, _ = RI.check_rooms(*args)
    _, counts = OPS.ism_rir(torch.from_numpy(geom).cuda(), torch.tensor(tp, dtype=torch.int32).cuda(), None, a.rooms, max(tp))
    counts = counts.cpu().numpy()
    per_room = counts[:, :, 1].sum(axis=1)
    images, summed = int(per_room.sum()), int(counts[:, :, 0].sum())

    def record(key, rec, dev, wall):
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, images=images, device_s_per_pass=[round(v, 6) for v in dev], wall_s_per_pass=[round(v, 6) for v in wall],
                   rooms_per_s=round(a.rooms / w, 1), rooms_per_s_device=round(a.rooms / d, 1), images_per_s_device=round(images / d),
                   lane_pairs_per_s_device=round(64 * summed / d), pairs_nominal_per_s_device=round(81 * images / d))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return d, w

    keep = []
    dev, wall = MR.timed(lambda: keep.append(RV.RirPool.shoebox(*args)), a.passes)
    pool = keep[-1]
    _, w_pool = record("pool", {"metric": "ism", "mode": "pool"}, dev, wall)
    keep.clear()
    dev, wall = MR.timed(lambda: keep.append(RI.shoebox_rir(*args)), a.passes)
    first = keep[-1][:4].cpu().numpy()
    record("kernel", {"metric": "ism", "mode": "kernel"}, dev, wall)
    keep.clear()

    n_host = a.rooms if a.host_rooms <= 0 else min(a.rooms, a.host_rooms)
    R.rir(rooms.room[0], rooms.source[0], rooms.mic[0], rooms.beta[0], 256)                              # the first call stays out of the time
    t0 = time.perf_counter()
    want = [R.rir(rooms.room[b], rooms.source[b], rooms.mic[b], rooms.beta[b], taps[b]) for b in range(n_host)]
    t_host = time.perf_counter() - t0
    host_images = int(per_room[:n_host].sum())
    diff = max(float(np.abs(first[b, :taps[b]] - want[b]).max() / np.abs(want[b]).max()) for b in range(min(4, n_host)))
    rec = dict(base, metric="ism", mode="host_numpy_float64", host_rooms=n_host, images=host_images, wall_s=round(t_host, 3),
               rooms_per_s=round(n_host / t_host, 3), images_per_s=round(host_images / t_host),
               worst_difference_over_peak_first_rows=diff,
               speedup_pool_by_images=round((images / w_pool) / (host_images / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host"] = rec

    rng = np.random.default_rng(a.seed)
    host_x = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in np.linspace(1 * SR, 10 * SR, 64).astype(int)]
    host_v = [(0.1 * rng.standard_normal(int(a.noise_s * SR))).astype(np.float32) for _ in range(64)]
    cp, npool = M.SignalPool(host_x, "cuda"), M.SignalPool(host_v, "cuda")
    counter = [0]

    def dyn(dm):
        counter[0] += 1
        return dm.batch(counter[0])
    for key, kw in (("dynamic_dry", {}), ("dynamic_p50", dict(rir_pool=pool, p_reverb=0.5))):
        dm = M.DynamicMixtures(cp, npool, 64, samples=64000, seed=a.seed, **kw)
        dev, wall = MR.timed(lambda: dyn(dm), a.passes)
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec = dict(base, metric="ism", mode=key, batch=64, samples=64000, p_reverb=kw.get("p_reverb"),
                   device_s_per_pass=[round(v, 6) for v in dev], wall_s_per_pass=[round(v, 6) for v in wall],
                   batches_per_s=round(1 / w, 2))
        print(json.dumps(rec), flush=True)
        results[key] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
