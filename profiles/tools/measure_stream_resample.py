"""What streaming at the caller's sample rate costs: hop pushes through streaming.AtRate / SessionsAtRate around a full-width
StreamingDCCRN / StreamingSessions, against the bare streamer measured in the same run, and the two resampler stages alone.

    python profiles/tools/measure_stream_resample.py [--batches 1,16,256] [--sessions-slots 256] [--rounds 5] [--reps 40]
                                                     [--out profiles/stream_resample/measure.json]

Per batch size B and rate (48 kHz: 300 samples in and 300 out per push; 44.1 kHz: 276 in, 276 on average out), after 20 untimed
pushes, ``--rounds`` rounds of ``--reps`` pushes each:
  device ms per push   HIP events around the round's pushes;
  wall ms per push     a host clock around each push, ended by a synchronise; the round's median.
The bare streamer (hop pushes of 100 samples at 16 kHz), the wrapped streamer and the two resampler stages alone (a
StreamingResampler of each direction fed what the wrapper feeds it) take turns inside every round, so that they share the card
and its clocks.  Reported per quantity: the median over the rounds and the spread [min, max]; ``resampler_share``: the two stages'
device time over the bare push's; ``rtf``: the push's audio time at fs over the wrapped push's wall time.  The sessions form
(every slot active, staggered by 13 * (b % 7) samples as stream_bench.py --sessions staggers them) is reported the same way at
``--sessions-slots`` slots.  One JSON line per measurement on stdout; ``--out`` writes them into one JSON file.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NFFT, HOP, WIN, SR = 512, 100, 400, 16000
PUSH = {48000: 300, 44100: 276}                 # samples per push at fs: one hop of the 16 kHz network (44.1 kHz: 100.14 samples)


def model():
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    from oracle import idccrn_oracle as O
    np_ = O.net_params(True, 32)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, [0, 1, 2, 3, 4, 5], "mask", False, None, None)
    m.load_state_dict(O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 7))
    return m.cuda()


class Pusher:
    """Round-robin column slices of a 4 s signal into ``fn`` (no copy), n samples per push."""

    def __init__(self, fn, B, n, length):
        self.fn, self.n, self.pos = fn, n, 0
        self.x = torch.randn(B, length - length % n, device="cuda") * 0.1

    def __call__(self):
        lo = self.pos % self.x.shape[1]
        self.pos += self.n
        return self.fn(self.x[:, lo:lo + self.n])


def measure(pushers, rounds, reps):
    """{name: pusher} -> {name: {"device_ms": [median, min, max], "wall_ms": [...]}}; the pushers take turns inside every round."""
    for pu in pushers.values():
        for _ in range(20):
            pu()
    torch.cuda.synchronize()
    dev = {k: [] for k in pushers}
    wall = {k: [] for k in pushers}
    for _ in range(rounds):
        for k, pu in pushers.items():
            walls = []
            for _ in range(reps):
                t0 = time.perf_counter()
                pu()
                torch.cuda.synchronize()
                walls.append(1e3 * (time.perf_counter() - t0))
            wall[k].append(statistics.median(walls))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                pu()
            e1.record()
            torch.cuda.synchronize()
            dev[k].append(e0.elapsed_time(e1) / reps)
    spread = lambda v: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]
    return {k: {"device_ms": spread(dev[k]), "wall_ms": spread(wall[k])} for k in pushers}


def report(metric, B, fs, n, res, extra=None):
    bare, wrapped = res["bare"], res["wrapped"]
    stages = res["down"]["device_ms"][0] + res["up"]["device_ms"][0]
    line = {"metric": metric, "B": B, "fs": fs, "samples_per_push": n, "bare": bare, "wrapped": wrapped, "down_stage": res["down"],
            "up_stage": res["up"], "stages_device_ms": round(stages, 4), "resampler_share": round(stages / bare["device_ms"][0], 4),
            "added_device_ms": round(wrapped["device_ms"][0] - bare["device_ms"][0], 4),
            "added_wall_ms": round(wrapped["wall_ms"][0] - bare["wall_ms"][0], 4),
            "rtf": round(1e3 * n / fs / wrapped["wall_ms"][0], 3)}
    line.update(extra or {})
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--sessions-slots", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_stream_resample.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    S = importlib.import_module("i-dccrn-vae_amd.streaming")
    m = model()
    lines = []
    for B in [int(v) for v in a.batches.split(",") if v]:
        for fs, n in PUSH.items():
            inner = S.StreamingDCCRN(m, batch=B)
            st = S.AtRate(S.StreamingDCCRN(m, batch=B), fs)
            down, up = S.StreamingResampler(fs, SR, B), S.StreamingResampler(SR, fs, B)
            res = measure({"bare": Pusher(inner.push, B, HOP, 4 * SR), "wrapped": Pusher(st.push, B, n, 4 * fs),
                           "down": Pusher(down.push, B, n, 4 * fs), "up": Pusher(up.push, B, HOP, 4 * SR)}, a.rounds, a.reps)
            lines.append(report("at_rate_push", B, fs, n, res, {"H_down": down.plan.H, "H_up": up.plan.H}))
            del inner, st
            torch.cuda.empty_cache()
    B = a.sessions_slots
    if B > 0:
        ahead = [13 * (b % 7) for b in range(B)]
        for fs, n in PUSH.items():
            scale = lambda v: v * fs // SR
            inner = S.StreamingSessions(m, slots=B)
            st = S.SessionsAtRate(S.StreamingSessions(m, slots=B), fs)
            down, up = S.StreamingResamplerSessions(fs, SR, B), S.StreamingResamplerSessions(SR, fs, B)
            z = lambda w: torch.zeros(B, w, device="cuda")
            inner.push(z(78), counts=ahead)                     # stagger the slots
            up.push(z(78), counts=ahead)
            st.push(z(scale(78)), counts=[scale(v) for v in ahead])
            down.push(z(scale(78)), counts=[scale(v) for v in ahead])
            c16, cfs = [HOP] * B, [n] * B
            res = measure({"bare": Pusher(lambda x: inner.push(x, c16)[0], B, HOP, 4 * SR),
                           "wrapped": Pusher(lambda x: st.push(x, cfs)[0], B, n, 4 * fs),
                           "down": Pusher(lambda x: down.push(x, cfs)[0], B, n, 4 * fs),
                           "up": Pusher(lambda x: up.push(x, c16)[0], B, HOP, 4 * SR)}, a.rounds, a.reps)
            lines.append(report("sessions_at_rate_push", B, fs, n, res))
            del inner, st
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"rounds": a.rounds, "reps_per_round": a.reps, "format": "[median, min, max] over the rounds", "lines": lines},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
