"""Throughput of the latent-space report (latent.py) on a set of utterances of different lengths: the device report against the
encoder pass that produces the latents, and against the reference's way on the same latents.

    python profiles/tools/measure_latent.py [--count 256] [--min-s 1] [--max-s 10] [--passes 3] [--host-count 0]
                                            [--repeat 20] [--out profiles/latent/measure.json]

``--count`` seeded lengths uniform in [--min-s, --max-s] seconds at 16 kHz, noise signals, cut into padded batches by
``inference.plan_ragged_batches``; full-width causal encoders (zdim 128) with seeded weights.
  encode:  the NSVAE noisy encoder (two latents) with ``lengths=`` over all batches;
  report:  on the latents of that pass, per batch ``posterior_stats`` (speech latent), ``pair_distance`` (clean encoder's against the
           noisy encoder's speech posterior), ``MiuMoments.update`` and ``sample_rows`` (40 frames of z_speech and z_noise per
           utterance); at the end ``MiuMoments.summary``, ``silhouette`` and one copy of the per-row values to the host;
  host:    the reference's way on the same latents: per utterance a ``.cpu()`` copy of its valid frames and the float32 formulas of
           tests/latent_ref.py on one thread, the covariance and the silhouette at the end, on the first ``--host-count`` utterances
           of the batch order, longest first (0: all of them).
One untimed pass first, then ``--passes`` timed ones (HIP events around the pass and a host clock ended by a synchronise); a timed
report pass goes over the set ``--repeat`` times, so that the window lasts about half a second, and reports the time of one.  One JSON
line per mode on stdout; ``--out`` writes them into one JSON file keyed by mode.
"""
from __future__ import annotations

import argparse
import importlib
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
import latent_ref as R  # noqa: E402

SR, ZDIM, PER_UTT = 16000, 128, 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=1.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-count", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=20, help="a timed report pass goes over the set this often and reports the time of one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_latent.py measures on the GPU; there is nothing to report without one")
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    sys.path.insert(0, HERE)
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    inf = importlib.import_module("i-dccrn-vae_amd.inference")
    L = importlib.import_module("i-dccrn-vae_amd.latent")
    from oracle import idccrn_oracle as O

    def load(m, seed):
        m.load_state_dict(O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
        return m.cuda()
    np_ = O.net_params(True, 32)
    noisy_enc = load(pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", ZDIM, MR.NFFT, MR.HOP, MR.WIN, 1, 2), 7)
    clean_enc = load(pm.pvae_dccrn_encoder_skip_prepare(np_, True, "cuda", ZDIM, MR.NFFT, MR.HOP, MR.WIN, 1), 8)

    rng = random.Random(a.seed)
    lens = [rng.randint(int(a.min_s * SR), int(a.max_s * SR)) for _ in range(a.count)]
    g = torch.Generator().manual_seed(a.seed)
    signals = [(torch.randn(n, generator=g) * 0.1).cuda() for n in lens]
    plan = inf.plan_ragged_batches(lens, MR.HOP)
    batches = []
    for batch in plan:
        blens = [lens[k] for k in batch]
        padded = torch.zeros(len(batch), max(blens), dtype=torch.float32, device="cuda")
        for row, k in enumerate(batch):
            padded[row, :lens[k]] = signals[k]
        batches.append((padded, blens))
    audio_s = sum(lens) / SR
    base = {"count": a.count, "audio_s": round(audio_s, 1), "lengths_s": [a.min_s, a.max_s], "seed": a.seed, "batches": len(plan),
            "frames": sum(1 + n // MR.HOP for n in lens), "zdim": ZDIM}
    results = {}

    def record(key, rec, dev, wall, n):
        d, w = sorted(dev)[len(dev) // 2], sorted(wall)[len(wall) // 2]
        rec.update(base, device_s_per_pass=[round(v, 4) for v in dev], wall_s_per_pass=[round(v, 4) for v in wall],
                   utt_per_s=round(n / w, 1), utt_per_s_device=round(n / d, 1))
        print(json.dumps(rec), flush=True)
        results[key] = rec
        return w

    noisy, clean = [], []

    def encode():
        noisy.clear()
        for padded, blens in batches:
            o = noisy_enc(padded, train=False, lengths=blens)
            noisy.append(o[:8] + (o[-1],))                   # the skip activations are not kept
    dev, wall = MR.timed(encode, a.passes)
    w_enc = record("encode", {"metric": "latent_report", "mode": "encode"}, dev, wall, a.count)
    for padded, blens in batches:
        o = clean_enc(padded, train=False, lengths=blens)
        clean.append(o[:4] + (o[-1],))
    torch.cuda.synchronize()

    got = {}

    def report():
        acc, sampler = L.MiuMoments(ZDIM, "cuda"), random.Random(a.seed)
        rows, set_s, set_n = [], [], []
        for out_n, out_c in zip(noisy, clean):
            fr = L.frames_of(out_n[-1])
            rows.append((L.posterior_stats(*out_n[1:4], frames=fr), L.pair_distance(out_c[1:4], out_n[1:4], frames=fr)))
            acc.update(out_n[1], fr)
            set_s.append(L.sample_rows(out_n[0], fr, PER_UTT, sampler))
            set_n.append(L.sample_rows(out_n[4], fr, PER_UTT, sampler))
        got["summary"] = acc.summary()
        got["silhouette"] = L.silhouette(torch.cat(set_s), torch.cat(set_n))
        got["rows"] = {k: torch.cat([r[j][k] for r in rows]).cpu() for j in (0, 1) for k in rows[0][j]}
    rep = max(1, a.repeat)
    dev, wall = MR.timed(lambda: [report() for _ in range(rep)], a.passes)
    w_rep = record("report", {"metric": "latent_report", "mode": "report", "repeat": rep}, [v / rep for v in dev], [v / rep for v in wall],
                   a.count)

    n_host = a.count if a.host_count <= 0 else min(a.count, a.host_count)
    order = [k for batch in plan for k in batch]               # utterance of every row, batch by batch
    t0 = time.perf_counter()
    sampler, done = random.Random(a.seed), 0
    mius, set_s, set_n, worst = [], [], [], 0.0
    for (out_n, out_c), batch in zip(zip(noisy, clean), plan):
        for row, k in enumerate(batch):
            if done == n_host:
                break
            n = 1 + lens[k] // MR.HOP
            z_s, miu, ls, dl, z_n = (out_n[j][row, :n].cpu().numpy() for j in (0, 1, 2, 3, 4))
            cm, cl, cd = (out_c[j][row, :n].cpu().numpy() for j in (1, 2, 3))
            st = R.posterior_stats(miu, ls, dl, np.float32)
            R.pair_distance((cm, cl, cd), (miu, ls, dl), np.float32)
            mius.append(miu)
            pick = sampler.sample(range(n), min(PER_UTT, n))
            set_s.append(z_s[pick])
            set_n.append(z_n[pick])
            at = order.index(k)
            worst = max(worst, abs(float(got["rows"]["kl"][at]) - st["kl"]) / abs(st["kl"]))
            done += 1
    cov = R.miu_cov(mius, np.float32)
    R.cov_summary(cov["cov_rr"], cov["cov_ri"], cov["cov_ii"])
    R.silhouette(np.concatenate(set_s), np.concatenate(set_n), np.float32)
    t_host = time.perf_counter() - t0
    rec = dict(base, metric="latent_report", mode="host_float32", utterances=n_host, wall_s=round(t_host, 3),
               utt_per_s=round(n_host / t_host, 2), max_rel_dev_of_device_kl=float(f"{worst:.3g}"),
               speedup_report=round((a.count / w_rep) / (n_host / t_host), 1))
    print(json.dumps(rec), flush=True)
    results["host_float32"] = rec
    rec = dict(base, metric="latent_report", mode="share", report_over_encode=round(w_rep / w_enc, 4), sc=got["silhouette"]["sc"],
               mean_dis=got["summary"]["mean_dis"])
    print(json.dumps(rec), flush=True)
    results["share"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
