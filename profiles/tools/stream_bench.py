"""Streaming enhancement benchmark: one JSON line per batch of lock-step streams, one hop (100 samples) per push.

    python profiles/tools/stream_bench.py [--batches 1,16,128,512,1024] [--seconds 2] [--catchup] [--far-seconds 3600] [--sessions]
                                           [--conv valu|mfma|bf16x3|both|mfma-bf16x3] [--vae [--sessions]]
                                           [--two-latents [--sessions] [--outtype O] [--phase P]]
                                           [--state]

Per line: device time per push (HIP events around >= --seconds of pushes after warm-up), host wall time per push (synchronised),
the real-time factor (hop / 16 kHz = 6.25 ms over the wall time) and the algorithmic GFLOP per push (4 real products per complex
product of every block at its kept positions, LSTM and dense, the DFTs), computed from the shapes.  --catchup adds one line of
4000-sample pushes at B = 64 in utterances (4 s) per second.  --far-seconds S adds one line at B = 1 measured after S seconds of
audio went through the streamer in 1 s pushes, with no flush: time per push must not depend on the stream's position.  --conv names the engine
of the conv blocks (streaming.check_conv); "both" measures the two fp32 engines in turn, twice, in one process per batch size, so
that they share the card and its clocks (field "round"), and "mfma-bf16x3" does the same for the fp32 MFMA and the split-bf16
engine (field "conv_engines_bf16x3": the blocks on the split-bf16 entries).  --sessions measures streaming.StreamingSessions
instead (metric "sessions_push"): every slot active, slot b 13 * (b % 7) samples ahead of slot 0, so the slots stand at staggered
positions and each hop push still completes one frame per slot; counts are passed as a host list on every push.  The
streams are never flushed; pushes are column slices of a 4 s signal taken round-robin (no copy).  Full-width DCCRN-CL,
synthetic weights.  --vae measures streaming.StreamingVAE instead (metric "vae_push"): the full-width NSVAE encoder (zdim 128,
latent_num 2: LSTM hidden 768) and fine-tuned decoder with num_samples 3, default batches 1,16,128; each line adds the device
time of the wide LSTM entry alone at the push's shape (events around repeated calls of idv_stream_clstm_wide on the streamer's
own buffers, after the push measurements) and its share of the device time of a push.  --vae --sessions measures
streaming.StreamingVAESessions (metric "vae_sessions_push": every slot active at the staggered positions of --sessions, counts as a
host list on every push) and, right after it in the same process and with the same models, the lock-step StreamingVAE at the same
B and engine (metric "vae_push"), so that the two lines of a pair share the card and its clocks.  --two-latents measures
streaming.StreamingVAETwoLatents (metric "two_latents_push"; --outtype, default phase_mask, and --phase, default 2; the encoder of
--vae, a speech and a noise decoder, num_samples 3, default batches 1,16) and, right after it in the same process with the same
encoder and speech decoder, StreamingVAE at the same B, ns and engine (metric "vae_push").  --two-latents --sessions measures
streaming.StreamingVAETwoLatentsSessions (metric "two_latents_sessions_push": every slot active at the staggered positions of
--sessions, counts as a host list on every push) and, right after it in the same process with the same three models, the lock-step
StreamingVAETwoLatents at the same B and engine (metric "two_latents_push").  --state measures save + load of streaming.StreamingSessions
(metric "state_save_load", default batches 16,256): after the hop pushes of --sessions (reported in the same line) the states of
1 slot and of all slots are saved and loaded back into their own slots (overwrite=True, so the streams go on as they were), with
the states left on the device and taken through the host (.cpu() of every state, then load from the CPU states); device time from
events around the repetitions, wall time synchronised after every save + load.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NFFT, HOP, WIN, SR = 512, 100, 400, 16000
PAIRS = {"both": ("valu", "mfma"), "mfma-bf16x3": ("mfma", "bf16x3")}      # --conv values that measure two engines in turn


def gflop_per_frame(st) -> float:
    macs = 0
    for cp in st.enc + st.dec:
        pos = cp.Fin if cp.transposed else cp.Fout
        macs += 4 * (cp.C0 + cp.C1) * cp.Cout * 10 * pos
    H, K = st.H, st.K
    macs += 2 * 8 * H * K + 4 * 3 * 4 * H * H       # layer-0 projection (2 parts x 2 sets), W_hh0 / W_ih1 / W_hh1 per run
    macs += 2 * H * st.dense_out[0] * st.dense_out[1]
    macs += 2 * st.F * WIN * 2                      # DFT and inverse DFT
    return 2 * macs / 1e9


def gflop_per_frame_vae(st) -> float:
    """Per stream: the encoder blocks, LSTM projection and recurrence once, the dense layer and decoder blocks ns times."""
    conv = lambda cp: 4 * (cp.C0 + cp.C1) * cp.Cout * 10 * (cp.Fin if cp.transposed else cp.Fout)
    H, K = st.H, st.K
    macs = sum(conv(cp) for cp in st.enc) + 2 * 8 * H * K + 4 * 3 * 4 * H * H + 2 * st.F * WIN
    macs += st.ns * (sum(conv(cp) for cp in st.dec) + 2 * st.zdim * st.dense_out[0] * st.dense_out[1] + 2 * st.F * WIN)
    return 2 * macs / 1e9


def gflop_per_frame_two(st) -> float:
    """gflop_per_frame_vae with every decoder chain ns times and, for the mask estimators, one inverse DFT per stream."""
    conv = lambda cp: 4 * (cp.C0 + cp.C1) * cp.Cout * 10 * (cp.Fin if cp.transposed else cp.Fout)
    H, K = st.H, st.K
    macs = sum(conv(cp) for cp in st.enc) + 2 * 8 * H * K + 4 * 3 * 4 * H * H + 2 * st.F * WIN
    macs += st.ns * sum(sum(conv(cp) for cp in ch.dec) + 2 * st.zdim * st.dense_out[0] * st.dense_out[1] for ch in st.chains)
    macs += (st.ns if st.noise is None else 1) * 2 * st.F * WIN
    return 2 * macs / 1e9


def wide_lstm_ms(st, k=1, reps=200) -> float:
    """Device time of idv_stream_clstm_wide alone for k steps at the streamer's batch (it advances the streamer's LSTM state)."""
    L = importlib.import_module("i-dccrn-vae_amd._lib")
    ops = importlib.import_module("i-dccrn-vae_amd.ops")
    Tp = k + 1
    Jp = ops.Planar.jp_for(st.B, Tp)
    args = (L.p(st.G), L.p(st.lstm_wt), L.p(st.lstm_b1), L.p(st.lstm_state), L.p(st.hstep), st.lat.ptr(), L.i(st.H), L.i(st.B), L.i(k),
            L.i(Tp), L.i(Jp), L.stream_ptr())
    for _ in range(10):
        L.call("idv_stream_clstm_wide", *args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        L.call("idv_stream_clstm_wide", *args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


_VAE_PAIR = []


def build(B, sessions=False, conv="valu", vae=False, two=None):
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    S = importlib.import_module("i-dccrn-vae_amd.streaming")
    from oracle import idccrn_oracle as O
    np_ = O.net_params(True, 32)
    if vae:
        if not _VAE_PAIR:                       # one pair for every streamer of the process
            load = lambda m, seed: m.load_state_dict(O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
            enc = pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cuda", 128, NFFT, HOP, WIN, 3, 2)
            dec = pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", 3, 128, NFFT, HOP, WIN, "mask", True, [0, 1, 2, 3, 4, 5], False)
            noise = pm.nsvae_pvae_dccrn_decoder_twophase(np_, True, "cuda", 3, 128, NFFT, HOP, WIN, "mask", True, [0, 1, 2, 3, 4, 5], False)
            load(enc, 9)
            load(dec, 10)
            load(noise, 11)
            _VAE_PAIR.extend([enc.cuda(), dec.cuda(), noise.cuda()])
        enc, dec, noise = _VAE_PAIR
        if two is not None and sessions:
            return S.StreamingVAETwoLatentsSessions(enc, dec, noise, slots=B, outtype=two[0], phase=two[1], seed=0, conv=conv)
        if two is not None:
            return S.StreamingVAETwoLatents(enc, dec, noise, batch=B, outtype=two[0], phase=two[1], seed=0, conv=conv)
        if sessions:
            return S.StreamingVAESessions(enc, dec, slots=B, seed=0, conv=conv)
        return S.StreamingVAE(enc, dec, batch=B, seed=0, conv=conv)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cuda", WIN, [0, 1, 2, 3, 4, 5], "mask", False, None, None)
    m.load_state_dict(O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 7))
    m = m.cuda()
    return S.StreamingSessions(m, slots=B, conv=conv) if sessions else S.StreamingDCCRN(m, batch=B, conv=conv)


def run(B, seconds, n=HOP, far_seconds=0, sessions=False, conv="valu", vae=False, two=None):
    st = build(B, sessions, conv, vae, two)
    x = torch.randn(B, 64000, device="cuda") * 0.1
    pos = 0
    if sessions:                                # stagger the slots: slot b starts 13 * (b % 7) samples ahead
        st.push(x[:, :13 * 6], counts=[13 * (b % 7) for b in range(B)])
    counts = [n] * B

    def push(m=n):
        nonlocal pos
        assert x.shape[1] % m == 0
        xs = x[:, pos % x.shape[1]:pos % x.shape[1] + m]
        y = st.push(xs, counts)[0] if sessions else st.push(xs)
        pos += m
        return y

    for _ in range(far_seconds):               # 1 s pushes, no flush
        push(SR)
    torch.cuda.synchronize()
    for _ in range(10):
        push()
    torch.cuda.synchronize()
    # host wall time, synchronised after every push
    t_end = time.perf_counter() + seconds
    walls = []
    while time.perf_counter() < t_end or len(walls) < 20:
        t0 = time.perf_counter()
        push()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    # device time: events around a run of pushes
    reps = max(20, len(walls))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        push()
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / reps
    wall_ms = 1e3 * sorted(walls)[len(walls) // 2]
    return st, dev_ms, wall_ms, pos


def state_round_trips(st, reps_dev=20, reps_host=5):
    """save + load of 1 and of all slots of a sessions object back into their own slots -> one dict per (slots, via)."""
    out = []
    for slots in ([0], list(range(st.B))):
        for via in ("device", "host"):
            def once():
                states = st.save(slots)
                if via == "host":
                    states = [s.cpu() for s in states]
                st.load(slots, states, overwrite=True)
                return states
            states = once()
            once()
            torch.cuda.synchronize()
            reps = reps_dev if via == "device" else reps_host
            walls = []
            for _ in range(reps):
                t0 = time.perf_counter()
                once()
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                once()
            e1.record()
            torch.cuda.synchronize()
            out.append({"slots_moved": len(slots), "via": via, "floats_per_slot": int(states[0].data.numel()),
                        "device_ms_per_save_load": round(e0.elapsed_time(e1) / reps, 4),
                        "wall_ms_per_save_load": round(1e3 * sorted(walls)[len(walls) // 2], 4), "reps": reps})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default=None)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--catchup", action="store_true")
    ap.add_argument("--far-seconds", type=int, default=0)
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--conv", choices=["valu", "mfma", "bf16x3", "both", "mfma-bf16x3"], default="valu")
    ap.add_argument("--vae", action="store_true")
    ap.add_argument("--two-latents", action="store_true")
    ap.add_argument("--outtype", default="phase_mask")
    ap.add_argument("--phase", type=int, default=2)
    ap.add_argument("--state", action="store_true")
    a = ap.parse_args()
    if a.state and (a.vae or a.two_latents or a.catchup or a.far_seconds or a.conv in PAIRS):
        ap.error("--state measures save + load of StreamingSessions next to its hop pushes only")
    if a.state and a.batches is None:
        a.batches = "16,256"
    if a.two_latents and (a.catchup or a.far_seconds):
        ap.error("--two-latents measures hop pushes of StreamingVAETwoLatents / StreamingVAETwoLatentsSessions and StreamingVAE only")
    a.vae = a.vae or a.two_latents
    if a.vae and (a.catchup or a.far_seconds):
        ap.error("--vae measures hop pushes of StreamingVAE / StreamingVAESessions only")
    if a.batches is None:
        a.batches = "1,16" if a.two_latents else "1,16,128" if a.vae else "1,16,128,512,1024"
    torch.set_grad_enabled(False)
    budget = 1e3 * HOP / SR
    turns = [(c, rnd) for rnd in (0, 1) for c in PAIRS[a.conv]] if a.conv in PAIRS else [(a.conv, 0)]
    conv1 = PAIRS[a.conv][1] if a.conv in PAIRS else a.conv   # the single-engine lines below
    for B in [int(v) for v in a.batches.split(",") if v]:
        for conv, rnd in turns:
            if a.state:
                st, dev_ms, wall_ms, _ = run(B, a.seconds, sessions=True, conv=conv)
                for line in state_round_trips(st):
                    print(json.dumps({"metric": "state_save_load", "B": B, **line, "push_device_ms": round(dev_ms, 4),
                                      "push_wall_ms": round(wall_ms, 4), "conv": conv}), flush=True)
                del st
                torch.cuda.empty_cache()
                continue
            if a.two_latents:
                two_ = (a.outtype, a.phase)
                # (estimator or None: StreamingVAE, sessions form): the sessions form first, then its lock-step form
                for two, sessions in (((two_, True), (two_, False)) if a.sessions else ((two_, False), (None, False))):
                    st, dev_ms, wall_ms, _ = run(B, a.seconds, sessions=sessions, conv=conv, vae=True, two=two)
                    gf = (gflop_per_frame_two(st) if two else gflop_per_frame_vae(st)) * B
                    metric = "two_latents_sessions_push" if sessions else "two_latents_push" if two else "vae_push"
                    line = {"metric": metric, "B": B, "ns": st.ns, "H": st.H, "hop": HOP}
                    if two:
                        line.update({"outtype": st.outtype, "phase": st.phase})
                    line.update({"device_ms_per_push": round(dev_ms, 4), "wall_ms_per_push": round(wall_ms, 4),
                                 "rtf": round(budget / wall_ms, 3), "device_rtf": round(budget / dev_ms, 3),
                                 "under_hop_budget": bool(wall_ms < budget), "gflop_per_push": round(gf, 3),
                                 "tflops_device": round(gf / dev_ms, 2), "frames_per_launch": st.cap, "conv": conv,
                                 "conv_engines": st.conv_engines.count("mfma"),
                                 "conv_engines_bf16x3": st.conv_engines.count("bf16x3"), "round": rnd})
                    print(json.dumps(line), flush=True)
                    del st
                    torch.cuda.empty_cache()
                continue
            if a.vae:
                for sessions in ([True, False] if a.sessions else [False]):
                    st, dev_ms, wall_ms, _ = run(B, a.seconds, sessions=sessions, conv=conv, vae=True)
                    gf = gflop_per_frame_vae(st) * B
                    line = {"metric": "vae_sessions_push" if sessions else "vae_push", "B": B, "ns": st.ns, "H": st.H, "hop": HOP,
                            "device_ms_per_push": round(dev_ms, 4), "wall_ms_per_push": round(wall_ms, 4),
                            "rtf": round(budget / wall_ms, 3), "device_rtf": round(budget / dev_ms, 3),
                            "under_hop_budget": bool(wall_ms < budget)}
                    if not sessions:
                        lstm_ms = wide_lstm_ms(st)
                        line.update({"wide_lstm_device_ms": round(lstm_ms, 4), "wide_lstm_share": round(lstm_ms / dev_ms, 3)})
                    line.update({"gflop_per_push": round(gf, 3), "tflops_device": round(gf / dev_ms, 2), "frames_per_launch": st.cap,
                                 "conv": conv, "conv_engines": st.conv_engines.count("mfma"),
                                 "conv_engines_bf16x3": st.conv_engines.count("bf16x3"), "round": rnd})
                    print(json.dumps(line), flush=True)
                    del st
                    torch.cuda.empty_cache()
                continue
            st, dev_ms, wall_ms, _ = run(B, a.seconds, sessions=a.sessions, conv=conv)
            gf = gflop_per_frame(st) * B
            print(json.dumps({"metric": "sessions_push" if a.sessions else "stream_push", "B": B, "hop": HOP,
                              "device_ms_per_push": round(dev_ms, 4),
                              "wall_ms_per_push": round(wall_ms, 4), "rtf": round(budget / wall_ms, 3),
                              "device_rtf": round(budget / dev_ms, 3), "gflop_per_push": round(gf, 3),
                              "tflops_device": round(gf / dev_ms, 2), "frames_per_launch": st.cap, "conv": conv,
                              "conv_engines": st.conv_engines.count("mfma"),
                              "conv_engines_bf16x3": st.conv_engines.count("bf16x3"), "round": rnd}), flush=True)
            del st
            torch.cuda.empty_cache()
    if a.catchup:
        B, n = 64, 4000
        st, dev_ms, wall_ms, _ = run(B, a.seconds, n, conv=conv1)
        utt = B * n / (4 * SR)                      # 4 s utterances per push
        print(json.dumps({"metric": "stream_catchup", "B": B, "samples_per_push": n, "wall_ms_per_push": round(wall_ms, 3),
                          "device_ms_per_push": round(dev_ms, 3), "utt_per_s": round(utt / (wall_ms / 1e3), 1),
                          "offline_utt_per_s": 901, "conv": conv1}), flush=True)
    if a.far_seconds:
        st, dev_ms, wall_ms, pos = run(1, a.seconds, HOP, a.far_seconds, conv=conv1)
        print(json.dumps({"metric": "stream_push_far", "B": 1, "hop": HOP, "position_s": round(pos / SR, 1),
                          "device_ms_per_push": round(dev_ms, 4), "wall_ms_per_push": round(wall_ms, 4),
                          "rtf": round(budget / wall_ms, 3), "conv": conv1}), flush=True)


if __name__ == "__main__":
    main()
