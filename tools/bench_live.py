#!/usr/bin/env python3
"""What live utterances cost: 64 concurrent streams of gated audio, 10 ms hops, host memory to host memory.

    python tools/bench_live.py [--streams 64] [--hops 1500] [--warmup 200] [--repeats 3] [--out profiles/live_bench.json]

One process, the paths alternating hop by hop so that clocks and the machine's other tenants hit them alike:

    (a) push_host_unarmed / push_host_armed   kws_stream_push_host_i16 on a plain context and on one armed with
                                              kws_stream_utt_open: p50 of the host wall time per hop; push_host_unarmed_b is a
                                              second plain context: what two contexts differ by with nothing armed
    (b) step_kernel                           kws_stream_utt_step_i16 (hop + energies) enqueued back to back, events around the
                                              batch: the step kernel's own time, launch gap included
    (c) close_to_utterances                   from "the step that closed U utterances has landed" to logits, labels and peaks in
                                              host memory, U = 1 and U = all streams: cut, classification and read, by events
    (d) host_route                            the same job the way it had to be done before: kws_stream_vad_f32 after every push
                                              (which turns the zero-copy path off), the PCM kept in NumPy, start point +
                                              normalize + fix_length in NumPy, infer_pcm16's upload and classification

Every figure is reported per repeat, with the spread across repeats beside the median."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "keyword-spotting_amd"))
import bench
from kws import _native

DEV = torch.device("cuda", 0)
STEP, FRAME_LEN, LAG, THR = 160, 400, 3, -10.0
ON, OFF, PRE_ROLL, MAX_FRAMES, SLACK = 40, 80, 60, 1000, 8


def gated_audio(S, hops, seed=0):
    """int16 [hops, S, 160]: one second of noise, one second of silence, every stream with its own phase."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-12000, 12001, (hops, S, STEP)).astype(np.int16)
    t = np.arange(hops)[:, None] + 17 * np.arange(S)[None, :]
    x[(t // 100) % 2 == 1] = 0
    return x


def open_ctx(S, armed, torch_stream=False):
    ctx = _native.Context(0)
    if torch_stream:
        ctx.use_torch_stream()
    ctx.load_dscnn(bench.bench_weights()[0], 12)
    ctx.stream_open(S)
    if armed:
        H = _native.host_stream_utt_history(FRAME_LEN, STEP, PRE_ROLL, MAX_FRAMES, SLACK)
        ctx.stream_utt_open(THR, ON, OFF, PRE_ROLL, MAX_FRAMES, H, max(S, 64))
    return ctx


def med_spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def per_hop(S, audio, warmup, hops):
    """(a) and the per-hop part of (d): p50 per path, paths alternating hop by hop."""
    plain, armed, plain_b, vad = open_ctx(S, False), open_ctx(S, True), open_ctx(S, False), open_ctx(S, False, torch_stream=True)
    hop_buf = torch.zeros((S, STEP), dtype=torch.int16, device=DEV)
    lg = torch.zeros((S, 12), dtype=torch.float32, device=DEV)
    lb = torch.zeros((S,), dtype=torch.int32, device=DEV)
    state = torch.zeros((S,), dtype=torch.int32, device=DEV)
    kept = np.zeros((S, (PRE_ROLL + MAX_FRAMES + LAG) * STEP), np.int16)  # the host route keeps every stream's PCM itself

    def host_route(h):
        nonlocal kept
        kept = np.concatenate([kept[:, STEP:], h], axis=1)
        hop_buf.copy_(torch.from_numpy(h))
        vad.stream_push_i16(hop_buf, lg, lb)
        vad.stream_vad_f32(THR, ON, OFF, state)
        torch.cuda.synchronize()
        return lb.cpu().numpy(), lg.cpu().numpy(), state.cpu().numpy()

    paths = {"push_host_unarmed": lambda h: plain.stream_push_host_i16(h, S), "push_host_armed": lambda h: armed.stream_push_host_i16(h, S),
             "push_host_unarmed_b": lambda h: plain_b.stream_push_host_i16(h, S), "host_route_push_vad": host_route}
    lat = {k: [] for k in paths}
    events = 0
    order = list(paths.items())
    for t in range(warmup + hops):
        h = np.ascontiguousarray(audio[t % len(audio)])
        # the order rotates hop by hop: whichever path follows the slow host route starts on a colder machine
        for name, fn in order[t % 4:] + order[:t % 4]:
            t0 = time.perf_counter()
            res = fn(h)
            _ = (res[0].copy(), res[1].copy())
            dt = (time.perf_counter() - t0) * 1e6
            if t >= warmup:
                lat[name].append(dt)
    events = armed.stream_utt_poll()[0]
    for c in (plain, armed, plain_b, vad):
        c.stream_close(); c.close()
    return {k: float(np.percentile(v, 50)) for k, v in lat.items()}, int(events)


def step_kernel(S, audio, n=400):
    """(b): n explicit steps back to back between two events."""
    ctx = open_ctx(S, True, torch_stream=True)
    hops = torch.from_numpy(np.ascontiguousarray(audio[:64])).to(DEV)
    energy = torch.full((S,), THR - 1.0, dtype=torch.float32, device=DEV)
    for t in range(50):
        ctx.stream_utt_step_i16(hops[t % 64], energy)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for t in range(n):
        ctx.stream_utt_step_i16(hops[t % 64], energy)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / n
    ctx.stream_close(); ctx.close()
    return us


def close_to_utterances(S, U, audio):
    """(c): drive U streams through one utterance with explicit steps so that all U close at one step, then time the parts."""
    ctx = open_ctx(S, True, torch_stream=True)
    hops = torch.from_numpy(np.ascontiguousarray(audio[:64])).to(DEV)
    loud = torch.full((S,), THR - 1.0, dtype=torch.float32, device=DEV)
    loud[:U] = THR + 1.0
    quiet = torch.full((S,), THR - 1.0, dtype=torch.float32, device=DEV)
    t = 0
    for _ in range(LAG - 1):
        ctx.stream_utt_step_i16(hops[t % 64], None); t += 1
    for e, n in ((loud, 60), (quiet, 73)):  # 73 unvoiced frames: more than 90 % of the last 80
        for _ in range(n):
            ctx.stream_utt_step_i16(hops[t % 64], e); t += 1
    t0 = time.perf_counter()
    total, _ = ctx.stream_utt_poll()
    assert total == U, (total, U)
    rec = ctx.stream_utt_read(0, U)
    clips = torch.empty((U, 16000), dtype=torch.int16, device=DEV)
    out = torch.empty((U * 14,), dtype=torch.float32, device=DEV)
    lg, ints = out[:U * 12].view(U, 12), out[U * 12:].view(torch.int32)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    ctx.stream_utt_cut_i16(0, clips, 16384, ints[U:])
    ev[1].record()
    ctx.infer_i16(clips, lg, ints[:U])
    ev[2].record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host = out.cpu()
    t2 = time.perf_counter()
    assert rec.shape == (U, 6) and host.shape[0] == U * 14
    ctx.stream_close(); ctx.close()
    return {"cut_us": ev[0].elapsed_time(ev[1]) * 1e3, "classify_us": ev[1].elapsed_time(ev[2]) * 1e3, "read_us": (t2 - t1) * 1e6,
            "total_us": (t2 - t0) * 1e6}


def host_close(S, U, spotter):
    """The close of (d): start point, normalize and fix_length in NumPy over the kept PCM, then infer_pcm16."""
    rng = np.random.default_rng(1)
    kept = rng.integers(-12000, 12001, (S, (PRE_ROLL + MAX_FRAMES + LAG) * STEP)).astype(np.int16)
    t0 = time.perf_counter()
    clips = []
    for s in range(U):
        x = kept[s, -(PRE_ROLL + 140) * STEP - FRAME_LEN:].astype(np.float64)
        x = np.trunc(x * (16384.0 / np.abs(x).max())).astype(np.int16)
        clips.append(np.pad(x, (0, max(0, 16000 - len(x))))[:16000])
    labels, logits = spotter.infer_pcm16(np.stack(clips))
    assert labels.shape == (U,)
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--hops", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_bench.json"))
    a = ap.parse_args()
    S = a.streams
    from kws.inference import KeywordSpotter

    spotter = KeywordSpotter()  # (d)'s classification: any weights time alike
    spotter.infer_pcm16(np.zeros((S, 16000), np.int16))  # the ingest pipeline's first use allocates
    audio = gated_audio(S, 400)
    runs = {"push_host_unarmed_p50_us": [], "push_host_armed_p50_us": [], "push_host_unarmed_b_p50_us": [], "host_route_push_vad_p50_us": [],
            "step_kernel_us": []}
    closes = {f"close_to_utterances_U{U}": {k: [] for k in ("cut_us", "classify_us", "read_us", "total_us")} for U in (1, S)}
    host_closes = {f"host_route_close_U{U}_us": [] for U in (1, S)}
    events = 0
    for _ in range(a.repeats):
        p50, events = per_hop(S, audio, a.warmup, a.hops)
        runs["push_host_unarmed_p50_us"].append(p50["push_host_unarmed"])
        runs["push_host_armed_p50_us"].append(p50["push_host_armed"])
        runs["push_host_unarmed_b_p50_us"].append(p50["push_host_unarmed_b"])
        runs["host_route_push_vad_p50_us"].append(p50["host_route_push_vad"])
        runs["step_kernel_us"].append(step_kernel(S, audio))
        for U in (1, S):
            close_to_utterances(S, U, audio)  # once unmeasured: first-use allocations of the classification
            r = close_to_utterances(S, U, audio)
            for k, v in r.items():
                closes[f"close_to_utterances_U{U}"][k].append(v)
            host_close(S, U, spotter)
            host_closes[f"host_route_close_U{U}_us"].append(host_close(S, U, spotter))
    out = {"config": f"{S} concurrent streams of gated audio, 10 ms hops, windows {ON} / {OFF}, pre-roll {PRE_ROLL}, time-out {MAX_FRAMES} frames; "
                     f"{a.hops} timed hops after {a.warmup}, paths alternating hop by hop in one process, {a.repeats} repeats",
           "utterances_closed_on_the_armed_context_per_repeat": events,
           **{k: {**med_spread(v), "runs": v} for k, v in runs.items()},
           **{k: {p: med_spread(v) for p, v in parts.items()} for k, parts in closes.items()},
           **{k: {**med_spread(v), "runs": v} for k, v in host_closes.items()}}
    out["arming_adds_p50_us"] = out["push_host_armed_p50_us"]["median"] - out["push_host_unarmed_p50_us"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
