#!/usr/bin/env python3
"""What live keyword events cost: 64 concurrent streams of gated audio, 10 ms hops, host memory to host memory.

    python tools/bench_live_detect.py [--streams 64] [--hops 1500] [--warmup 200] [--repeats 3] [--out profiles/live_detect_bench.json]

One process, the paths alternating hop by hop so that clocks and the machine's other tenants hit them alike:

    (a) push_host_unarmed / push_host_armed   kws_stream_push_host_i16 on a plain context and on one armed with
                                              kws_stream_detect_open (smooth_window 30): p50 of the host wall time per hop;
                                              push_host_unarmed_b is a second plain context: what two contexts differ by with
                                              nothing armed.  The armed path also polls and reads its events once per hop
                                              (push_host_armed_pop: push + kws_stream_detect_poll + kws_stream_detect_read)
    (b) step_kernel                           kws_stream_detect_step_f32 enqueued back to back, 400 steps between two events: the
                                              step kernel's own stream time per hop, launch gap included, at (S, C, smooth_window)
                                              = (64, 12, 30) and (1024, 12, 256)
    (c) old_way                               the same job the way it had to be done before: StreamingSpotter(smooth_window=30),
                                              whose push includes the smoothing launch, a synchronise and two reads, plus the
                                              threshold and the refractory rule in NumPy

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
STEP, N_CLASSES = 160, 12
SMOOTH, FIRST_KEYWORD, THRESHOLD, REFRACTORY, FIRST_HOP = 30, 2, 0.12, 50, 101


def gated_audio(S, hops, seed=0):
    """int16 [hops, S, 160]: one second of noise, one second of silence, every stream with its own phase."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-12000, 12001, (hops, S, STEP)).astype(np.int16)
    t = np.arange(hops)[:, None] + 17 * np.arange(S)[None, :]
    x[(t // 100) % 2 == 1] = 0
    return x


def open_ctx(S, armed):
    ctx = _native.Context(0)
    ctx.load_dscnn(bench.bench_weights()[0], N_CLASSES)
    ctx.stream_open(S)
    if armed:
        ctx.stream_detect_open(N_CLASSES, SMOOTH, FIRST_KEYWORD, THRESHOLD, REFRACTORY, FIRST_HOP, max(S, 64))
    return ctx


def med_spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def per_hop(S, audio, warmup, hops):
    """(a) and (c): p50 per path, paths alternating hop by hop."""
    from kws.inference import StreamingSpotter
    from kws.libs.models import DepthwiseSeparableConv

    plain, armed, plain_b, armed_pop = open_ctx(S, False), open_ctx(S, True), open_ctx(S, False), open_ctx(S, True)
    old = StreamingSpotter(S, DepthwiseSeparableConv(num_classes=N_CLASSES), smooth_window=SMOOTH)  # any weights time alike
    state = {"seq": 0, "d": 0, "next": np.zeros(S, np.int64), "old_events": 0}
    rows = np.arange(S)

    def push_pop(h):
        res = armed_pop.stream_push_host_i16(h, S)
        total, _ = armed_pop.stream_detect_poll()
        if total > state["seq"]:
            first = max(state["seq"], total - max(S, 64))
            armed_pop.stream_detect_read(first, total - first)
            state["seq"] = total
        return res

    def old_way(h):
        labels, post = old.push(torch.from_numpy(h))  # a device tensor: the route smooth_window leaves
        if state["d"] + 1 >= FIRST_HOP:
            d = state["d"] + 1 - FIRST_HOP
            top = post[rows, labels]
            fire = (labels >= FIRST_KEYWORD) & (top >= THRESHOLD) & (d >= state["next"])
            state["next"][fire] = d + REFRACTORY
            state["old_events"] += len([(int(s), d, int(labels[s]), float(top[s])) for s in np.nonzero(fire)[0]])
        state["d"] += 1
        return post, labels

    paths = {"push_host_unarmed": lambda h: plain.stream_push_host_i16(h, S), "push_host_armed": lambda h: armed.stream_push_host_i16(h, S),
             "push_host_unarmed_b": lambda h: plain_b.stream_push_host_i16(h, S), "push_host_armed_pop": push_pop, "old_way": old_way}
    lat = {k: [] for k in paths}
    order = list(paths.items())
    n = len(order)
    for t in range(warmup + hops):
        h = np.ascontiguousarray(audio[t % len(audio)])
        # the order rotates hop by hop: whichever path follows the slow old way starts on a colder machine
        for name, fn in order[t % n:] + order[:t % n]:
            t0 = time.perf_counter()
            res = fn(h)
            _ = (res[0].copy(), res[1].copy())
            dt = (time.perf_counter() - t0) * 1e6
            if t >= warmup:
                lat[name].append(dt)
    events = armed.stream_detect_poll()[0]
    for c in (plain, armed, plain_b, armed_pop):
        c.stream_close(); c.close()
    old.close()
    return {k: float(np.percentile(v, 50)) for k, v in lat.items()}, int(events), state["old_events"]


def step_kernel(S, C, smooth_window, n=400):
    """(b): n explicit steps back to back between two events, the ring full before the clock starts."""
    ctx = _native.Context(0)
    ctx.use_torch_stream()
    ctx.stream_open(S)
    ctx.stream_detect_open(C, smooth_window, FIRST_KEYWORD, 0.5, REFRACTORY, 0, max(S, 64))
    rng = np.random.default_rng(2)
    z = torch.from_numpy(rng.uniform(-4, 4, (64, S, C)).astype(np.float32)).to(DEV)
    for t in range(smooth_window + 8):
        ctx.stream_detect_step_f32(z[t % 64])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for t in range(n):
        ctx.stream_detect_step_f32(z[t % 64])
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / n
    ctx.stream_close(); ctx.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--hops", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_detect_bench.json"))
    a = ap.parse_args()
    S = a.streams
    audio = gated_audio(S, 400)
    shapes = ((S, N_CLASSES, SMOOTH), (1024, N_CLASSES, 256))
    runs = {"push_host_unarmed_p50_us": [], "push_host_armed_p50_us": [], "push_host_unarmed_b_p50_us": [], "push_host_armed_pop_p50_us": [],
            "old_way_p50_us": [], **{f"step_kernel_S{s}_C{c}_W{w}_us": [] for s, c, w in shapes}}
    events = old_events = 0
    for _ in range(a.repeats):
        p50, events, old_events = per_hop(S, audio, a.warmup, a.hops)
        for k in ("push_host_unarmed", "push_host_armed", "push_host_unarmed_b", "push_host_armed_pop", "old_way"):
            runs[f"{k}_p50_us"].append(p50[k])
        for s, c, w in shapes:
            runs[f"step_kernel_S{s}_C{c}_W{w}_us"].append(step_kernel(s, c, w))
    out = {"config": f"{S} concurrent streams of gated audio, 10 ms hops, smooth_window {SMOOTH}, threshold {THRESHOLD}, refractory {REFRACTORY}, "
                     f"first_hop {FIRST_HOP}; {a.hops} timed hops after {a.warmup}, paths alternating hop by hop in one process, {a.repeats} repeats",
           "events_on_the_armed_context_per_repeat": events, "events_the_old_way_per_repeat": old_events,
           **{k: {**med_spread(v), "runs": v} for k, v in runs.items()}}
    med = lambda k: out[k]["median"]
    out["arming_adds_p50_us"] = med("push_host_armed_p50_us") - med("push_host_unarmed_p50_us")
    out["two_plain_contexts_differ_by_p50_us"] = med("push_host_unarmed_b_p50_us") - med("push_host_unarmed_p50_us")
    out["old_way_over_armed_pop"] = med("old_way_p50_us") / med("push_host_armed_pop_p50_us")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
