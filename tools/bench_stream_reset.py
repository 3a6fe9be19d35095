#!/usr/bin/env python3
"""What resetting single streams of a live set costs: 64 concurrent streams, 10 ms hops, plain and armed (utterances + events).

    python tools/bench_stream_reset.py [--streams 64] [--hops 1500] [--warmup 200] [--repeats 3] [--out profiles/stream_reset_bench.json]
                                       [--never-reset LABEL=live.json,live_detect.json ...]

    (a) reset_host / reset_device   kws_stream_reset of 1, 8 and 64 streams: p50 of the host wall time of the call (it returns
                                    when its launches are enqueued), and the stream time per call of 200 calls back to back
                                    between two events, launch gaps included
    (b) push_host_p50               kws_stream_push_host_i16, host memory to host memory, on a set that resets one stream every
                                    100 hops against a set that never does, the two alternating hop by hop in one process
    (c) close_open_rearm            what a caller had to do before: kws_stream_close + kws_stream_open + re-arming, host wall
                                    time up to a drained stream -- and every other stream's state is gone with it

--never-reset embeds, per label, the figures of tools/bench_live.py and tools/bench_live_detect.py runs (their JSON outputs) that
say what a set that is never reset pays: the armed pushes' p50 and the armed step kernels' times.  Give the runs of the parent
commit and of this tree, taken alternately in one session; the tool states whether each of the tree's medians lies inside the
interval of the parent's runs (or below both: these are times).

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
STEP, FRAME_LEN, N_CLASSES, THR = 160, 400, 12, -10.0
ON, OFF, PRE_ROLL, MAX_FRAMES, SLACK = 40, 80, 60, 1000, 8
SMOOTH, FIRST_KEYWORD, THRESHOLD, REFRACTORY, FIRST_HOP = 30, 2, 0.12, 50, 101
RESET_EVERY = 100
NEVER_RESET_KEYS = {"live": ["push_host_armed_p50_us", "step_kernel_us"],
                    "live_detect": ["push_host_armed_p50_us", "push_host_armed_pop_p50_us", "step_kernel_S64_C12_W30_us",
                                    "step_kernel_S1024_C12_W256_us"]}


def gated_audio(S, hops, seed=0):
    """int16 [hops, S, 160]: one second of noise, one second of silence, every stream with its own phase."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-12000, 12001, (hops, S, STEP)).astype(np.int16)
    t = np.arange(hops)[:, None] + 17 * np.arange(S)[None, :]
    x[(t // 100) % 2 == 1] = 0
    return x


def arm(ctx, S):
    history = _native.host_stream_utt_history(FRAME_LEN, STEP, PRE_ROLL, MAX_FRAMES, SLACK)
    ctx.stream_utt_open(THR, ON, OFF, PRE_ROLL, MAX_FRAMES, history, max(S, 64))
    ctx.stream_detect_open(N_CLASSES, SMOOTH, FIRST_KEYWORD, THRESHOLD, REFRACTORY, FIRST_HOP, max(S, 64))


def open_ctx(S, armed, torch_stream=False):
    ctx = _native.Context(0)
    if torch_stream:
        ctx.use_torch_stream()
    ctx.load_dscnn(bench.bench_weights()[0], N_CLASSES)
    ctx.stream_open(S)
    if armed:
        arm(ctx, S)
    return ctx


def med_spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": [float(x) for x in v]}


def reset_cost(S, armed, audio, counts, calls=200):
    """(a): {n: (host p50 us, device us per call)} on a set that has heard 150 hops."""
    ctx = open_ctx(S, armed, torch_stream=True)
    hop = torch.from_numpy(audio).to(DEV)
    lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    for t in range(150):
        ctx.stream_push_i16(hop[t % len(hop)], lg, None)
    out = {}
    for n in counts:
        idx = np.arange(n, dtype=np.int32) * (S // n)
        ctx.stream_reset(idx)  # the set's first reset makes the silence row; not timed
        ctx.sync()
        host = []
        for _ in range(calls):
            t0 = time.perf_counter()
            ctx.stream_reset(idx)
            host.append((time.perf_counter() - t0) * 1e6)
            ctx.sync()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            ctx.stream_reset(idx)
        b.record()
        torch.cuda.synchronize()
        out[n] = (float(np.percentile(host, 50)), a.elapsed_time(b) * 1e3 / calls)
    ctx.stream_close(); ctx.close()
    return out


def push_with_resets(S, armed, audio, warmup, hops):
    """(b): p50 of the host-to-host push, a set that resets one stream every RESET_EVERY hops beside one that never does."""
    never, resets = open_ctx(S, armed), open_ctx(S, armed)
    state = {"t": 0}

    def push_reset(h):
        if state["t"] % RESET_EVERY == 0:
            resets.stream_reset([(state["t"] // RESET_EVERY) % S])
        state["t"] += 1
        return resets.stream_push_host_i16(h, S)

    order = [("never_reset", lambda h: never.stream_push_host_i16(h, S)), ("reset_every_100_hops", push_reset)]
    lat = {k: [] for k, _ in order}
    for t in range(warmup + hops):
        h = np.ascontiguousarray(audio[t % len(audio)])
        for name, fn in order[t % 2:] + order[:t % 2]:
            t0 = time.perf_counter()
            res = fn(h)
            _ = (res[0].copy(), res[1].copy())
            dt = (time.perf_counter() - t0) * 1e6
            if t >= warmup:
                lat[name].append(dt)
    for c in (never, resets):
        c.stream_close(); c.close()
    return {k: float(np.percentile(v, 50)) for k, v in lat.items()}


def close_open_rearm(S, armed, n=20):
    """(c): host wall time of kws_stream_close + kws_stream_open (+ re-arming) up to a drained stream, p50 of n."""
    ctx = open_ctx(S, armed)
    took = []
    for _ in range(n):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.stream_close()
        ctx.stream_open(S)
        if armed:
            arm(ctx, S)
        ctx.sync()
        took.append((time.perf_counter() - t0) * 1e6)
    ctx.stream_close(); ctx.close()
    return float(np.percentile(took, 50))


def never_reset_section(specs):
    """{label: figures} of the named bench_live / bench_live_detect outputs, and the verdict on the label 'tree'."""
    runs, repeats = {}, {}
    for spec in specs:
        label, paths = spec.split("=", 1)
        live, detect = (json.load(open(p)) for p in paths.split(","))
        repeats[label] = {**{f"live.{k}": live[k]["runs"] for k in NEVER_RESET_KEYS["live"]},
                          **{f"live_detect.{k}": detect[k]["runs"] for k in NEVER_RESET_KEYS["live_detect"]}}
        runs[label] = {**{f"live.{k}": live[k]["median"] for k in NEVER_RESET_KEYS["live"]},
                       **{f"live_detect.{k}": detect[k]["median"] for k in NEVER_RESET_KEYS["live_detect"]}}
    out = {"runs": runs, "repeats": repeats}
    parents = [v for k, v in runs.items() if k.startswith("parent")]
    if "tree" in runs and len(parents) >= 2:
        verdict = {}
        for key, got in runs["tree"].items():
            lo, hi = min(p[key] for p in parents), max(p[key] for p in parents)
            verdict[key] = {"parent_min": lo, "parent_max": hi, "tree": got, "within_parent_interval": bool(lo <= got <= hi),
                            "below_both_parent_runs": bool(got < lo)}
        out["tree_against_parent"] = verdict
        out["condition"] = "every figure (a time: lower is better) of the tree lies inside the interval of the two parent runs, or below both"
        out["condition_met"] = bool(all(v["within_parent_interval"] or v["below_both_parent_runs"] for v in verdict.values()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--hops", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--never-reset", nargs="*", default=[], metavar="LABEL=live.json,live_detect.json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_reset_bench.json"))
    a = ap.parse_args()
    S = a.streams
    audio = gated_audio(S, 400)
    counts = [n for n in (1, 8, 64) if n <= S]
    out = {"config": f"{S} concurrent streams of gated audio, 10 ms hops; armed = utterances (windows {ON} / {OFF}, pre-roll {PRE_ROLL}) + events "
                     f"(smooth_window {SMOOTH}); {a.hops} timed hops after {a.warmup}, {a.repeats} repeats"}
    for armed in (False, True):
        tag = "armed" if armed else "plain"
        host = {n: [] for n in counts}
        dev = {n: [] for n in counts}
        push = {"never_reset": [], "reset_every_100_hops": []}
        rearm = []
        for _ in range(a.repeats):
            for n, (h, d) in reset_cost(S, armed, audio, counts).items():
                host[n].append(h)
                dev[n].append(d)
            for k, v in push_with_resets(S, armed, audio, a.warmup, a.hops).items():
                push[k].append(v)
            rearm.append(close_open_rearm(S, armed))
        sec = {**{f"reset_{n}_streams_host_p50_us": med_spread(host[n]) for n in counts},
               **{f"reset_{n}_streams_device_us": med_spread(dev[n]) for n in counts},
               **{f"push_host_p50_us_{k}": med_spread(v) for k, v in push.items()},
               "close_open_rearm_p50_us": med_spread(rearm)}
        sec["resets_add_to_push_p50_us"] = sec["push_host_p50_us_reset_every_100_hops"]["median"] - sec["push_host_p50_us_never_reset"]["median"]
        out[tag] = sec
    if a.never_reset:
        out["never_reset_set"] = never_reset_section(a.never_reset)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
