#!/usr/bin/env python3
"""What a sparse live set costs: a set sized for its peak (1024 slots) of which only some streams are active, 10 ms hops.

    python tools/bench_stream_active.py [--slots 1024] [--hops 600] [--warmup 100] [--repeats 3] [--out profiles/stream_active_bench.json]
                                        [--never-deactivated LABEL=run.json ...]
    python tools/bench_stream_active.py --dense-only --package-root DIR --out run.json     # a set that never deactivates, any commit

    (a) sparse_cost    1024 slots with 16, 64, 256 and 1024 active beside DENSE sets of 16, 64 and 256 streams, all in one process,
                       the paths alternating hop by hop: p50 of kws_stream_push_host_i16, host memory to host memory, and the push
                       kernel's own duration (the library's event bracket around every 8th launch of a device push).  The
                       yardstick for "sparse costs what its active streams cost" is the dense set of the same count; for the
                       gain, the dense 1024-slot set (= 1024 of 1024 active).
    (b) armed_cost     the same at 64 of 1024 with utterances and events armed, beside the dense armed sets of 64 and 1024.
    (c) transitions    kws_stream_deactivate / kws_stream_activate / kws_stream_reset of 1, 8 and 64 streams of the 1024-slot set:
                       p50 of the call's host wall time and the stream time per call of 100 calls back to back between two events.
    (d) never_deactivated   --dense-only measures a 64-stream set that never deactivates, plain and armed: push p50 host to host,
                       the push kernel's duration, and the stream time per armed push (the two step kernels ride in it).  It uses
                       nothing a commit before this feature lacks, so the same file runs against the parent's package
                       (--package-root).  --never-deactivated embeds such runs; with labels parent*, tree the tool states whether
                       each of the tree's figures lies inside the interval of the parent's runs (or below both: these are times).

Every figure is reported per repeat, with the spread across repeats beside the median."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=1024)
ap.add_argument("--hops", type=int, default=600)
ap.add_argument("--warmup", type=int, default=100)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--dense-only", action="store_true")
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--never-deactivated", nargs="*", default=[], metavar="LABEL=run.json")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.package_root)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "keyword-spotting_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
from kws import _native  # noqa: E402

DEV = torch.device("cuda", 0)
STEP, FRAME_LEN, N_CLASSES, THR = 160, 400, 12, -10.0
ON, OFF, PRE_ROLL, MAX_FRAMES, SLACK = 40, 80, 60, 1000, 8
SMOOTH, FIRST_KEYWORD, THRESHOLD, REFRACTORY, FIRST_HOP = 30, 2, 0.12, 50, 101
K_DSCNN = 1  # KWS_K_DSCNN


def gated_audio(S, hops, seed=0):
    """int16 [hops, S, 160]: one second of noise, one second of silence, every stream with its own phase."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-12000, 12001, (hops, S, STEP)).astype(np.int16)
    t = np.arange(hops)[:, None] + 17 * np.arange(S)[None, :]
    x[(t // 100) % 2 == 1] = 0
    return x


def open_ctx(S, armed, active=None, torch_stream=False):
    """A set of S streams; active: how many stay active (spread evenly over the slots), None = never deactivated."""
    ctx = _native.Context(0)
    if torch_stream:
        ctx.use_torch_stream()
    ctx.load_dscnn(bench.bench_weights()[0], N_CLASSES)
    ctx.stream_open(S)
    if armed:
        history = _native.host_stream_utt_history(FRAME_LEN, STEP, PRE_ROLL, MAX_FRAMES, SLACK)
        ctx.stream_utt_open(THR, ON, OFF, PRE_ROLL, MAX_FRAMES, history, max(S, 64))
        ctx.stream_detect_open(N_CLASSES, SMOOTH, FIRST_KEYWORD, THRESHOLD, REFRACTORY, FIRST_HOP, max(S, 64))
    if active is not None and active < S:
        keep = set((np.arange(active) * S // active).tolist())
        ctx.stream_deactivate([s for s in range(S) if s not in keep])
    return ctx


def med_spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": [float(x) for x in v]}


def alternating_p50(sets, audio, warmup, hops):
    """sets: {name: (ctx, S)} -> {name: p50 us of kws_stream_push_host_i16 with the results copied out}, the sets taking turns
    hop by hop and the order rotating.  A push returns behind its kernel's flag, ahead of the armed steps; the stream is drained
    after every timed push, so no set's figure holds another set's steps (they are in stream_us_per_push)."""
    order = list(sets.items())
    hop_of = {name: [np.ascontiguousarray(audio[t % len(audio), :S]) for t in range(len(audio))] for name, (_, S) in order}
    lat = {name: [] for name in sets}
    for t in range(warmup + hops):
        r = t % len(order)
        for name, (ctx, S) in order[r:] + order[:r]:
            h = hop_of[name][t % len(audio)]
            t0 = time.perf_counter()
            res = ctx.stream_push_host_i16(h, S)
            _ = (res[0].copy(), res[1].copy())
            dt = (time.perf_counter() - t0) * 1e6
            if t >= warmup:
                lat[name].append(dt)
            ctx.sync()  # untimed: the armed steps behind this push are done before the next set's push starts
    return {name: float(np.percentile(v, 50)) for name, v in lat.items()}


def kernel_us(ctx, S, audio, pushes=160):
    """The push kernel's own duration: device pushes with the library's event bracket around every 8th launch."""
    hop = torch.from_numpy(np.ascontiguousarray(audio[:8, :S])).to(DEV)
    lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.prof_enable(8)
    ctx.prof_reset()
    for t in range(pushes):
        ctx.stream_push_i16(hop[t % 8], lg, None)
    ctx.sync()
    ms, n = ctx.prof_read(K_DSCNN)
    ctx.prof_enable(False)
    return ms * 1e3 / max(n, 1)


def stream_us_per_push(ctx, S, audio, pushes=200):
    """Stream time per push, launches back to back between two events: the push kernel and whatever steps behind it."""
    hop = torch.from_numpy(np.ascontiguousarray(audio[:8, :S])).to(DEV)
    lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for t in range(pushes):
        ctx.stream_push_i16(hop[t % 8], lg, None)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / pushes


def cost_section(slots, armed, actives, denses, audio, a):
    """(a) / (b): per set the push p50 and the kernel's duration, `a.repeats` times."""
    names = [f"sparse_{k}_of_{slots}" if k < slots else f"dense_{slots}" for k in actives] + [f"dense_{k}" for k in denses]
    p50 = {n: [] for n in names}
    kern = {n: [] for n in names}
    strm = {n: [] for n in names}
    for _ in range(a.repeats):
        sets = {}
        for k in actives:
            sets[f"sparse_{k}_of_{slots}" if k < slots else f"dense_{slots}"] = (open_ctx(slots, armed, k, torch_stream=True), slots)
        for k in denses:
            sets[f"dense_{k}"] = (open_ctx(k, armed, torch_stream=True), k)
        for name, v in alternating_p50(sets, audio, a.warmup, a.hops).items():
            p50[name].append(v)
        for name, (ctx, S) in sets.items():
            kern[name].append(kernel_us(ctx, S, audio))
            strm[name].append(stream_us_per_push(ctx, S, audio))
            ctx.stream_close(); ctx.close()
    return {n: {"push_host_p50_us": med_spread(p50[n]), "push_kernel_us": med_spread(kern[n]), "stream_us_per_push": med_spread(strm[n])}
            for n in names}


def transitions(slots, audio, counts, calls=100):
    """(c): {entry: {n: (host p50 us, stream us per call)}} on a plain set that has heard 150 hops."""
    ctx = open_ctx(slots, False, torch_stream=True)
    hop = torch.from_numpy(np.ascontiguousarray(audio[:8])).to(DEV)
    lg = torch.zeros((slots, N_CLASSES), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    for t in range(150):
        ctx.stream_push_i16(hop[t % 8], lg, None)
    out = {"deactivate": {}, "activate": {}, "reset": {}}
    for n in counts:
        idx = np.arange(n, dtype=np.int32) * (slots // n)
        ctx.stream_reset(idx)       # the set's first reset makes the silence row, its first deactivation the list: not timed
        ctx.stream_deactivate(idx)
        ctx.stream_activate(idx)
        ctx.sync()
        host = {k: [] for k in out}
        for _ in range(calls):
            for k, fn in (("deactivate", ctx.stream_deactivate), ("activate", ctx.stream_activate), ("reset", ctx.stream_reset)):
                t0 = time.perf_counter()
                fn(idx)
                host[k].append((time.perf_counter() - t0) * 1e6)
                ctx.sync()
        dev = {}
        for k, body in (("pair", lambda: (ctx.stream_deactivate(idx), ctx.stream_activate(idx))), ("activate", lambda: ctx.stream_activate(idx)),
                        ("reset", lambda: ctx.stream_reset(idx))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                body()
            b.record()
            torch.cuda.synchronize()
            dev[k] = a.elapsed_time(b) * 1e3 / calls
        # stream time: a deactivation changes something only on an active stream, so it is timed as the pair deactivate + activate
        # (two list rebuilds and the reset); "activate" here names streams that are active, which is a plain reset
        for k in out:
            out[k][n] = (float(np.percentile(host[k], 50)), dev["pair" if k == "deactivate" else k])
    ctx.stream_close(); ctx.close()
    return out


def dense_only(a):
    """(d): a 64-stream set that never deactivates, plain and armed."""
    S = 64
    audio = gated_audio(S, 400)
    fig = {k: [] for k in ("plain.push_host_p50_us", "armed.push_host_p50_us", "plain.push_kernel_us", "armed.push_kernel_us", "armed.stream_us_per_push",
                           "plain.stream_us_per_push")}
    for _ in range(a.repeats):
        sets = {"plain": (open_ctx(S, False, torch_stream=True), S), "armed": (open_ctx(S, True, torch_stream=True), S)}
        for name, v in alternating_p50(sets, audio, a.warmup, a.hops).items():
            fig[f"{name}.push_host_p50_us"].append(v)
        for name, (ctx, _) in sets.items():
            fig[f"{name}.push_kernel_us"].append(kernel_us(ctx, S, audio))
            fig[f"{name}.stream_us_per_push"].append(stream_us_per_push(ctx, S, audio))
            ctx.stream_close(); ctx.close()
    return {k: med_spread(v) for k, v in fig.items()}


def never_deactivated_section(specs):
    runs = {}
    for spec in specs:
        label, path = spec.split("=", 1)
        runs[label] = json.load(open(path))
    out = {"runs": runs}
    parents = [v for k, v in runs.items() if k.startswith("parent")]
    if "tree" in runs and len(parents) >= 2:
        verdict = {}
        for key, got in runs["tree"].items():
            lo, hi = min(p[key]["median"] for p in parents), max(p[key]["median"] for p in parents)
            verdict[key] = {"parent_min": lo, "parent_max": hi, "tree": got["median"], "within_parent_interval": bool(lo <= got["median"] <= hi),
                            "below_both_parent_runs": bool(got["median"] < lo)}
        out["tree_against_parent"] = verdict
        out["condition"] = "every figure (a time: lower is better) of the tree lies inside the interval of the two parent runs, or below both"
        out["condition_met"] = bool(all(v["within_parent_interval"] or v["below_both_parent_runs"] for v in verdict.values()))
    return out


def main():
    a = ARGS
    if a.dense_only:
        out = dense_only(a)
    else:
        slots = a.slots
        audio = gated_audio(slots, 200)
        out = {"config": f"{slots} slots of gated audio, 10 ms hops; armed = utterances (windows {ON} / {OFF}, pre-roll {PRE_ROLL}) + events "
                         f"(smooth_window {SMOOTH}); {a.hops} timed hops after {a.warmup}, {a.repeats} repeats; the sets of a section alternate hop by hop"}
        out["sparse_cost"] = cost_section(slots, False, [16, 64, 256, slots], [16, 64, 256], audio, a)
        out["armed_cost"] = cost_section(slots, True, [64, slots], [64], audio, a)
        counts = [1, 8, 64]
        host = {k: {n: [] for n in counts} for k in ("deactivate", "activate", "reset")}
        dev = {k: {n: [] for n in counts} for k in host}
        for _ in range(a.repeats):
            for k, per in transitions(slots, audio, counts).items():
                for n, (h, d) in per.items():
                    host[k][n].append(h)
                    dev[k][n].append(d)
        stream_key = {"deactivate": "stream_us_deactivate_then_activate", "activate": "stream_us_on_active_streams", "reset": "stream_us"}
        out["transitions"] = {f"{k}_{n}_streams": {"host_p50_us": med_spread(host[k][n]), stream_key[k]: med_spread(dev[k][n])}
                              for k in host for n in counts}
        for sec in ("sparse_cost", "armed_cost"):
            s = out[sec]
            d64 = s["dense_64"]["push_host_p50_us"]
            out[sec]["sparse_64_minus_dense_64_p50_us"] = s[f"sparse_64_of_{slots}"]["push_host_p50_us"]["median"] - d64["median"]
            out[sec]["dense_64_run_to_run_spread_us"] = d64["max"] - d64["min"]
            out[sec]["dense_slots_over_sparse_64_p50"] = s[f"dense_{slots}"]["push_host_p50_us"]["median"] / s[f"sparse_64_of_{slots}"]["push_host_p50_us"]["median"]
        if a.never_deactivated:
            out["never_deactivated_set"] = never_deactivated_section(a.never_deactivated)
    path = a.out or os.path.join(ROOT, "profiles", "stream_active_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
