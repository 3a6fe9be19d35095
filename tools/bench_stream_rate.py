#!/usr/bin/env python3
"""What streaming at another sample rate costs: 64 concurrent streams, 10 ms hops, host memory to host memory.

    python tools/bench_stream_rate.py [--streams 64] [--hops 2000] [--warmup 200] [--out profiles/stream_rate_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python tools/bench_stream_rate.py --hops 300 --device-only

One process, four contexts, the paths alternating hop by hop so that clocks and the machine's other tenants hit them alike:

    push_host_16k      kws_stream_push_host_i16 with 160 samples per stream at 16 kHz: the unchanged path, the baseline
    push_host_rate_48k kws_stream_push_host_rate_i16 with 480 samples per stream at 48 kHz
    push_host_rate_44k kws_stream_push_host_rate_i16 with 441 samples per stream at 44.1 kHz
    scipy_then_push    what a caller did before: scipy.signal.resample_poly over history + hop for every stream on the host
                       (48 kHz, a kept history of 62 samples, the delayed outputs cut out), then kws_stream_push_host_i16

Latency = host wall time from the hop in a numpy array to logits and labels readable in host memory.  --device-only runs the
two rate paths alone (for a kernel trace: the resampler's own time comes from there, it is not timed by kws_prof_*)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "keyword-spotting_amd"))
import bench
from kws import _native


def open_ctx(S, rate=None, hop_in=0):
    ctx = _native.Context(0)
    ctx.load_dscnn(bench.bench_weights()[0], 12)
    ctx.stream_open(S)
    ctx.stream_host_results(True)
    if rate:
        ctx.stream_resample_open(S, rate, 16000, hop_in)
    return ctx


class ScipyThenPush:
    """Stateful host resampling at 48 kHz: keep the last H samples, filter history + hop, cut the hop's 160 delayed outputs."""

    def __init__(self, S):
        from scipy.signal import resample_poly

        self.resample_poly = resample_poly
        self.ctx = open_ctx(S)
        self.S = S
        up, down, self.delay, self.H = _native.host_stream_resample_plan(48000, 16000)
        self.keep = -(-(self.H + 3 * self.delay) // 3) * 3  # a multiple of down, so the hop's outputs start on an output index
        self.hist = np.zeros((S, self.keep), np.float64)

    def push(self, hop48):
        buf = np.concatenate([self.hist, hop48.astype(np.float64)], axis=1)
        y = self.resample_poly(buf, 1, 3, axis=1, window=("kaiser", 14.0))
        lo = self.keep // 3 - self.delay
        hop16 = np.rint(np.clip(y[:, lo:lo + 160], -32768.0, 32767.0)).astype(np.int16)
        self.hist = buf[:, -self.keep:]
        return self.ctx.stream_push_host_i16(np.ascontiguousarray(hop16), self.S)


def stats(lat):
    lat = np.asarray(lat)
    return {"p50_us": float(np.percentile(lat, 50)), "p90_us": float(np.percentile(lat, 90)), "p99_us": float(np.percentile(lat, 99)),
            "mean_us": float(lat.mean()), "hops_timed": int(lat.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--hops", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_rate_bench.json"))
    ap.add_argument("--device-only", action="store_true", help="the two rate paths alone, nothing written (for a kernel trace)")
    a = ap.parse_args()
    S = a.streams
    rng = np.random.default_rng(0)
    audio = {"16k": rng.integers(-16384, 16384, (64, S, 160), dtype=np.int16), "48k": rng.integers(-16384, 16384, (64, S, 480), dtype=np.int16),
             "44k": rng.integers(-16384, 16384, (64, S, 441), dtype=np.int16)}
    c48, c44 = open_ctx(S, 48000, 480), open_ctx(S, 44100, 441)
    paths = {"push_host_rate_48k": lambda t: c48.stream_push_host_rate_i16(audio["48k"][t % 64], S),
             "push_host_rate_44k": lambda t: c44.stream_push_host_rate_i16(audio["44k"][t % 64], S)}
    closers = [c48, c44]
    if not a.device_only:
        c16, host = open_ctx(S), ScipyThenPush(S)
        paths = {"push_host_16k": lambda t: c16.stream_push_host_i16(audio["16k"][t % 64], S), **paths,
                 "scipy_then_push": lambda t: host.push(audio["48k"][t % 64])}
        closers += [c16, host.ctx]
    lat = {k: [] for k in paths}
    for t in range(a.warmup + a.hops):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            lg, lb = fn(t)
            res = (lb.copy(), lg.copy())
            dt = (time.perf_counter() - t0) * 1e6
            if t >= a.warmup:
                lat[name].append(dt)
    for c in closers:
        c.stream_close(); c.close()
    out = {"config": f"{S} concurrent streams, 10 ms hops, host array in -> logits and labels in host arrays; paths alternate hop by hop in one process",
           "warmup_hops": a.warmup, **{k: stats(v) for k, v in lat.items()}}
    if not a.device_only:
        base = out["push_host_16k"]["p50_us"]
        out["added_p50_us"] = {k: out[k]["p50_us"] - base for k in ("push_host_rate_48k", "push_host_rate_44k", "scipy_then_push")}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
