#!/usr/bin/env python3
"""float32 recordings: the wavefront-resident float front end against the tile kernel and the int16 entry, and the float methods
of KeywordSpotter against their work-arounds, on one MI355X.

    python tools/bench_scan_f32.py [--seconds 600] [--recordings 64] [--reps 20] [--warmup 3] [--out profiles/scan_f32_bench.json]

All variants run in one process, alternated repetition by repetition, after a warm-up.  Every figure is a median; next to it
stands the SPREAD of the same code: the repetitions of a variant are split into the even and the odd ones, and the spread is the
distance between the two halves' medians.  A difference between two variants below their spreads is no difference.

  frames of one long recording (events on the context's stream around each call, device samples in)
    frames_f32_ms        kws_frames_f32: the wavefront-resident float kernel (n_total % 8 == 0)
    mfcc_f32_tile_ms     kws_mfcc_f32 on a context configured for a clip of n_total samples: the tile kernel, the only float route
                         before kws_frames_f32 -- the same words (asserted)
    frames_i16_ms        kws_frames_i16 on the same audio quantised to int16 (half the sample bytes)
  host to host (wall time, host samples in, Python results out)
    scan_f32_ms          KeywordSpotter.scan_f32
    quantise_scan_ms     the work-around: upload, quantise on the device with torch, KeywordSpotter.scan
    batch_f32_ms         scan_batch_f32 + segment_batch_f32 over R float recordings of 2 .. 59 s
    loop_f32_ms          the loop over scan_f32 + segment_f32
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "keyword-spotting_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import bench
import _segment_ref as ref
from bench_segment import recording, timed, wall
from kws import _native
from kws.inference import KeywordSpotter
from kws.libs.models import DepthwiseSeparableConv

DEV = torch.device("cuda", 0)
C, NCEP = 12, 10


def summary(v):
    """median, the same code's spread (even against odd repetitions), min and max of one variant's repetitions."""
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "spread": float(abs(np.median(v[0::2]) - np.median(v[1::2]))), "min": float(v.min()),
            "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_f32_bench.json"))
    a = ap.parse_args()
    blob = bench.bench_weights()[0]
    model = DepthwiseSeparableConv(num_classes=C)
    model.load_state_dict(ref.state_from_blob(blob))
    spotter = KeywordSpotter(model)
    ctx = model._context(0)
    tile_ctx = _native.Context(0)
    tile_ctx.use_torch_stream()

    pcm = recording(a.seconds)
    n = len(pcm)
    assert n % 8 == 0
    rng = np.random.default_rng(1)
    x = (pcm.astype(np.float32) / np.float32(32768.0)) * np.float32(0.83) + rng.normal(0.0, 1e-5, n).astype(np.float32)  # off the int16 grid
    F, W = _native.host_scan_shape(n)
    tile_ctx.set_frontend(n_samples=n)
    d_x = torch.from_numpy(x).to(DEV)[None, :]
    d_q = torch.from_numpy(pcm).to(DEV)[None, :]
    feat, feat_tile, feat_i16 = (torch.empty((1, F, NCEP), device=DEV) for _ in range(3))
    front = {"frames_f32_ms": lambda: ctx.frames_f32(d_x, feat),
             "mfcc_f32_tile_ms": lambda: tile_ctx.mfcc_f32(d_x, feat_tile.view(1, 1, F, NCEP)),
             "frames_i16_ms": lambda: ctx.frames_i16(d_q, feat_i16)}
    for fn in front.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(feat, feat_tile), "the wavefront-resident float kernel and the tile kernel differ"

    # host to host: one recording of a tenth of the long one, and the batch of bench_ragged.py
    one = x[:n // 10 // 8 * 8].copy()

    def quantise_scan():
        q = (torch.from_numpy(one).to(DEV) * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        return spotter.scan(q, hop_frames=1)

    lengths = np.exp(rng.uniform(np.log(2.0), np.log(60.0), a.recordings) + np.log(16000.0)).astype(np.int64)
    source = recording(61).astype(np.float32) / np.float32(32768.0) * np.float32(0.83)
    recs = [np.roll(source, -16000 * int(r))[:int(m)].copy() for r, m in enumerate(lengths)]
    f0 = torch.empty((1, _native.host_scan_shape(len(recs[0]))[0], NCEP), device=DEV)
    ctx.frames_f32(torch.from_numpy(recs[0]).to(DEV)[None, :], f0)
    col = f0[0, :, 0].cpu().numpy()
    second = (np.arange(len(col)) * 160 // 16000) % 2
    threshold = 0.5 * float(np.median(col[second == 0]) + np.median(col[second == 1]))
    routes = {"scan_f32_ms": lambda: spotter.scan_f32(one, hop_frames=1),
              "quantise_scan_ms": quantise_scan,
              "batch_f32_ms": lambda: (spotter.scan_batch_f32(recs, hop_frames=1, threshold=0.5), spotter.segment_batch_f32(recs, threshold)),
              "loop_f32_ms": lambda: ([spotter.scan_f32(r, hop_frames=1, threshold=0.5) for r in recs],
                                      [spotter.segment_f32(r, threshold) for r in recs])}
    (b_scan, b_seg), (l_scan, l_seg) = routes["batch_f32_ms"](), routes["loop_f32_ms"]()
    assert all(np.array_equal(g.labels, w.labels) and g.events == w.events for g, w in zip(b_scan, l_scan))
    assert [len(g) for g in b_seg] == [len(w[0]) for w in l_seg]

    times = {k: [] for k in list(front) + list(routes)}
    for rep in range(a.warmup + a.reps):
        for k, fn in front.items():
            ms = timed(fn)
            if rep >= a.warmup:
                times[k].append(ms)
        for k, fn in routes.items():
            ms = wall(fn)
            if rep >= a.warmup:
                times[k].append(ms)

    res = {"device": torch.cuda.get_device_name(0), "seconds": a.seconds, "samples": n, "frames": F, "scan_seconds": len(one) / 16000.0,
           "recordings": len(recs), "batch_seconds_total": float(lengths.sum() / 16000.0), "utterances": sum(len(g) for g in b_seg),
           "reps": a.reps, "warmup": a.warmup,
           "timing": "medians; spread = |median(even reps) - median(odd reps)| of the same variant; the front end by events around each "
                     "call, host-to-host routes by wall time; all variants alternated in one process"}
    for k, v in times.items():
        s = summary(v)
        res[k] = s["median"]
        res[k.replace("_ms", "_spread_ms")] = s["spread"]
        res[k.replace("_ms", "_min_ms")] = s["min"]
        res[k.replace("_ms", "_max_ms")] = s["max"]
    res["f32_kernel_not_slower_than_tile"] = bool(res["frames_f32_ms"] <= res["mfcc_f32_tile_ms"] + max(res["frames_f32_spread_ms"], res["mfcc_f32_tile_spread_ms"]))
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    tile_ctx.close()


if __name__ == "__main__":
    main()
