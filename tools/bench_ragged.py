#!/usr/bin/env python3
"""A batch of recordings of unequal length: KeywordSpotter.scan_batch / segment_batch against the loop over the single-recording
methods, on one MI355X.

    python tools/bench_ragged.py [--recordings 64] [--reps 7] [--warmup 2] [--out profiles/ragged_bench.json]

Workload: R recordings (default 64) of gated speech-like audio (the generator of tools/bench_segment.py: a second of speech-like
signal, a second of +-3 floor, ...), lengths drawn log-uniform in [2 s, 60 s] from a fixed seed; hop 1; host PCM in, Python results
out.  All routes run in one process, alternated repetition by repetition, after a warm-up; medians are reported.

  host to host (wall time)
    (a) batch       one scan_batch call, one segment_batch call
    (b) loop        scan / segment per recording -- the baseline, code the ragged entries do not touch
  front end alone (events on the context's stream around each call, device PCM in)
    ragged          kws_frames_ragged_i16 over the packed buffer
    loop            kws_frames_i16 per recording, summed
    (c) padded      kws_frames_i16 on the batch zero-padded to its longest (a different answer at every recording's end: timing only)
  device time per kernel family (kws_prof_read, one profiled pass per route)
    KWS_K_MFCC, KWS_K_MFCC_REFINE, KWS_K_DSCNN of (a) and (b), and the straddling windows' share of the packed scan
"""
import argparse
import json
import os
import sys
import time

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
FAMILIES = {"mfcc_ms": _native.KWS_K_MFCC, "mfcc_refine_ms": _native.KWS_K_MFCC_REFINE, "dscnn_ms": _native.KWS_K_DSCNN}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.json"))
    a = ap.parse_args()
    blob = bench.bench_weights()[0]
    model = DepthwiseSeparableConv(num_classes=C)
    model.load_state_dict(ref.state_from_blob(blob))
    spotter = KeywordSpotter(model)
    ctx = model._context(0)

    rng = np.random.default_rng(0)
    lengths = np.exp(rng.uniform(np.log(2.0), np.log(60.0), a.recordings) + np.log(16000.0)).astype(np.int64)
    source = recording(61)
    recs = [np.roll(source, -16000 * int(r))[:int(n)].copy() for r, n in enumerate(lengths)]
    frames, frame_off, windows, win_off, W_pack = _native.host_ragged_plan(lengths)
    # the threshold of tools/bench_segment.py: midway between the two kinds of second, from the first recording's frames
    x0 = torch.from_numpy(recs[0]).to(DEV)[None, :]
    f0 = torch.empty((1, int(frames[0]), NCEP), device=DEV)
    ctx.frames_i16(x0, f0)
    col = f0[0, :, 0].cpu().numpy()
    second = (np.arange(len(col)) * 160 // 16000) % 2
    threshold = 0.5 * float(np.median(col[second == 0]) + np.median(col[second == 1]))

    scan_kw = dict(hop_frames=1, threshold=0.5)
    routes = {"batch_scan_ms": lambda: spotter.scan_batch(recs, **scan_kw),
              "loop_scan_ms": lambda: [spotter.scan(x, **scan_kw) for x in recs],
              "batch_segment_ms": lambda: spotter.segment_batch(recs, threshold),
              "loop_segment_ms": lambda: [spotter.segment(x, threshold) for x in recs]}
    # the two routes answer alike (the GPU tests hold them bit for bit; here: the counts)
    got, want = routes["batch_scan_ms"](), routes["loop_scan_ms"]()
    assert all(np.array_equal(g.labels, w.labels) and g.events == w.events for g, w in zip(got, want))
    n_events = sum(len(g.events[0]) for g in got)
    got, want = routes["batch_segment_ms"](), routes["loop_segment_ms"]()
    assert [len(g) for g in got] == [len(w[0]) for w in want]
    n_utts = sum(len(g) for g in got)

    # the front end alone, device PCM in
    buf, start, length = spotter._pack_batch([torch.from_numpy(x) for x in recs], [16000] * len(recs))
    feat = torch.empty((int(frame_off[-1]), NCEP), device=DEV)
    singles = [(torch.from_numpy(x).to(DEV)[None, :], torch.empty((1, int(F), NCEP), device=DEV)) for x, F in zip(recs, frames)]
    n_max = int(lengths.max())
    padded = torch.zeros((len(recs), n_max), dtype=torch.int16, device=DEV)
    for row, x in zip(padded, recs):
        row[:len(x)].copy_(torch.from_numpy(x))
    feat_padded = torch.empty((len(recs), _native.host_scan_shape(n_max)[0], NCEP), device=DEV)
    torch.cuda.synchronize()
    front = {"frames_ragged_ms": lambda: ctx.frames_ragged_i16(buf, start, length, 1, feat),
             "frames_loop_ms": lambda: [ctx.frames_i16(x, f) for x, f in singles],
             "frames_padded_ms": lambda: ctx.frames_i16(padded, feat_padded)}

    times = {k: [] for k in list(routes) + list(front)}
    for rep in range(a.warmup + a.reps):
        for k, fn in front.items():
            ms = timed(fn)
            if rep >= a.warmup:
                times[k].append(ms)
        for k, fn in routes.items():
            ms = wall(fn)
            if rep >= a.warmup:
                times[k].append(ms)

    # device time per kernel family: one profiled pass per route (events around every launch)
    families = {}
    ctx.prof_enable(True)
    for k, fn in list(routes.items()) + list(front.items()):
        ctx.prof_reset()
        fn()
        families[k.replace("_ms", "")] = {name: round(ctx.prof_read(kid)[0], 4) for name, kid in FAMILIES.items()}
        families[k.replace("_ms", "")]["launches"] = {name.replace("_ms", ""): ctx.prof_read(kid)[1] for name, kid in FAMILIES.items()}
    ctx.prof_enable(False)

    res = {"device": torch.cuda.get_device_name(0), "recordings": len(recs), "seconds_total": float(lengths.sum() / 16000.0),
           "seconds_min": float(lengths.min() / 16000.0), "seconds_max": float(lengths.max() / 16000.0),
           "frames_total": int(frames.sum()), "frames_padded": int(len(recs) * _native.host_scan_shape(n_max)[0]),
           "windows_total": int(windows.sum()), "windows_packed": int(W_pack),
           "straddling_window_share": float((W_pack - int(windows.sum())) / W_pack), "events": n_events, "utterances": n_utts,
           "threshold": threshold, "reps": a.reps, "warmup": a.warmup,
           "timing": "medians; host-to-host routes by wall time, the front end by events around each call, alternated in one process; "
                     "device_by_family from one profiled pass per route (kws_prof_read)",
           "device_by_family": families}
    res.update({k: float(np.median(v)) for k, v in times.items()})
    res.update({k.replace("_ms", "_min_ms"): float(np.min(v)) for k, v in times.items()})
    res["batch_ms"] = res["batch_scan_ms"] + res["batch_segment_ms"]
    res["loop_ms"] = res["loop_scan_ms"] + res["loop_segment_ms"]
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
