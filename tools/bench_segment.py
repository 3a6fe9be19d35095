#!/usr/bin/env python3
"""Utterances from a long recording: KeywordSpotter.segment and its parts against the ways to do without them, on one MI355X.

    python tools/bench_segment.py [--seconds 600] [--reps 20] [--warmup 3] [--out profiles/segment_bench.json]

One recording (default 10 minutes = 9.6 M samples) of gated speech-like audio: the generator of tests/golden/speechlike.py for one
second, a floor of +-3 for the next, and so on.  The threshold lies midway between the median log energy of the two kinds of
second.  All routes run in one process, alternated repetition by repetition, after a warm-up; medians are reported.

  device parts (events on the context's stream around each call)
    frames     kws_frames_i16
    walk       kws_segment_f32 (its two launches)
    cut        kws_cut_i16 of the U spans into [U, 16000]
    classify   kws_infer_i16 on the U clips
  host to host (wall time, host PCM in, Python results out)
    segment    KeywordSpotter.segment
    host route kws_frames_i16, download, the walk and the cut in NumPy, upload, kws_infer_i16
    scan       KeywordSpotter.scan at hop 1 with events: the same question asked of every window
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
from kws import _native
from kws.inference import KeywordSpotter
from kws.libs.models import DepthwiseSeparableConv

DEV = torch.device("cuda", 0)
C, NCEP, N_CLIP = 12, 10, 16000
ON, OFF, PRE_ROLL, MAX_FRAMES, MAX_UTTS = 40, 80, 60, 1000, 1024


def recording(seconds):
    from speechlike import speechlike_clip

    rng = np.random.default_rng(0)
    pool = [speechlike_clip(400 + i, -6.0 - 2.0 * i, "zeros" if i % 2 == 0 else "dither") for i in range(16)]
    parts = [pool[(s // 2) % 16] if s % 2 == 0 else rng.integers(-3, 4, N_CLIP).astype(np.int16) for s in range(seconds)]
    return np.concatenate(parts)


def host_walk(c0, threshold, n_total):
    """The walk of tests/_segment_ref.py with its per-frame conditions vectorised and the walk hopping from event to event."""
    v = ref.voiced_flags(c0, threshold)
    F = len(v)
    open_ok = np.flatnonzero(10 * ref.window_counts(v, ON) > 8 * ON)
    close_ok = np.flatnonzero(10 * (OFF - ref.window_counts(v, OFF)) > 9 * OFF)
    out, f, prev_close = [], 0, -1
    while True:
        i = np.searchsorted(open_ok, f)
        if i == len(open_ok):
            return out
        opened = int(open_ok[i])
        j = np.searchsorted(close_ok, opened + 1)
        closed, reason = (int(close_ok[j]), 0) if j < len(close_ok) else (F, 2)
        if MAX_FRAMES > 0 and opened + MAX_FRAMES - 1 < closed:
            closed, reason = opened + MAX_FRAMES - 1, 1
        if closed > F - 1:
            closed, reason = F - 1, 2
        out.append((max(opened - PRE_ROLL, prev_close + 1, 0) * 160, min(n_total, closed * 160 + 400), opened, closed, reason))
        prev_close, f = closed, closed + 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench.json"))
    a = ap.parse_args()
    blob = bench.bench_weights()[0]
    model = DepthwiseSeparableConv(num_classes=C)
    model.load_state_dict(ref.state_from_blob(blob))
    spotter = KeywordSpotter(model)
    ctx = model._context(0)
    host = recording(a.seconds)
    n = len(host)
    pcm = torch.from_numpy(host).to(DEV)[None, :]
    F = _native.host_scan_shape(n)[0]
    feat = torch.empty((1, F, NCEP), device=DEV)
    ctx.frames_i16(pcm, feat)
    c0 = feat[0, :, 0].cpu().numpy()
    second = (np.arange(F) * 160 // N_CLIP) % 2
    threshold = 0.5 * float(np.median(c0[second == 0]) + np.median(c0[second == 1]))
    count = torch.empty((1,), dtype=torch.int32, device=DEV)
    utt = torch.empty((1, MAX_UTTS, 5), dtype=torch.int32, device=DEV)
    ctx.segment_f32(feat, n, threshold, count, utt, MAX_UTTS, ON, OFF, PRE_ROLL, MAX_FRAMES)
    U = int(count.item())
    found = utt[0, :U].cpu().numpy()
    want = host_walk(c0, threshold, n)
    assert U > 0 and found.tolist() == [list(w) for w in want], "the device walk and the host walk disagree"
    span = torch.tensor([(0, int(s), int(e)) for s, e in found[:, :2]], dtype=torch.int32, device=DEV)
    clips = torch.empty((U, N_CLIP), dtype=torch.int16, device=DEV)
    logits, labels = torch.empty((U, C), device=DEV), torch.empty((U,), dtype=torch.int32, device=DEV)
    ctx.cut_i16(pcm, span, clips)
    want_clips = ref.cut_ref(host[None, :], [(0, int(s), int(e)) for s, e in found[:, :2]], 16384, N_CLIP)[0]
    assert np.array_equal(clips.cpu().numpy(), want_clips), "the device cut and the NumPy cut disagree"

    def host_route():
        ctx.frames_i16(pcm, feat)
        col = feat[0, :, 0].cpu().numpy()
        spans = [(0, w[0], w[1]) for w in host_walk(col, threshold, n)]
        x = torch.from_numpy(ref.cut_ref(host[None, :], spans, 16384, N_CLIP)[0]).to(DEV)
        ctx.infer_i16(x, logits, labels)
        return labels.cpu().numpy()

    device_parts = {"frames_ms": lambda: ctx.frames_i16(pcm, feat),
                    "walk_ms": lambda: ctx.segment_f32(feat, n, threshold, count, utt, MAX_UTTS, ON, OFF, PRE_ROLL, MAX_FRAMES),
                    "cut_ms": lambda: ctx.cut_i16(pcm, span, clips),
                    "classify_ms": lambda: ctx.infer_i16(clips, logits, labels)}
    host_to_host = {"segment_host_pcm_ms": lambda: spotter.segment(host, threshold, ON, OFF, PRE_ROLL, MAX_FRAMES / 100.0),
                    "segment_device_pcm_ms": lambda: spotter.segment(pcm, threshold, ON, OFF, PRE_ROLL, MAX_FRAMES / 100.0),
                    "host_route_device_pcm_ms": host_route,
                    "scan_hop1_device_pcm_ms": lambda: spotter.scan(pcm, hop_frames=1, threshold=0.5)}
    times = {k: [] for k in list(device_parts) + list(host_to_host)}
    for rep in range(a.warmup + a.reps):
        for k, fn in device_parts.items():
            ms = timed(fn)
            if rep >= a.warmup:
                times[k].append(ms)
        for k, fn in host_to_host.items():
            ms = wall(fn)
            if rep >= a.warmup:
                times[k].append(ms)
    res = {"device": torch.cuda.get_device_name(0), "seconds": a.seconds, "samples": n, "frames": F, "utterances": U,
           "threshold": threshold, "windows": [ON, OFF], "reps": a.reps, "warmup": a.warmup,
           "timing": "medians; device parts by events around each call, host-to-host routes by wall time, all alternated in one process",
           "device_walk_equals_host_walk": True, "device_cut_equals_numpy_cut": True}
    res.update({k: float(np.median(v)) for k, v in times.items()})
    res.update({k.replace("_ms", "_min_ms"): float(np.min(v)) for k, v in times.items()})
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
