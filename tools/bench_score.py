#!/usr/bin/env python3
"""Time an event-level threshold sweep two ways on one GPU: kws_scan_score_f32 and the way there was before it.

The logits are synthetic (a piecewise-constant label track per recording, logit 12 on the track's class, uniform noise of +-0.5
elsewhere, as the decision tests use), so no model is needed: --recordings recordings of --minutes minutes at hop_frames = 1
(one window per 10 ms), C = 12, smooth_window = 30, refractory = 50, --thresholds thresholds evenly spaced in (0, 1), and a few
hundred annotations per recording cut from the label track (some of them displaced, so that misses and false alarms occur).

  score     ONE kws_scan_score_f32 call and the read-back of its K * C * 4 counters
  detect    K calls of kws_scan_detect_f32 (max_events = the most events a recording can have), per call the read-back of the
            counts, windows and labels, and a vectorised NumPy matcher of the events against the sorted table (one searchsorted
            over all events of the call, hits and duplicates by the first occurrence of each matched interval)

Both run in one process, alternated, --reps times each after --warmup of each; a run is timed with device events around its
work and with a host clock that ends with the last result on the host.  The detect loop reads back and matches between its calls,
so both of its clocks span that host work as well: it is part of that way of getting the curve.  The two must give the same
counters, exactly.

The stages of the score call: stage 1 (softmax + smoothing at a threshold of -inf) does not depend on K, and stage 2 is one walk
per recording and threshold.  The entry does not expose them apart, so they are taken from two calls timed with device events:
K = 1 without annotations (stage 1 and one walk per recording) and K thresholds; their difference is the cost of the other
K - 1 walks and of the matching.  One kws_scan_detect_f32 call is timed the same way for scale.

    python tools/bench_score.py [--recordings 64] [--minutes 10] [--thresholds 256] [--reps 5] [--warmup 1] [--out profiles/score_bench.json]

Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "keyword-spotting_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

C, S, REFRACTORY, FIRST_KEYWORD = 12, 30, 50, 2


def make_case(R, W, per_recording, seed=0):
    """(logits float32 [R, W, C], annotations int32 [N, 4]): the label track in segments of 1..40 windows; an annotation is a
    keyword segment of the track, from its first window to 20 windows past its last (every fifth one moved 300 windows on)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-0.5, 0.5, size=(R, W, C)).astype(np.float32)
    rows = []
    for r in range(R):
        lens = rng.integers(1, 41, size=W)  # more than enough segments
        ends = np.cumsum(lens)
        n = int(np.searchsorted(ends, W)) + 1
        starts, ends, labels = np.concatenate([[0], ends[:n - 1]]), np.minimum(ends[:n], W), rng.integers(0, C, size=n)
        track = np.repeat(labels, ends - starts)
        z[r, np.arange(W), track] += 12.0
        picked = 0
        for i in rng.permutation(n)[:4 * per_recording]:
            k = int(labels[i])
            if k < FIRST_KEYWORD or picked >= per_recording:
                continue
            rows.append([r, k, int(starts[i]), int(ends[i]) + 19])
            picked += 1
    rows = np.asarray(rows, np.int64)
    rows[::5, 2:4] += 300
    # intervals of one recording and label must be disjoint: in window order, drop what overlaps the one kept before it
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    keep = np.ones(len(rows), bool)
    last = {}
    for i, (r, k, a, b) in enumerate(rows):
        if last.get((r, k), -1) >= a:
            keep[i] = False
        else:
            last[(r, k)] = b
    return z, np.ascontiguousarray(rows[keep].astype(np.int32))


def numpy_counts(count, ev_w, ev_k, table, off, num_classes):
    """One threshold's events (count [R], windows and labels [R, M], in window order) against the sorted table -> int64 [C, 4]."""
    R, M = ev_w.shape
    valid = np.arange(M)[None, :] < count[:, None]
    r = np.broadcast_to(np.arange(R)[:, None], (R, M))[valid]
    w, k = ev_w[valid].astype(np.int64), ev_k[valid].astype(np.int64)
    out = np.zeros((num_classes, 4), np.int64)
    if len(w) == 0:
        return out
    big = np.int64(1) << 32
    key = (table[:, 0].astype(np.int64) * num_classes + table[:, 1]) * big + table[:, 2]  # ascending: the table is sorted
    j = np.searchsorted(key, (r * num_classes + k) * big + w, "right") - 1  # the last interval that begins at or before the event
    lst = r * num_classes + k
    inside = (j >= off[lst]) & (j >= 0)
    jj = np.where(inside, j, 0)
    inside &= w <= table[jj, 3]
    out[:, 1] = np.bincount(k[~inside], minlength=num_classes)
    jm, km, wm = jj[inside], k[inside], w[inside]
    _, first = np.unique(jm, return_index=True)  # events are in window order within a recording: the first occurrence is the hit
    out[:, 0] = np.bincount(km[first], minlength=num_classes)
    out[:, 2] = np.bincount(km, minlength=num_classes) - out[:, 0]
    out[:, 3] = np.bincount(km[first], weights=(wm[first] - table[jm[first], 2]).astype(np.float64), minlength=num_classes).astype(np.int64)
    return out


def timed(fn):
    """(result, device ms between two events, host ms until fn has returned and the device is idle)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--thresholds", type=int, default=256)
    ap.add_argument("--annotations", type=int, default=300, help="per recording, before overlapping ones are dropped")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score needs a GPU: the timings are of HIP kernels and there is no CPU fallback")
    from kws import _native

    dev = torch.device("cuda", 0)
    R, K = args.recordings, args.thresholds
    _, W = _native.host_scan_shape(int(args.minutes * 60 * 16000), 400, 160, 99, 1)
    z, truth = make_case(R, W, args.annotations)
    table, off = _native.host_score_plan(truth, R, C, FIRST_KEYWORD)
    thresholds = ((np.arange(K) + 0.5) / K).astype(np.float32)
    M = W // REFRACTORY + 1  # the most events of a recording
    ctx = _native.Context(0)
    ctx.use_torch_stream()
    zd = torch.from_numpy(z).to(dev)
    counts = torch.zeros((K, C, 4), dtype=torch.int64, device=dev)
    count = torch.zeros((R,), dtype=torch.int32, device=dev)
    ev_w, ev_k = (torch.zeros((R, M), dtype=torch.int32, device=dev) for _ in range(2))
    ev_s = torch.zeros((R, M), device=dev)

    def by_score(th=thresholds, tr=truth, out=counts):
        ctx.scan_score_f32(zd, S, FIRST_KEYWORD, REFRACTORY, th, tr, out)
        return out.cpu().numpy()

    def one_detect(t):
        ctx.scan_detect_f32(zd, S, FIRST_KEYWORD, float(t), REFRACTORY, count, ev_w, ev_k, ev_s, M)

    def by_detect():
        got = np.zeros((K, C, 4), np.int64)
        for i, t in enumerate(thresholds):
            one_detect(t)
            got[i] = numpy_counts(count.cpu().numpy(), ev_w.cpu().numpy(), ev_k.cpu().numpy(), table, off, C)
        return got

    runs = {"score": [], "detect": []}
    results = {}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("score", by_score), ("detect", by_detect)):
            out, dev_ms, host_ms = timed(fn)
            if rep >= args.warmup:
                runs[name].append((dev_ms, host_ms))
            assert name not in results or np.array_equal(results[name], out), f"{name}: two runs differ"
            results[name] = out
    same = bool(np.array_equal(results["score"], results["detect"]))
    stages = {"score_one_threshold_no_annotations": [], "score_all_thresholds": [], "one_detect_call": []}
    one = torch.zeros((1, C, 4), dtype=torch.int64, device=dev)
    for rep in range(args.warmup + args.reps):
        for name, fn in (("score_one_threshold_no_annotations", lambda: ctx.scan_score_f32(zd, S, FIRST_KEYWORD, REFRACTORY, thresholds[K // 2:K // 2 + 1], None, one)),
                         ("score_all_thresholds", lambda: ctx.scan_score_f32(zd, S, FIRST_KEYWORD, REFRACTORY, thresholds, truth, counts)),
                         ("one_detect_call", lambda: one_detect(0.5))):
            _, dev_ms, _ = timed(fn)
            if rep >= args.warmup:
                stages[name].append(dev_ms)
    med = lambda v: float(np.median(v))
    summary = lambda v: {"device_events_ms": med([a for a, _ in v]), "host_clock_ms": med([b for _, b in v]),
                         "host_min_max_ms": [float(min(b for _, b in v)), float(max(b for _, b in v))]}
    st = {k: med(v) for k, v in stages.items()}
    total = results["score"].sum(axis=1)
    res = {"tool": "bench_score", "device": torch.cuda.get_device_name(0), "recordings": R, "windows_per_recording": W, "num_classes": C,
           "smooth_window": S, "refractory": REFRACTORY, "first_keyword": FIRST_KEYWORD, "thresholds": K, "annotations": int(len(truth)),
           "hours": R * args.minutes / 60.0, "reps": args.reps, "warmup": args.warmup,
           "score": summary(runs["score"]), "detect_loop": summary(runs["detect"]),
           "score_over_detect_loop": {"device_events": med([a for a, _ in runs["score"]]) / med([a for a, _ in runs["detect"]]),
                                      "host_clock": med([b for _, b in runs["score"]]) / med([b for _, b in runs["detect"]])},
           "counters_equal": same,
           "stages_device_events_ms": dict(st, sweep_of_the_other_thresholds=st["score_all_thresholds"] - st["score_one_threshold_no_annotations"]),
           "counts_at_lowest_middle_highest_threshold": {name: [int(v) for v in total[i]] for name, i in
                                                         (("lowest", 0), ("middle", K // 2), ("highest", K - 1))}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not same:
        raise SystemExit("the counters of kws_scan_score_f32 differ from the detect loop's")


if __name__ == "__main__":
    main()
