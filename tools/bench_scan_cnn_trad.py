#!/usr/bin/env python3
"""What cnn-trad-fpool3 costs on recordings and streams, against the contiguous-clip path it replaces.

    python tools/bench_scan_cnn_trad.py [--minutes 10] [--repeats 5] [--streams 64] [--hops 600] [--warmup 100]
                                        [--out profiles/scan_cnn_trad_bench.json]

One process, the paths alternating repeat by repeat (hop by hop for the push) so that clocks and the machine's other tenants hit
them alike:

    (a) windows_vs_clips   device time (events around the launches) of kws_forward_cnn_trad_windows_f32 over the frame array of
                           `minutes` of audio, at hop 1 and hop 10, against kws_forward_cnn_trad_f32 over the same windows
                           gathered into contiguous clips beforehand, in chunks of kws_host_cnn_trad_window_chunk().  The
                           contiguous path is timed twice per repeat (clips_a, clips_b): their ratio is the spread the
                           windows / clips ratio is read against.
    (b) scan_host_to_host  KeywordSpotter.scan(pcm, hop_frames) from host PCM to host logits, against the same job done by
                           cutting clips on the device (kws_cut_i16 over the windows' spans) and classifying them
                           (kws_infer_cnn_trad_i16): wall time.
    (c) push               kws_stream_push_cnn_trad_i16 on `streams` streams, hop in device memory to logits and labels in host
                           memory (sync + one read): p50 of the host wall time per push, the three kernels' event times, and
                           the DS-CNN push (kws_stream_push_host_i16, one launch, zero-copy) of the same box for orientation.
"""
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
T, NF, STEP, FRAME_LEN, C = 99, 10, 160, 400, 12


def med_spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def timed(fn):
    """Device milliseconds of what fn enqueues on torch's current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def windows_vs_clips(ctx, frames, hop, repeats):
    F = frames.shape[1]
    W = (F - T) // hop + 1
    chunk = _native.host_cnn_trad_window_chunk()
    logits = torch.empty((1, W, C), device=DEV)
    labels = torch.empty((1, W), dtype=torch.int32, device=DEV)
    idx = (torch.arange(W, device=DEV) * hop)[:, None] + torch.arange(T, device=DEV)[None, :]
    clips = frames[0][idx].reshape(W, 1, T, NF).contiguous()  # gathered beforehand: not part of the contiguous path's time
    want_l, want_k = torch.empty((W, C), device=DEV), torch.empty((W,), dtype=torch.int32, device=DEV)

    def in_place():
        ctx.forward_cnn_trad_windows_f32(frames, hop, logits, labels)

    def contiguous():
        for i in range(0, W, chunk):
            ctx.forward_cnn_trad_f32(clips[i:i + chunk], want_l[i:i + chunk], want_k[i:i + chunk])

    for fn in (in_place, contiguous):
        timed(fn)
    assert torch.equal(logits[0], want_l) and torch.equal(labels[0], want_k), "windows differ from their contiguous twins"
    ms = {"windows": [], "clips_a": [], "clips_b": []}
    order = [("windows", in_place), ("clips_a", contiguous), ("clips_b", contiguous)]
    for r in range(repeats):
        for name, fn in order[r % 3:] + order[:r % 3]:
            ms[name].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"windows": W, "chunk": chunk, "ms": {k: med_spread(v) for k, v in ms.items()},
            "windows_over_clips": med["windows"] / (0.5 * (med["clips_a"] + med["clips_b"])),
            "clips_a_over_clips_b": med["clips_a"] / med["clips_b"], "windows_per_s": W / med["windows"] * 1e3}


def scan_host_to_host(spotter, ctx, pcm, hop, repeats):
    n = pcm.shape[0]
    _, W = _native.host_scan_shape(n, FRAME_LEN, STEP, T, hop)

    def scan():
        return spotter.scan(pcm, hop_frames=hop).logits

    def cut_and_classify():
        x = torch.from_numpy(pcm[None]).to(DEV)
        start = torch.arange(W, dtype=torch.int32) * (hop * STEP)
        span = torch.stack([torch.zeros_like(start), start, start + 16000], dim=1).contiguous().to(DEV)
        out = np.empty((W, C), np.float32)
        for i in range(0, W, 4096):
            m = min(4096, W - i)
            clips = torch.empty((m, 16000), dtype=torch.int16, device=DEV)
            logits = torch.empty((m, C), device=DEV)
            ctx.cut_i16(x, span[i:i + m], clips, 0)
            ctx.infer_cnn_trad_i16(clips, logits)
            out[i:i + m] = logits.cpu().numpy()
        return out

    paths = [("scan", scan), ("cut_and_classify", cut_and_classify)]
    for _, fn in paths:
        fn()
    s = {k: [] for k, _ in paths}
    for r in range(repeats):
        for name, fn in paths[r % 2:] + paths[:r % 2]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            s[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in s.items()}
    return {"windows": W, "ms": {k: med_spread(v) for k, v in s.items()}, "scan_over_cut_and_classify": med["scan"] / med["cut_and_classify"]}


def push(S, hops, warmup, blob_ct):
    audio = np.random.default_rng(0).integers(-12000, 12001, (64, S, STEP)).astype(np.int16)
    ct = _native.Context(0)
    ct.use_torch_stream()
    ct.load_cnn_trad(blob_ct, C)
    ct.stream_open(S)
    ds = _native.Context(0)
    ds.load_dscnn(bench.bench_weights()[0], C)
    ds.stream_open(S)
    hop_buf = torch.zeros((S, STEP), dtype=torch.int16, device=DEV)
    out = torch.zeros((S * (C + 1),), device=DEV)
    lg, lb = out[:S * C].view(S, C), out[S * C:].view(torch.int32)

    def ct_push(h):
        hop_buf.copy_(torch.from_numpy(h))
        ct.stream_push_cnn_trad_i16(hop_buf, lg, lb)
        return out.cpu()  # waits for the stream: the one read

    paths = [("cnn_trad_push", ct_push), ("dscnn_push_host", lambda h: ds.stream_push_host_i16(h, S))]
    lat = {k: [] for k, _ in paths}
    for t in range(warmup + hops):
        h = np.ascontiguousarray(audio[t % len(audio)])
        for name, fn in paths[t % 2:] + paths[:t % 2]:
            t0 = time.perf_counter()
            fn(h)
            if t >= warmup:
                lat[name].append((time.perf_counter() - t0) * 1e6)
    ct.prof_enable(1)  # the kernels' own times, in pushes of their own: the events around every launch cost stream time
    for t in range(100):
        ct_push(np.ascontiguousarray(audio[t % len(audio)]))
    kernels = {}
    for name, kid in (("frame", _native.KWS_K_STREAM_FRAME), ("conv", _native.KWS_K_CNNTRAD_CONV), ("dense", _native.KWS_K_CNNTRAD_DENSE)):
        ms, n = ct.prof_read(kid)
        kernels[name + "_us"] = ms / max(n, 1) * 1e3
    ct.prof_enable(False)
    for c in (ct, ds):
        c.stream_close(); c.close()
    return {"streams": S, "hops": hops, "p50_us": {k: float(np.percentile(v, 50)) for k, v in lat.items()},
            "p99_us": {k: float(np.percentile(v, 99)) for k, v in lat.items()}, "cnn_trad_kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--hops", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_cnn_trad_bench.json"))
    args = ap.parse_args()
    from kws.inference import KeywordSpotter
    from kws.libs.models import CnnTradFpool3

    blob = bench.synth_cnn_trad_weights()
    n = int(args.minutes * 60 * 16000)
    pcm = np.random.default_rng(1).integers(-8000, 8001, n).astype(np.int16)
    ctx = _native.Context(0)
    ctx.use_torch_stream()
    ctx.load_cnn_trad(blob, C)
    F, _ = _native.host_scan_shape(n, FRAME_LEN, STEP, T, 1)
    frames = torch.empty((1, F, NF), device=DEV)
    ctx.frames_i16(torch.from_numpy(pcm[None]).to(DEV), frames)
    torch.cuda.synchronize()
    model = CnnTradFpool3(C)
    state, at = {}, 0
    for k, v in model.state_dict().items():
        state[k] = torch.from_numpy(blob[at:at + v.numel()].reshape(tuple(v.shape)).copy())
        at += v.numel()
    model.load_state_dict(state)
    spotter = KeywordSpotter(model)
    out = {"device": torch.cuda.get_device_name(0), "minutes": args.minutes, "frames": F, "repeats": args.repeats,
           "windows_vs_clips": {f"hop_{hop}": windows_vs_clips(ctx, frames, hop, args.repeats) for hop in (1, 10)},
           "scan_host_to_host": {f"hop_{hop}": scan_host_to_host(spotter, ctx, pcm, hop, max(2, args.repeats // 2)) for hop in (10, 1)},
           "push": push(args.streams, args.hops, args.warmup, blob)}
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
