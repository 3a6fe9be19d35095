#!/usr/bin/env python3
"""Resident training loader benchmark (GPU box): what a batch costs to produce on the device, against the parent route.

    python tools/bench_loader.py [--batches 1028,4096] [--iters 60] [--warmup 10] [--out profiles/train_loader_bench.json]

Prints one JSON line and writes it to --out.  Device events, medians over --iters timed iterations (at least 50) after
--warmup, the routes alternated iteration by iteration in one process so that they see the same clocks and neighbours.
Per kind of clip ("uniform": full-scale uniform noise; "speechlike": tests/golden/speechlike.py, dense precision flags) and
batch size B, on a split that lives in device memory:
  draw_ms       kws_augment_draw: the four draws of B clips
  fused_ms      kws_mfcc_augment_i16: gather + augment + MFCC (+ refinement) in one call
  composed_ms   index_select + kws_augment_i16 + kws_mfcc_f32 on the same draws: the kernels this route had before the fused
                entry existed -- the yardstick
  refined_frames_fused / _composed   frames the last call of each route redid in float64 (kws_frontend_stats)
  speedup       composed_ms / fused_ms
"host_draw_ms": per B, the wall time of transform_batch's host loop (four NumPy / random calls per clip) and the uploads of its four draw arrays.
"step": the bench_train.py DS-CNN step (zero_grad, refresh, forward, CrossEntropyLoss, backward, Adam) at B = 1028 on one
resident batch (resident_ms) against the same step fed a new DeviceBatchLoader batch every time (loader_fed_ms, the batch's
production inside the timed region), alternated.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "keyword-spotting_amd"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_SAMPLES = 16000
BG_LENS = [20000, 48000, 16001, 960000, 32000, 61234]


def med(xs):
    return round(float(np.median(np.asarray(xs))), 4)


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn):
    a, b = ev(), ev()
    a.record()
    fn()
    b.record()
    return a, b


def kernels(ctx, dev, pcm, labels, B, iters, warmup, cfg, seed):
    """draw / fused / composed on a resident split: pcm int16[N, n] and labels int32[N] on the device."""
    N = pcm.shape[0]
    rng = np.random.default_rng(seed)
    pool = torch.from_numpy((rng.standard_normal(sum(BG_LENS)) * 0.1).astype(np.float32)).to(dev)
    starts = torch.from_numpy(np.cumsum([0] + BG_LENS[:-1]).astype(np.int32)).to(dev)
    lens = torch.from_numpy(np.asarray(BG_LENS, np.int32)).to(dev)
    shift, off = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    vol, sil = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    idx = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).to(dev)
    idx64 = idx.long()
    nf, nc = ctx.frontend_shape()
    out_f = torch.empty((B, 1, nf, nc), dtype=torch.float32, device=dev)
    out_c = torch.empty_like(out_f)
    sig = torch.empty((B, N_SAMPLES), dtype=torch.float32, device=dev)
    kw = dict(shift=shift, bg=pool, bg_off=off, bg_vol=vol, silence=sil)

    def draw():
        ctx.augment_draw(seed, 0, idx, shift, off, vol, sil, labels=labels, time_shift=cfg.time_shift, bg_start=starts, bg_len=lens,
                         bg_volume=cfg.background_volume, bg_frequency=cfg.background_frequency, n_samples=N_SAMPLES)

    def fused():
        ctx.mfcc_augment_i16(pcm, idx, out_f, **kw)

    def composed():
        ctx.augment_i16(pcm.index_select(0, idx64), sig, **kw)
        ctx.mfcc_f32(sig, out_c)

    for _ in range(warmup):
        draw(), fused(), composed()
    torch.cuda.synchronize()
    evs = {"draw": [], "fused": [], "composed": []}
    for _ in range(iters):
        evs["draw"].append(timed(draw))
        evs["fused"].append(timed(fused))
        evs["composed"].append(timed(composed))
    torch.cuda.synchronize()
    ms = {k: med([a.elapsed_time(b) for a, b in v]) for k, v in evs.items()}
    fused()
    ctx.sync()
    refined_f = ctx.frontend_stats()[2]
    composed()
    ctx.sync()
    refined_c = ctx.frontend_stats()[2]
    return {"B": B, "draw_ms": ms["draw"], "fused_ms": ms["fused"], "composed_ms": ms["composed"],
            "speedup": round(ms["composed"] / ms["fused"], 3), "refined_frames_fused": refined_f, "refined_frames_composed": refined_c,
            "outputs_equal": bool(torch.equal(out_f, out_c))}


def host_draw_ms(B, iters, cfg, dev):
    """transform_batch's host work per batch: the per-clip draws (audio_processor.py) and the four uploads."""
    rng = np.random.default_rng(B)
    labels = rng.integers(0, 12, B)
    starts = np.cumsum([0] + BG_LENS[:-1])
    n, limit = N_SAMPLES, cfg.time_shift
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        shift = np.array([np.random.randint(-limit, limit) if limit > 0 else 0 for _ in range(B)], dtype=np.int32)
        silence = (labels == 0).astype(np.uint8)
        o, v = np.zeros(B, np.int32), np.zeros(B, np.float32)
        for i in range(B):
            k = random.randrange(len(BG_LENS))
            o[i] = starts[k] + np.random.randint(0, BG_LENS[k] - n)
            if silence[i]:
                v[i] = np.random.uniform(0, 1)
            elif np.random.uniform(0, 1) < cfg.background_frequency:
                v[i] = np.random.uniform(0, cfg.background_volume)
        up = [torch.from_numpy(a).to(dev) for a in (shift, silence, o, v)]
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        del up
    return med(out)


def step_pair(dev, pcm, labels, ap, B, iters, warmup):
    from kws.libs.data_loader import DeviceBatchLoader
    from kws.libs.models import DepthwiseSeparableConv

    torch.manual_seed(0)
    model = DepthwiseSeparableConv().to(dev).train()
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loader = DeviceBatchLoader.from_arrays(pcm, labels, ap, B, drop_last=True, seed=1)
    fixed_x, fixed_y = next(iter(loader))

    def batches():
        while True:
            yield from loader

    feed = batches()

    def step(x, y):
        opt.zero_grad()
        model._context(dev.index or 0)
        crit(model(x), y).backward()
        opt.step()

    def resident():
        step(fixed_x, fixed_y)

    def fed():
        step(*next(feed))

    for _ in range(warmup):
        resident(), fed()
    torch.cuda.synchronize()
    r, f = [], []
    for _ in range(iters):
        r.append(timed(resident))
        f.append(timed(fed))
    torch.cuda.synchronize()
    rm, fm = med([a.elapsed_time(b) for a, b in r]), med([a.elapsed_time(b) for a, b in f])
    return {"B": B, "resident_ms": rm, "loader_fed_ms": fm, "ratio": round(fm / rm, 4), "fused": loader.fused}


def main(argv=None):
    ap_ = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap_.add_argument("--batches", default="1028,4096")
    ap_.add_argument("--iters", type=int, default=60)
    ap_.add_argument("--warmup", type=int, default=10)
    ap_.add_argument("--clips", type=int, default=8192, help="uniform-noise clips of the resident split")
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loader_bench.json"))
    args = ap_.parse_args(argv)
    if args.iters < 50:
        ap_.error("--iters must be at least 50")
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader.py needs a GPU (there is no CPU fallback to time)")
    from kws.libs.audio_processor import AudioProcessor
    from speechlike import speechlike_set

    dev = torch.device("cuda", 0)
    ap = AudioProcessor(None)
    cfg = ap.config
    rng = np.random.default_rng(0)
    splits = {"uniform": rng.integers(-32768, 32768, size=(args.clips, N_SAMPLES), dtype=np.int16),
              "speechlike": speechlike_set(64)[0].astype(np.int16)}
    ctx = ap._context(N_SAMPLES, cfg.sample_rate, cfg.num_cepstral_coeffs, cfg.frame_length, cfg.frame_step, cfg.num_mel_filters)
    ctx.use_torch_stream()
    batches = [int(b) for b in args.batches.split(",")]
    res = {"tool": "bench_loader", "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "kernels": {}}
    for kind, clips in splits.items():
        pcm = torch.from_numpy(clips).to(dev)
        labels = torch.from_numpy(rng.integers(0, 12, len(clips)).astype(np.int32)).to(dev)
        res["kernels"][kind] = [kernels(ctx, dev, pcm, labels, B, args.iters, args.warmup, cfg, 17) for B in batches]
    res["host_draw_ms"] = {str(B): host_draw_ms(B, 50, cfg, dev) for B in batches}
    ap.background_data = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in BG_LENS]
    res["step"] = step_pair(dev, splits["uniform"], rng.integers(0, 12, args.clips), ap, 1028, args.iters, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
