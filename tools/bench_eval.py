#!/usr/bin/env python3
"""Time a validation epoch two ways on one GPU: the reference's loop and kws.libs.evaluation.evaluate().

The split is synthetic and resident (DeviceBatchLoader.from_arrays, batch 1028, augment=False), the model the DS-CNN.

  torch loop   forward, nn.CrossEntropyLoss, torch.max, two .item() per batch (Trainer.evaluate, train.py:79-98;
               KWSTrainer.validate, kws/libs/training.py:347-393)
  evaluate()   forward, kws_eval_update_f32 per batch, one read-back at the end -- with a fresh Evaluator per epoch (a native
               context is created and destroyed inside the timed window) and with one kept across epochs (evaluator=)

The three are alternated in one process; each epoch is timed with device events and with a host clock that ends in a device
synchronise; medians over --epochs epochs after --warmup epochs of each.  Both must report the same accuracy and the same
clip-mean loss within 1e-5.

Also: the stream time of one kws_eval_update_f32 at B = 1028 and 4096, with and without d_dlogits, and of the int64 -> int32
label cast beside it (device events around --calls back-to-back calls, divided by the count: launch gaps included).

    python tools/bench_eval.py [--clips 8224] [--epochs 30] [--warmup 5] [--calls 200] [--out profiles/eval_bench.json]

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

BATCH, C = 1028, 12


def timed(fn):
    """(result, device ms between two events, host ms ending in a synchronise) of one call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def torch_epoch(model, loader):
    """The reference's validation loop: (mean of the batch losses, clip-mean loss, accuracy in per cent)."""
    criterion = torch.nn.CrossEntropyLoss()
    model.eval()
    running, weighted, correct, total = 0.0, 0.0, 0, 0
    with torch.no_grad():
        for x, y in loader:
            out = model(x)
            loss = criterion(out, y)
            v = loss.item()
            running += v
            weighted += v * y.size(0)
            _, pred = torch.max(out, 1)
            total += y.size(0)
            correct += (pred == y).sum().item()
    return running / len(loader), weighted / total, 100.0 * correct / total


def stream_ms(fn, calls):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def update_times(dev, calls):
    from kws.libs.evaluation import Evaluator

    out = []
    rng = np.random.default_rng(0)
    for B in (1028, 4096):
        z = torch.from_numpy((rng.standard_normal((B, C)) * 5).astype(np.float32)).to(dev)
        y64 = torch.from_numpy(rng.integers(0, C, B)).to(dev)
        y32 = y64.to(torch.int32)
        ev = Evaluator(C, 256)
        ctx = ev._ctx
        dl = torch.empty_like(z)
        samples = {"update_ms": [], "update_dlogits_ms": [], "label_cast_ms": [], "evaluator_update_ms": []}
        for _ in range(5):  # alternated, median of five
            samples["update_ms"].append(stream_ms(lambda: ctx.eval_update_f32(z, y32), calls))
            samples["update_dlogits_ms"].append(stream_ms(lambda: ctx.eval_update_f32(z, y32, 1.0 / B, dl), calls))
            samples["label_cast_ms"].append(stream_ms(lambda: y64.to(torch.int32), calls))
            samples["evaluator_update_ms"].append(stream_ms(lambda: ev.update(z, y64), calls))
        rep = ev.report()
        assert rep.n_ignored == 0 and rep.n_nonfinite == 0 and rep.n % B == 0
        ev.close()
        out.append({"batch": B, "n_bins": 256, **{k: float(np.median(v)) for k, v in samples.items()}})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--clips", type=int, default=8 * BATCH)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a GPU (there is no CPU fallback to time)")
    from kws.libs.audio_processor import AudioProcessor
    from kws.libs.data_loader import DeviceBatchLoader
    from kws.libs.evaluation import evaluate
    from kws.libs.models import DepthwiseSeparableConv

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    pcm = np.clip(np.round(rng.standard_normal((args.clips, 16000)) * 3000.0), -32768, 32767).astype(np.int16)
    labels = rng.integers(0, C, args.clips)
    loader = DeviceBatchLoader.from_arrays(pcm, labels, AudioProcessor(None), BATCH, shuffle=False, augment=False)
    torch.manual_seed(0)
    model = DepthwiseSeparableConv(num_classes=C).to(dev)

    for _ in range(args.warmup):
        want = torch_epoch(model, loader)
        rep = evaluate(model, loader)
    assert rep.n == args.clips and abs(rep.accuracy - want[2]) < 1e-9 and abs(rep.loss - want[1]) <= 1e-5, (rep.loss, rep.accuracy, want)
    from kws.libs.evaluation import Evaluator

    kept = Evaluator(C, 256)
    assert evaluate(model, loader, evaluator=kept).confusion.sum() == args.clips
    t_dev, t_host, e_dev, e_host, k_dev, k_host = [], [], [], [], [], []
    for _ in range(args.epochs):
        for fn, dv, hv in ((lambda: torch_epoch(model, loader), t_dev, t_host), (lambda: evaluate(model, loader), e_dev, e_host),
                           (lambda: evaluate(model, loader, evaluator=kept), k_dev, k_host)):
            _, d, h = timed(fn)
            dv.append(d)
            hv.append(h)
    kept.close()
    med = lambda v: float(np.median(v))
    spread = lambda v: [float(np.min(v)), float(np.max(v))]
    res = {
        "tool": "bench_eval", "device": torch.cuda.get_device_name(0), "model": "ds-cnn", "clips": args.clips, "batch": BATCH,
        "batches_per_epoch": len(loader), "num_classes": C, "n_bins": 256, "epochs": args.epochs, "warmup": args.warmup,
        "torch_loop_epoch_ms": {"device_events": med(t_dev), "host_clock": med(t_host), "host_min_max": spread(t_host)},
        "evaluate_epoch_ms": {"device_events": med(e_dev), "host_clock": med(e_host), "host_min_max": spread(e_host)},
        "evaluate_kept_evaluator_epoch_ms": {"device_events": med(k_dev), "host_clock": med(k_host), "host_min_max": spread(k_host)},
        "evaluate_over_torch_loop": {"device_events": med(e_dev) / med(t_dev), "host_clock": med(e_host) / med(t_host)},
        "evaluate_kept_evaluator_over_torch_loop": {"device_events": med(k_dev) / med(t_dev), "host_clock": med(k_host) / med(t_host)},
        "agreement": {"accuracy_percent": rep.accuracy, "clip_mean_loss_evaluate": rep.loss, "clip_mean_loss_torch": want[1],
                      "batch_mean_loss_torch": want[0]},
        "update_calls": args.calls, "update": update_times(dev, args.calls),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
