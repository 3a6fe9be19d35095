#!/usr/bin/env python3
"""Training benchmark (GPU box): the reference trainer's step on DepthwiseSeparableConv at 99 x 10 features --
zero_grad -> forward -> CrossEntropyLoss -> loss.backward() -> Adam(lr=1e-3) (train.py:39-49, kws/libs/training.py:286-297)
-- with the HIP model (forward kernels + kws_dscnn_backward_f32), against the same step in torch-ROCm eager on the same GPU
(oracle.dscnn.forward with the parameters on the GPU, autograd, Adam), alternated step by step in one process.

    python tools/bench_train.py [--batches 1028,4096] [--steps 60] [--warmup 10] [--out FILE]
    python tools/bench_train.py --backward-only --batches 1028     # only the kws_dscnn_backward_f32 loop (for rocprofv3)
    python tools/bench_train.py --model cnn-trad-fpool3 [--batches 1024,4096]   # the same step on CnnTradFpool3
                                   (oracle.cnn_trad.forward for torch eager; kws_cnn_trad_backward_f32; --backward-only as above)
    python tools/bench_train.py --model ds-cnn-bn [--batches 1028,4096] --out profiles/train_bn_bench.json
                                   the same step on DepthwiseSeparableConvBN in train mode (kws_dscnn_bn_train_forward_f32 +
                                   kws_dscnn_bn_backward_f32, batch statistics, running statistics updated) against torch eager on an
                                   unfolded nn definition of the same model (nn.Conv2d / nn.BatchNorm2d in train mode);
                                   --backward-only loops kws_dscnn_bn_backward_f32 alone

Prints one JSON line.  Per batch size B:
  hip.step_ms            device-event time of a whole step (median, p10, p90 over --steps steps), clips/s at the median
  hip.split_ms           medians of the phases of the same steps: refresh (the parameters re-uploaded after the optimizer
                         step, DepthwiseSeparableConv._context), forward, backward (CrossEntropyLoss + loss.backward(), whose
                         work is kws_dscnn_backward_f32), optimizer (Adam.step)
  backward_call_ms       kws_dscnn_backward_f32 alone (ctypes call on the same inputs, device events, median)
  backward_gflop         algorithmic FLOPs of the call, from the shapes: the recomputed forward (conv1, 4 x depthwise +
                         pointwise) and the backward (pointwise: two 64 x 64 GEMMs per block; depthwise: weight and input
                         gradients; conv1: weight gradient; fc), 2 FLOP per multiply-add
  backward_tflops, backward_peak_frac   backward_gflop over backward_call_ms, and that over the 157.3 TF f32 matrix peak
  torch_eager.step_ms    the eager step (median, p10, p90), clips/s
  speedup                torch eager median / HIP median
  hip.refresh_host_ms    the same refresh through the host (packed_weights() + the host load, device events around the call,
                         median), measured in the same run: what the refresh costs without the device-side load
  hip.host_route         (ds-cnn) step_ms and split_ms of the same steps with the model's refresh switched to the host route
                         (DepthwiseSeparableConv._device_refresh = False), run after the device-route steps in the same process
With --model cnn-trad-fpool3 the result also carries the model name and
backward_bf16_split_floor_ms (backward_gflop at the 2.5 PF dense bf16 rate over the six products of the exact split).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "keyword-spotting_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F32_MATRIX_PEAK_TF = 157.3
T_IN, F_IN, C = 99, 10, 12


def backward_flops(B, T=T_IN, F=F_IN, num_classes=C):
    """Algorithmic FLOPs of kws_dscnn_backward_f32 for B clips of T x F: recompute + backward."""
    h1, w1 = (T - 6) // 2 + 1, (F - 6) // 2 + 1
    p0 = h1 * w1
    pk = [(h1 + 2 * k) * (w1 + 2 * k) for k in range(4)]
    q4 = (h1 + 8) * (w1 + 8)
    fwd = 2 * 64 * 100 * p0 + sum(2 * 64 * 9 * p + 2 * 64 * 64 * p for p in pk) + 64 * q4 + 2 * num_classes * 64
    bwd = (2 * 2 * num_classes * 64                        # fc: weight gradient, dpool
           + sum(2 * (2 * 64 * 64 * p) for p in pk)        # pointwise: g_w = dZ X^T, dX = W^T dZ
           + sum(2 * (2 * 64 * 9 * p) for p in pk)         # depthwise: g_w, dX_in
           + 2 * 64 * 100 * p0)                            # conv1: g_w
    return B * (fwd + bwd)


def cnntrad_forward_macs(num_classes=C):
    """Multiply-adds of one cnn-trad-fpool3 forward per clip: conv1, conv2, lin, dnn, fc."""
    return 64 * 990 * 160 + 64 * 297 * 2560 + 19008 * 32 + 32 * 128 + 128 * num_classes


def cnntrad_backward_flops(B, num_classes=C):
    """Algorithmic FLOPs of kws_cnn_trad_backward_f32 for B clips: the recompute (the forward without fc) and the backward --
    fc and dnn (input and weight gradients), lin (dy2 and g_lin.w), conv2 (weight and input gradients), conv1's weight gradient
    over the 297 pool winners per channel -- 2 FLOP per multiply-add."""
    rec = cnntrad_forward_macs(num_classes) - 128 * num_classes
    bwd = 2 * 128 * num_classes + 2 * 32 * 128 + 2 * 19008 * 32 + 2 * 64 * 297 * 2560 + 64 * 297 * 160
    return 2 * B * (rec + bwd)


def stats(xs):
    a = np.asarray(xs)
    return {"median": round(float(np.median(a)), 4), "p10": round(float(np.percentile(a, 10)), 4),
            "p90": round(float(np.percentile(a, 90)), 4)}


def backward_calls(ctx, x, dl, grad, n):
    evs = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.dscnn_backward_f32(x, T_IN, F_IN, dl, grad)
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def run(B, steps, warmup, dev, backward_only=False):
    from kws.libs.models import DepthwiseSeparableConv
    from oracle import dscnn as o_dscnn

    torch.manual_seed(0)
    model = DepthwiseSeparableConv().to(dev).train()   # as the reference trainer does every epoch
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, 1, T_IN, F_IN, generator=gen).to(dev)
    y = torch.randint(0, C, (B,), generator=gen).to(dev)
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    st = {k: v.clone().requires_grad_(True) for k, v in init.items()}
    opt_t = torch.optim.Adam(list(st.values()), lr=1e-3)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    if backward_only:
        ctx = model._context(dev.index or 0)
        dl = torch.randn(B, C, generator=gen).to(dev) / B
        grad = torch.empty(sum(p.numel() for p in model.parameters()), dtype=torch.float32, device=dev)
        backward_calls(ctx, x, dl, grad, warmup)
        call_ms = stats(backward_calls(ctx, x, dl, grad, steps))
        return {"B": B, "backward_call_ms": call_ms, "backward_gflop": round(backward_flops(B) / 1e9, 3)}

    def hip_step():
        e = [ev() for _ in range(5)]
        e[0].record()
        opt.zero_grad()
        model._context(dev.index or 0)   # refresh: re-uploads the parameters the last optimizer step changed
        e[1].record()
        logits = model(x)
        e[2].record()
        crit(logits, y).backward()
        e[3].record()
        opt.step()
        e[4].record()
        return e

    def torch_step():
        e = [ev(), ev()]
        e[0].record()
        opt_t.zero_grad()
        crit(o_dscnn.forward(st, x), y).backward()
        opt_t.step()
        e[1].record()
        return e

    names = ["refresh", "forward", "backward", "optimizer"]

    def timed_steps():
        for _ in range(warmup):
            hip_step()
            torch_step()
        torch.cuda.synchronize()
        hip_ev, t_ev = [], []
        for _ in range(steps):  # alternated: both see the same clocks and neighbours
            hip_ev.append(hip_step())
            t_ev.append(torch_step())
        torch.cuda.synchronize()
        return ([e[0].elapsed_time(e[4]) for e in hip_ev],
                {name: stats([e[i].elapsed_time(e[i + 1]) for e in hip_ev])["median"] for i, name in enumerate(names)},
                [e[0].elapsed_time(e[1]) for e in t_ev])

    step, split, t_step = timed_steps()
    # the same steps with the refresh through the host (packed_weights() + kws_load_dscnn), as before kws_load_dscnn_device
    model._device_refresh = False
    host_step, host_split, _ = timed_steps()
    del model._device_refresh
    ctx = model._context(dev.index or 0)
    host = []
    for _ in range(max(10, steps // 5)):  # and that refresh alone
        a, b = ev(), ev()
        a.record()
        ctx.load_dscnn(model.packed_weights(), C)
        b.record()
        torch.cuda.synchronize()
        host.append(a.elapsed_time(b))
    model.sync_weights()

    # the C call alone, on the same inputs
    ctx = model._context(dev.index or 0)
    dl = torch.randn(B, C, generator=gen).to(dev) / B
    grad = torch.empty(sum(p.numel() for p in model.parameters()), dtype=torch.float32, device=dev)
    backward_calls(ctx, x, dl, grad, warmup)
    call_ms = stats(backward_calls(ctx, x, dl, grad, steps))
    gflop = backward_flops(B) / 1e9
    tflops = gflop / call_ms["median"]
    hs, ts = stats(step), stats(t_step)
    return {
        "B": B,
        "hip": {"step_ms": hs, "clips_per_s": round(B / hs["median"] * 1e3), "split_ms": split,
                "refresh_host_ms": stats(host)["median"], "host_route": {"step_ms": stats(host_step), "split_ms": host_split}},
        "backward_call_ms": call_ms,
        "backward_gflop": round(gflop, 3),
        "backward_tflops": round(tflops, 3),
        "backward_peak_frac": round(tflops / F32_MATRIX_PEAK_TF, 4),
        "torch_eager": {"step_ms": ts, "clips_per_s": round(B / ts["median"] * 1e3)},
        "speedup": round(ts["median"] / hs["median"], 3),
    }


BF16_MATRIX_PEAK_TF = 2516.6


def run_cnntrad(B, steps, warmup, dev, backward_only=False):
    from kws.libs.models import CnnTradFpool3
    from oracle import cnn_trad as o_ct

    torch.manual_seed(0)
    model = CnnTradFpool3().to(dev).train()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, 1, T_IN, F_IN, generator=gen).to(dev)
    y = torch.randint(0, C, (B,), generator=gen).to(dev)
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    st = {k: v.clone().requires_grad_(True) for k, v in init.items()}
    opt_t = torch.optim.Adam(list(st.values()), lr=1e-3)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def calls(ctx, dl, grad, n):
        evs = []
        for _ in range(n):
            a, b = ev(), ev()
            a.record()
            ctx.cnn_trad_backward_f32(x, dl, grad)
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in evs]

    gflop = cnntrad_backward_flops(B) / 1e9
    ctx = model._context(dev.index or 0)
    dl = torch.randn(B, C, generator=gen).to(dev) / B
    grad = torch.empty(sum(p.numel() for p in model.parameters()), dtype=torch.float32, device=dev)
    if backward_only:
        calls(ctx, dl, grad, warmup)
        return {"B": B, "backward_call_ms": stats(calls(ctx, dl, grad, steps)), "backward_gflop": round(gflop, 3)}

    def hip_step():
        e = [ev() for _ in range(5)]
        e[0].record()
        opt.zero_grad()
        model._context(dev.index or 0)   # refresh: the device load of the parameters the last optimizer step changed
        e[1].record()
        logits = model(x)
        e[2].record()
        crit(logits, y).backward()
        e[3].record()
        opt.step()
        e[4].record()
        return e

    def torch_step():
        e = [ev(), ev()]
        e[0].record()
        opt_t.zero_grad()
        crit(o_ct.forward(st, x), y).backward()
        opt_t.step()
        e[1].record()
        return e

    for _ in range(warmup):
        hip_step()
        torch_step()
    torch.cuda.synchronize()
    hip_ev, t_ev = [], []
    for _ in range(steps):
        hip_ev.append(hip_step())
        t_ev.append(torch_step())
    torch.cuda.synchronize()
    step = [e[0].elapsed_time(e[4]) for e in hip_ev]
    split = {name: stats([e[i].elapsed_time(e[i + 1]) for e in hip_ev])["median"]
             for i, name in enumerate(["refresh", "forward", "backward", "optimizer"])}
    t_step = [e[0].elapsed_time(e[1]) for e in t_ev]
    # the refresh through the host load, as before kws_load_cnn_trad_device
    host = []
    for _ in range(max(10, steps // 5)):
        a, b = ev(), ev()
        a.record()
        ctx.load_cnn_trad(model.packed_weights(), C)
        b.record()
        torch.cuda.synchronize()
        host.append(a.elapsed_time(b))
    model.sync_weights()
    ctx = model._context(dev.index or 0)
    calls(ctx, dl, grad, warmup)
    call_ms = stats(calls(ctx, dl, grad, steps))
    tflops = gflop / call_ms["median"]
    hs, ts = stats(step), stats(t_step)
    return {
        "B": B,
        "hip": {"step_ms": hs, "clips_per_s": round(B / hs["median"] * 1e3), "split_ms": split,
                "refresh_host_ms": stats(host)["median"]},
        "backward_call_ms": call_ms,
        "backward_gflop": round(gflop, 3),
        "backward_tflops": round(tflops, 3),
        "backward_peak_frac": round(tflops / F32_MATRIX_PEAK_TF, 4),
        "backward_f32_floor_ms": round(gflop / F32_MATRIX_PEAK_TF, 3),
        "backward_bf16_split_floor_ms": round(6 * gflop / BF16_MATRIX_PEAK_TF, 3),
        "torch_eager": {"step_ms": ts, "clips_per_s": round(B / ts["median"] * 1e3)},
        "speedup": round(ts["median"] / hs["median"], 3),
    }


class EagerDscnnBN(torch.nn.Module):
    """DepthwiseSeparableConvBN unfolded, as plain torch modules: what a user trains in eager mode to obtain a BatchNorm checkpoint."""

    def __init__(self, num_classes=C, eps=1e-5):
        super().__init__()
        nn = torch.nn
        self.conv1, self.bn_conv1 = nn.Conv2d(1, 64, 10, stride=2, padding=2), nn.BatchNorm2d(64, eps=eps)
        self.dw = nn.ModuleList([nn.Conv2d(64, 64, 3, padding=1, groups=64) for _ in range(4)])
        self.pw = nn.ModuleList([nn.Conv2d(64, 64, 1, padding=1) for _ in range(4)])
        self.bn_dw = nn.ModuleList([nn.BatchNorm2d(64, eps=eps) for _ in range(4)])
        self.bn_pw = nn.ModuleList([nn.BatchNorm2d(64, eps=eps) for _ in range(4)])
        self.fc = nn.Linear(64, num_classes)

    def forward(self, x):
        h = torch.relu(self.bn_conv1(self.conv1(x)))
        for k in range(4):
            h = self.bn_dw[k](self.dw[k](h))
            h = torch.relu(self.bn_pw[k](self.pw[k](h)))
        return self.fc(h.mean(dim=(2, 3)))

    def load_from(self, model):
        """The parameters of a DepthwiseSeparableConvBN, tensor by tensor."""
        with torch.no_grad():
            pairs = [(self.conv1, model.plain.conv1), (self.fc, model.plain.fc), (self.bn_conv1, model.bn_conv1)]
            for k in range(4):
                blk = getattr(model.plain, f"dsconv{k + 1}")
                pairs += [(self.dw[k], blk.depthwise), (self.pw[k], blk.pointwise), (self.bn_dw[k], model.bn_dw[k]), (self.bn_pw[k], model.bn_pw[k])]
            for mine, theirs in pairs:
                mine.weight.copy_(theirs.weight)
                mine.bias.copy_(theirs.bias)
        return self


def run_bn(B, steps, warmup, dev, backward_only=False):
    from kws.libs.models import DepthwiseSeparableConvBN

    torch.manual_seed(0)
    model = DepthwiseSeparableConvBN().to(dev).train()
    with torch.no_grad():  # off the default init's degenerate point (every beta and bias zero puts the rings on the ReLU threshold)
        for name, p in model.named_parameters():
            if name.startswith("bn_") or name.endswith("bias"):
                p.add_(torch.randn_like(p) * 0.1)
    eager = EagerDscnnBN().load_from(model).to(dev).train()
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, 1, T_IN, F_IN, generator=gen).to(dev)
    y = torch.randint(0, C, (B,), generator=gen).to(dev)
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt_t = torch.optim.Adam(eager.parameters(), lr=1e-3)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def calls(n):
        ctx, blob = model._train_context(dev.index or 0)
        evs = []
        for _ in range(n):
            a, b = ev(), ev()
            a.record()
            ctx.dscnn_bn_backward_f32(blob, C, x, model._eps(), dl, grad)
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in evs]

    dl = torch.randn(B, C, generator=gen).to(dev) / B
    grad = torch.empty(sum(p.numel() for p in model.parameters()), dtype=torch.float32, device=dev)
    if backward_only:
        calls(warmup)
        return {"B": B, "backward_call_ms": stats(calls(steps))}

    def hip_step():
        e = [ev() for _ in range(4)]
        e[0].record()
        opt.zero_grad()
        logits = model(x)
        e[1].record()
        crit(logits, y).backward()
        e[2].record()
        opt.step()
        e[3].record()
        return e

    def torch_step():
        e = [ev(), ev()]
        e[0].record()
        opt_t.zero_grad()
        crit(eager(x), y).backward()
        opt_t.step()
        e[1].record()
        return e

    for _ in range(warmup):
        hip_step()
        torch_step()
    torch.cuda.synchronize()
    hip_ev, t_ev = [], []
    for _ in range(steps):  # alternated: both see the same clocks and neighbours
        hip_ev.append(hip_step())
        t_ev.append(torch_step())
    torch.cuda.synchronize()
    step = [e[0].elapsed_time(e[3]) for e in hip_ev]
    split = {name: stats([e[i].elapsed_time(e[i + 1]) for e in hip_ev])["median"]
             for i, name in enumerate(["forward", "backward", "optimizer"])}
    t_step = [e[0].elapsed_time(e[1]) for e in t_ev]
    calls(warmup)
    call_ms = stats(calls(steps))
    hs, ts = stats(step), stats(t_step)
    return {
        "B": B,
        "hip": {"step_ms": hs, "clips_per_s": round(B / hs["median"] * 1e3), "split_ms": split},
        "backward_call_ms": call_ms,
        "torch_eager": {"step_ms": ts, "clips_per_s": round(B / ts["median"] * 1e3)},
        "speedup": round(ts["median"] / hs["median"], 3),
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="ds-cnn", choices=["ds-cnn", "cnn-trad-fpool3", "ds-cnn-bn"])
    ap.add_argument("--batches", default=None, help="comma-separated batch sizes (default 1028,4096; cnn-trad-fpool3: 1024,4096)")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--backward-only", action="store_true", help="time only the model's backward entry")
    args = ap.parse_args(argv)
    if args.steps < 50:
        ap.error("--steps must be at least 50")
    if not torch.cuda.is_available():
        raise SystemExit("bench_train.py needs a GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda", 0)
    cnntrad = args.model == "cnn-trad-fpool3"
    batches = args.batches or ("1024,4096" if cnntrad else "1028,4096")
    fn = run_cnntrad if cnntrad else run_bn if args.model == "ds-cnn-bn" else run
    res = {"tool": "bench_train", "device": torch.cuda.get_device_name(0), "features": [1, T_IN, F_IN], "num_classes": C,
           "steps": args.steps, "warmup": args.warmup, "f32_matrix_peak_tf": F32_MATRIX_PEAK_TF}
    if args.model != "ds-cnn":
        res = {"tool": "bench_train", "model": args.model, **{k: v for k, v in res.items() if k != "tool"}}
    res["results"] = [fn(int(b), args.steps, args.warmup, dev, args.backward_only) for b in batches.split(",")]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
