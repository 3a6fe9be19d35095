#!/usr/bin/env python3
"""Digests of what the training back ends and the composed forward's stage dump compute, for comparing two builds of the library
bit for bit (GPU box): run it once per build (KWS_HIP_LIB selects one) and compare the lines.

    python tools/ab_train_bits.py [--out FILE]

Prints one JSON line: {"lib": path, "digests": {case: SHA-256 of the raw float32 / int32 bytes}} for
  dscnn_grad TxF B C        kws_dscnn_backward_f32, seeded inputs and oracle.dscnn.random_state, at map sizes with one tile and a
                            remainder, class counts 12 and 35, a batch with a short last clip group and one over the clip cap
  dscnn_layers / _logits    the stage dump and the logits of kws_forward_map_debug_f32
  cnntrad_grad B C          kws_cnn_trad_backward_f32 (one clip, a short last group, several clips per group, two chunks)
  cnntrad_debug_*           the four arrays of kws_cnn_trad_train_debug_f32
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "keyword-spotting_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DSCNN_GRAD = [(6, 6, 9, 12), (22, 20, 5, 12), (99, 10, 7, 12), (61, 13, 7, 35), (20, 8, 1025, 12), (6, 6, 16421, 12)]  # T, F, B, C
DSCNN_DUMP = [(22, 20, 5, 12), (61, 13, 7, 35)]
CNNTRAD_GRAD = [(1, 1), (33, 12), (1025, 64), (8195, 12)]  # B, C
CNNTRAD_DEBUG = (33, 12)


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ab_train_bits.py needs a GPU")
    from kws import _native
    from oracle import cnn_trad as o_ct
    from oracle import dscnn as o_ds

    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    ctx.use_torch_stream()
    out = {}

    def inputs(B, T, F, C, seed):
        gen = torch.Generator().manual_seed(seed)
        return torch.randn(B, 1, T, F, generator=gen).to(dev), (torch.randn(B, C, generator=gen) / B).to(dev)

    for T, F, B, C in DSCNN_GRAD:
        blob = o_ds.flatten_state(o_ds.random_state(T * 1000 + F + B, num_classes=C))
        ctx.load_dscnn(blob, C)
        x, dl = inputs(B, T, F, C, T + F + B)
        g = torch.full((blob.size,), float("nan"), device=dev)
        ctx.dscnn_backward_f32(x, T, F, dl, g)
        ctx.sync()
        out[f"dscnn_grad {T}x{F} B={B} C={C}"] = sha(g)
    for T, F, B, C in DSCNN_DUMP:
        ctx.load_dscnn(o_ds.flatten_state(o_ds.random_state(T * 1000 + F, num_classes=C)), C)
        x, _ = inputs(B, T, F, C, T + F)
        h1, w1 = (T - 6) // 2 + 1, (F - 6) // 2 + 1
        layers = torch.full((B * 64 * sum((h1 + 2 * k) * (w1 + 2 * k) for k in range(5)),), float("nan"), device=dev)
        logits = torch.empty((B, C), device=dev)
        ctx.forward_map_f32(x, logits, None, layers=layers)
        ctx.sync()
        out[f"dscnn_layers {T}x{F} B={B} C={C}"] = sha(layers)
        out[f"dscnn_logits {T}x{F} B={B} C={C}"] = sha(logits)
    for B, C in CNNTRAD_GRAD:
        blob = o_ct.flatten_state(o_ct.random_state(B + C, num_classes=C))
        ctx.load_cnn_trad(blob, C)
        x, dl = inputs(B, 99, 10, C, B + C)
        g = torch.full((blob.size,), float("nan"), device=dev)
        ctx.cnn_trad_backward_f32(x, dl, g)
        ctx.sync()
        out[f"cnntrad_grad B={B} C={C}"] = sha(g)
        del x, dl, g
    B, C = CNNTRAD_DEBUG
    ctx.load_cnn_trad(o_ct.flatten_state(o_ct.random_state(B + C, num_classes=C)), C)
    x, _ = inputs(B, 99, 10, C, B + C)
    conv1 = torch.full((B, 64, 99, 10), float("nan"), device=dev)
    winner = torch.full((B, 64, 99, 3), -1, dtype=torch.int32, device=dev)
    conv2 = torch.full((B, 64, 99, 3), float("nan"), device=dev)
    hidden = torch.full((B, 160), float("nan"), device=dev)
    ctx.cnn_trad_train_debug_f32(x, conv1, winner, conv2, hidden)
    ctx.sync()
    for name, t in (("conv1", conv1), ("winner", winner), ("conv2", conv2), ("hidden", hidden)):
        out[f"cnntrad_debug_{name} B={B} C={C}"] = sha(t)
    ctx.close()
    line = json.dumps({"tool": "ab_train_bits", "lib": _native.LIB_PATH, "digests": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
