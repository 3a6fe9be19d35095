"""cnn-trad-fpool3 restated with PINNED decisions, for gradient tests of kws_cnn_trad_backward_f32 (test helper, not a test).

``oracle.cnn_trad.forward`` with its three ReLUs and its max-pool replaced by fixed decisions: a ReLU with the mask ``m`` is
``z * m``, the 1x3 pool with the winners ``w`` (0..2 within each window of bins 3j..3j+2) is a ``gather``.  Pinned to the GPU's
own decisions (``kws_cnn_trad_train_debug_f32``), a float64 reference cannot disagree with the GPU about a value that lies within
rounding of zero or of a tie.  Pinned to its own decisions (``own_pins``) it is the unpinned model, the first maximum winning a
tie as in torch's ``max_pool2d``.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn_trad as o_ct


def keys(num_classes=12):
    return list(o_ct.state_shapes(num_classes))


def _z1(state, x):
    return F.conv2d(F.pad(x, (3, 4, 9, 10)), state["conv1.weight"], state["conv1.bias"])


def _pool(y1, winner):
    """y1 [B,64,99,10], winner int64 [B,64,99,3] -> y1 at bin 3j + winner[..., j]."""
    idx = winner + torch.arange(3, device=winner.device).mul(3)
    return torch.gather(y1[..., :9], 3, idx)


def forward(state, x, pins):
    """logits of the pinned model; pins = dict(m1 [B,64,99,10], winner [B,64,99,3], m2 [B,64,99,3], md [B,128]) (masks 0/1)."""
    y1 = _z1(state, x) * pins["m1"]
    yp = _pool(y1, pins["winner"])
    y2 = F.conv2d(F.pad(yp, (1, 2, 4, 5)), state["conv2.weight"], state["conv2.bias"]) * pins["m2"]
    h = F.linear(y2.flatten(1), state["lin.weight"], state["lin.bias"])
    d = F.linear(h, state["dnn.weight"], state["dnn.bias"]) * pins["md"]
    return F.linear(d, state["fc.weight"], state["fc.bias"]), {"conv1": y1, "pool": yp, "conv2": y2, "lin": h, "dnn": d}


@torch.no_grad()
def own_pins(state, x):
    """The decisions of the unpinned model on x: ReLU masks where the pre-activation is > 0, the first maximum of each window."""
    z1 = _z1(state, x)
    y1 = F.relu(z1)
    winner = torch.argmax(y1[..., :9].reshape(*y1.shape[:3], 3, 3), dim=-1)  # first maximal index
    yp = _pool(y1, winner)
    z2 = F.conv2d(F.pad(yp, (1, 2, 4, 5)), state["conv2.weight"], state["conv2.bias"])
    h = F.linear(F.relu(z2).flatten(1), state["lin.weight"], state["lin.bias"])
    zd = F.linear(h, state["dnn.weight"], state["dnn.bias"])
    return {"m1": (z1 > 0).to(x.dtype), "winner": winner, "m2": (z2 > 0).to(x.dtype), "md": (zd > 0).to(x.dtype)}


def gpu_pins(conv1, winner, conv2, hidden, dtype=torch.float64):
    """Pins from the GPU's stages (CPU tensors): conv1 / conv2 after ReLU, winners, [h | d]."""
    return {"m1": (conv1 > 0).to(dtype), "winner": winner.to(torch.int64), "m2": (conv2 > 0).to(dtype),
            "md": (hidden[:, 32:] > 0).to(dtype)}


def grads(state, x, dl, pins, dtype=torch.float64):
    """d(sum(logits * dl)) / d(state) of the pinned model in ``dtype`` on the CPU, as NumPy arrays in state_dict order."""
    st = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    p = {k: (v.to(dtype) if k != "winner" else v) for k, v in pins.items()}
    logits, _ = forward(st, x.to(dtype), p)
    (logits * dl.to(dtype)).sum().backward()
    return {k: st[k].grad.numpy() for k in keys(state["fc.bias"].numel())}
