"""The train-mode BatchNorm DS-CNN restated in torch on the CPU, in float64 (the answer) or float32 (the yardstick of torch-f32's
own error), for tests/test_dscnn_bn_train_cpu.py and tests/test_dscnn_bn_train_gpu.py.

    z0 = conv1(x) + b                a0  = relu(BN(z0))
    z  = depthwise_k(a_{k-1}) + b    u   = BN(z)            (no ReLU)
    z  = pointwise_k(u) + b          a_k = relu(BN(z))      (padding 1: the ring equals the bias and counts in the statistics)
    logits = fc(mean of a_4 over all positions)

BN(z)_c = gamma_c (z - mean_c) / sqrt(var_c + eps) + beta_c with the mean and the BIASED variance over batch and positions.
Parameters travel as a dict keyed by ``DepthwiseSeparableConvBN.named_parameters()`` names, in that order.  ``masks`` (five bool
tensors, a0 .. a4) pins the ReLU decisions: relu(y) becomes where(mask, y, 0), so a comparison against another arithmetic measures
rounding only, never a unit switched on one side and off on the other."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ["conv1"] + [f"{p}{k}" for k in range(1, 5) for p in ("dw", "pw")]  # data-flow order, the order of d_stats
BN_OF = {"conv1": "bn_conv1", **{f"dw{k}": f"bn_dw.{k - 1}" for k in range(1, 5)}, **{f"pw{k}": f"bn_pw.{k - 1}" for k in range(1, 5)}}
CONV_OF = {"conv1": "plain.conv1", **{f"dw{k}": f"plain.dsconv{k}.depthwise" for k in range(1, 5)},
           **{f"pw{k}": f"plain.dsconv{k}.pointwise" for k in range(1, 5)}}


def param_shapes(num_classes=12):
    """name -> shape, in ``DepthwiseSeparableConvBN.parameters()`` order."""
    s = OrderedDict()
    s["plain.conv1.weight"], s["plain.conv1.bias"] = (64, 1, 10, 10), (64,)
    for k in range(1, 5):
        s[f"plain.dsconv{k}.depthwise.weight"], s[f"plain.dsconv{k}.depthwise.bias"] = (64, 1, 3, 3), (64,)
        s[f"plain.dsconv{k}.pointwise.weight"], s[f"plain.dsconv{k}.pointwise.bias"] = (64, 64, 1, 1), (64,)
    s["plain.fc.weight"], s["plain.fc.bias"] = (num_classes, 64), (num_classes,)
    for mod in ["bn_conv1"] + [f"bn_dw.{i}" for i in range(4)] + [f"bn_pw.{i}" for i in range(4)]:
        s[f"{mod}.weight"], s[f"{mod}.bias"] = (64,), (64,)
    return s


def random_params(seed, num_classes=12):
    """Seeded float32 parameters: He-scaled convolution weights, biases ~ N(0, 0.1) (rings neither 0 nor equal), gamma = 1 +- 0.3,
    beta = +- 0.3 (uniform), fc.weight ~ N(0, 0.3)."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for name, shp in param_shapes(num_classes).items():
        if name.startswith("bn_"):
            v = (1.0 if name.endswith("weight") else 0.0) + rs.uniform(-0.3, 0.3, shp)
        elif name.endswith("bias"):
            v = rs.standard_normal(shp) * 0.1
        elif name == "plain.fc.weight":
            v = rs.standard_normal(shp) * 0.3
        else:
            v = rs.standard_normal(shp) * (2.0 / np.prod(shp[1:])) ** 0.5
        out[name] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return out


def flatten(params):
    """The blob of the C entries: every tensor in order, float32."""
    return np.concatenate([np.asarray(v.detach(), dtype=np.float32).reshape(-1) for v in params.values()])


def forward(params, x, eps=1e-5, masks=None, keep=None):
    """-> (logits, [a0 .. a4], stats [9, 2, 64]: batch mean and UNBIASED batch variance per layer); dtype follows ``x``.
    ``keep`` (a dict) receives every BatchNorm output before its ReLU under the layer's name, and 1 / sigma under name + '.rstd'."""
    p = {k: v.to(x.dtype) for k, v in params.items()}
    stats, acts = [], []

    def bn(z, layer):
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        n = z.numel() // z.shape[1]
        stats.append(torch.stack([mean.detach(), var.detach() * (n / (n - 1))]))
        rstd = 1.0 / torch.sqrt(var + eps)
        y = (z - mean[None, :, None, None]) * rstd[None, :, None, None]
        y = y * p[BN_OF[layer] + ".weight"][None, :, None, None] + p[BN_OF[layer] + ".bias"][None, :, None, None]
        if keep is not None:
            keep[layer], keep[layer + ".rstd"] = y, rstd.detach()
        return y

    def relu(y):
        if masks is None:
            a = F.relu(y)
        else:
            m = masks[len(acts)]
            assert m.shape == y.shape, (m.shape, y.shape)
            a = torch.where(m, y, y.new_zeros(()))
        acts.append(a)
        return a

    def conv(h, layer, **kw):
        return F.conv2d(h, p[CONV_OF[layer] + ".weight"], p[CONV_OF[layer] + ".bias"], **kw)

    h = relu(bn(conv(x, "conv1", stride=2, padding=2), "conv1"))
    for k in range(1, 5):
        h = bn(conv(h, f"dw{k}", padding=1, groups=64), f"dw{k}")
        h = relu(bn(conv(h, f"pw{k}", padding=1), f"pw{k}"))
    logits = F.linear(h.mean(dim=(2, 3)), p["plain.fc.weight"], p["plain.fc.bias"])
    return logits, acts, torch.stack(stats)


def grads(params, x, dlogits, dtype, eps=1e-5, masks=None):
    """Gradient of sum(logits * dlogits) with respect to every parameter, by torch autograd in ``dtype`` -> ({name: float64
    array}, {layer: magnitude of what cancels in the convolution bias's gradient = max_c |gamma_c| / sigma_c * sum |dy^_c|})."""
    st = OrderedDict((k, v.detach().to(dtype).requires_grad_(True)) for k, v in params.items())
    keep = {}
    logits, _, _ = forward(st, x.to(dtype), eps, masks, keep)
    for layer in LAYERS:
        keep[layer].retain_grad()
    logits.backward(dlogits.to(dtype))
    g = {k: v.grad.detach().to(torch.float64).numpy() for k, v in st.items()}
    cancels = {}
    for layer in LAYERS:
        dy = keep[layer].grad.abs().sum(dim=(0, 2, 3))  # already masked where a ReLU follows
        cancels[layer] = float((st[BN_OF[layer] + ".weight"].detach().abs() * keep[layer + ".rstd"] * dy).max())
    return g, cancels


def gate(got, ref32, ref64, floor=None):
    """The project's idiom: (error of ``got``, its bound 4 max|ref32 - ref64| + 1e-6 max|ref64|, or + ``floor`` where one is given)."""
    got, ref32, ref64 = (np.asarray(v, dtype=np.float64) for v in (got, ref32, ref64))
    err = float(np.abs(got - ref64).max())
    return err, 4.0 * float(np.abs(ref32 - ref64).max()) + (1e-6 * float(np.abs(ref64).max()) if floor is None else floor)
