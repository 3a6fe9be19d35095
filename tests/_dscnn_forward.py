"""DS-CNN forward helpers shared by the GPU tests of the composed and the fused paths (tests/test_dscnn_geometry_gpu.py,
tests/test_dscnn_multichannel_gpu.py): the stage-dump reader of kws_forward_map_debug_f32, the stage-by-stage check against the
float64 oracle, and the model whose float64 labels reach every 16-lane row of the fused kernel's classifier wavefront.  Every
helper takes the input channel count from the model's conv1.weight, so one set of rules serves input_channels == 1 and > 1."""
import numpy as np
import torch

from oracle import dscnn as o_dscnn

DEV = torch.device("cuda", 0)
TOL = 1e-4          # logits, as tests/test_gpu_parity.py
LAYER_RTOL = 2e-5   # stage outputs: max abs error <= LAYER_RTOL * max |float64 stage|, as tests/test_gpu_parity.py


def geometry(T, F):
    H1, W1 = (T - 6) // 2 + 1, (F - 6) // 2 + 1
    return [(64, H1 + 2 * k, W1 + 2 * k) for k in range(5)]


def in_channels(state):
    return int(state["conv1.weight"].shape[1])


def load_state(ctx, state, device=False):
    """kws_load_dscnn (or, ``device``, kws_load_dscnn_device) of ``state``: classes from fc.weight, channels from conv1.weight."""
    C, cin = int(state["fc.weight"].shape[0]), in_channels(state)
    blob = o_dscnn.flatten_state(state)
    if device:
        ctx.load_dscnn_device(torch.from_numpy(blob).to(DEV), C, cin)
    else:
        ctx.load_dscnn(blob, C, cin)
    return C


def gpu_forward(ctx, x, C):
    """kws_forward_map_debug_f32 (the composed path the backward recomputes with) -> logits, labels, {stage: output} on the
    CPU.  The stage buffer is NaN-filled before the call: a float never written stays NaN."""
    B, _, T, F = x.shape
    shapes = geometry(T, F)
    sizes = [int(np.prod(s)) for s in shapes]
    layers = torch.full((B * sum(sizes),), float("nan"), device=DEV)
    logits = torch.empty((B, C), device=DEV)
    labels = torch.empty((B,), dtype=torch.int32, device=DEV)
    ctx.forward_map_f32(x, logits, labels, layers=layers)
    ctx.sync()
    stages, off = {}, 0
    for name, shp, n in zip(o_dscnn.MASKED, shapes, sizes):
        stages[name] = layers[off:off + B * n].reshape(B, *shp).cpu()
        off += B * n
    return logits.cpu(), labels.cpu(), stages


def check_forward(ctx, state, x, what):
    """Load ``state`` and hold the composed path to the float64 oracle: every stage within LAYER_RTOL of the stage's largest
    value, the relu(bias) ring bit-exact, logits within TOL, labels wherever the float64 top-2 margin exceeds TOL, and the
    product entry (no stage dump) bit-identical to the debug entry.  Returns (logits, labels, stages, float64 logits)."""
    C = load_state(ctx, state)
    logits, labels, stages = gpu_forward(ctx, x.to(DEV), C)
    want, layers = o_dscnn.forward(state, x.double(), return_layers=True)
    for k in o_dscnn.MASKED:
        w, got = layers[k].numpy(), stages[k].double().numpy()
        assert got.shape == w.shape, (what, k)
        assert np.abs(got - w).max() <= LAYER_RTOL * np.abs(w).max(), f"{what} stage {k}"
        if k != "conv1":  # the ring is relu(bias) exactly
            assert np.array_equal(got[:, :, 0, :], w[:, :, 0, :]) and np.array_equal(got[:, :, :, -1], w[:, :, :, -1]), (what, k)
    want = want.numpy()
    assert np.abs(logits.double().numpy() - want).max() <= TOL, what
    top = np.sort(want, axis=1)
    sure = (top[:, -1] - top[:, -2] > TOL) if C > 1 else np.ones(len(want), bool)
    assert np.array_equal(labels.numpy()[sure], want.argmax(axis=1)[sure]), what
    # the product entry (no stage dump) gives the same bits
    l2 = torch.empty((x.shape[0], C), device=DEV)
    ctx.forward_map_f32(x.to(DEV), l2, None)
    ctx.sync()
    if tuple(x.shape[2:]) != (99, 10):  # 99 x 10 takes the fused kernel there (checked in the fused kernels' own tests)
        assert torch.equal(l2.cpu(), logits), what
    return logits, labels, stages, want


def he_scale(state, bias_gain=0.01):
    """In place: every convolution weight (drawn N(0, 1)) times sqrt(2 / fan_in), every bias times ``bias_gain``; fc.weight is
    left alone.  conv1's fan_in is 100 input_channels, so stage magnitudes do not grow with the channel count."""
    for k, v in state.items():
        if k.endswith("bias"):
            state[k] = v * bias_gain
        elif k != "fc.weight":
            state[k] = v * (2.0 / v[0].numel()) ** 0.5
    return state


def fused_case(C, input_channels=1):
    """A random model whose fc row c is clip c's centred pooled vector, normalised (bias: minus its product with the mean),
    so that clip c gets label c: the float64 labels of the clip set cover every 16-lane row of the fused kernel's classifier
    wavefront below C.  For C > 16, row b in another 16-lane row is an exact copy of row a: a tie the kernel must resolve
    to a."""
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(96, input_channels, 99, 10, generator=gen)
    x[C % 96] = 0.0
    state = o_dscnn.random_state(500 + C, num_classes=C, std=1.0, input_channels=input_channels)
    he_scale(state)  # He-scaled weights, small biases: the pooled vectors differ from clip to clip
    _, layers = o_dscnn.forward(state, x.double(), return_layers=True)
    pooled = layers["pool"]
    u = pooled - pooled.mean(dim=0)
    w = 5.0 * u[:C] / u[:C].norm(dim=1, keepdim=True)
    state["fc.weight"] = w.float()
    state["fc.bias"] = -(w @ pooled.mean(dim=0)).float()
    ties = []
    if C > 16:
        ties = [(2, 17)] + ([(20, 33)] if C > 33 else []) + ([(40, 63)] if C > 63 else [])
        for a, b in ties:
            state["fc.weight"][b] = state["fc.weight"][a]
            state["fc.bias"][b] = state["fc.bias"][a]
    want = o_dscnn.forward(state, x.double()).numpy()
    return state, x, want, ties


def check_class_counts(native, ctx, C, mode, case):
    """The assertions of the fused kernel's class-count test on ``case`` = fused_case(C, ...): the float64 labels reach every
    16-lane row below C and every tie row wins somewhere (preconditions), logits within TOL (relative above 100), tied columns
    bit-identical, labels on every sure clip, and never a tie's second column."""
    state, x, want, ties = case
    B = x.shape[0]
    cols = [c for c in range(C) if c not in {b for _, b in ties}]  # the copies tie their originals exactly
    ref = np.asarray(cols)[want[:, cols].argmax(axis=1)]
    assert set(ref // 16) == set(range((C + 15) // 16)), "the clip set must reach every 16-lane row"
    for a, _ in ties:
        assert (ref == a).any(), f"tie row {a} never wins"
    load_state(ctx, state)
    logits = torch.empty((B, C), device=DEV)
    labels = torch.empty((B,), dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    if mode in (4, 5):
        ctx.set_pointwise_math(mode)
        try:
            ctx.forward_f32(xd, logits, labels)
        finally:
            ctx.set_pointwise_math(native.PW_DEFAULT)
    else:
        act = torch.zeros((B, native.ACT_FLOATS_PER_CLIP), device=DEV)
        ctx.forward_debug_f32(xd, logits, labels, act, use_mfma=mode)
    ctx.sync()
    lg, lb = logits.cpu().double().numpy(), labels.cpu().numpy()
    assert np.abs(lg - want).max() <= TOL * max(1.0, float(np.abs(want).max()) / 100), f"C={C} mode {mode}"
    for a, b in ties:
        assert np.array_equal(lg[:, a], lg[:, b])
    top = np.sort(want[:, cols], axis=1) if len(cols) > 1 else None
    sure = (top[:, -1] - top[:, -2] > TOL) if top is not None else np.ones(B, bool)
    assert sure.sum() >= B // 2
    assert np.array_equal(lb[sure], ref[sure]), f"C={C} mode {mode}: {lb[sure][lb[sure] != ref[sure]]} vs {ref[sure][lb[sure] != ref[sure]]}"
    assert not np.isin(lb, [b for _, b in ties]).any(), "a tie must go to the first maximum"
    return lg, lb, sure
