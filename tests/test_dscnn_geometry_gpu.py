"""DS-CNN forward and gradients away from the 99 x 10, 12-class corner: feature maps from the smallest (6 x 6, conv1 output
1 x 1) to the largest accepted ((T + 4)(F + 4) = 40960), class counts 1 to 64, batch sizes whose last clip group is short,
the 16384-clip chunk cap, inputs that put ReLU units exactly at zero, and the autograd wiring of DepthwiseSeparableConv.

Gradients are checked against the float64 oracle with the ReLU decisions pinned to the GPU's own stage outputs
(``oracle.dscnn.forward(..., masks=)``): the kernel and torch-f32 then compute the same function and the comparison measures
arithmetic error only.  The acceptance rule is the suite's: max|g - g64| <= 4 max|g32 - g64| + 1e-6 max|g64| per tensor,
g32 being torch-f32 autograd with the same masks."""
import os

import numpy as np
import pytest
import torch

from _dscnn_forward import DEV, LAYER_RTOL, TOL  # noqa: F401  (the gates of tests/test_gpu_parity.py)
from _dscnn_forward import check_class_counts as _check_class_counts
from _dscnn_forward import check_forward as _check_forward
from _dscnn_forward import fused_case as _fused_case
from _dscnn_forward import geometry as _geometry
from _dscnn_forward import gpu_forward as _gpu_forward

pytestmark = pytest.mark.gpu

N_BODY = 6464 + 4 * 4800  # conv1 + four blocks; fc adds 65 C


@pytest.fixture(scope="module")
def native():
    from kws import _native

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def _gpu_grad(ctx, x, dl, C):
    """kws_dscnn_backward_f32 into a NaN-filled buffer of 25664 + 65 C floats (an entry never written stays NaN)."""
    g = torch.full((N_BODY + 65 * C,), float("nan"), device=DEV)
    ctx.dscnn_backward_f32(x, x.shape[2], x.shape[3], dl, g)
    ctx.sync()
    return g


def _split(flat, C):
    from oracle import dscnn as o_dscnn

    out, off = {}, 0
    for k, shp in o_dscnn.state_shapes(C).items():
        n = int(np.prod(shp))
        out[k] = flat[off:off + n].reshape(shp)
        off += n
    assert off == flat.size
    return out


def _oracle_grads(state, x, dl, masks):
    """(g64, g32) with the ReLU decisions pinned.  Batches above 2^28 floats of float64 activations run in chunks: g64 sums
    the chunks in float64, g32 in float32 (torch-f32 accumulating micro-batches), so host memory stays bounded."""
    from oracle import dscnn as o_dscnn

    B, _, T, F = x.shape
    per_clip = sum(int(np.prod(s)) for s in _geometry(T, F)) * 2
    step = max(1, (1 << 28) // per_clip)
    g64 = g32 = None
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        m = {k: v[sl] for k, v in masks.items()}
        a = o_dscnn.grads(state, x[sl], dl[sl], torch.float64, m)
        b = {k: v.astype(np.float32) for k, v in o_dscnn.grads(state, x[sl], dl[sl], torch.float32, m).items()}
        g64 = a if g64 is None else {k: g64[k] + a[k] for k in a}
        g32 = b if g32 is None else {k: g32[k] + b[k] for k in b}
    return g64, {k: v.astype(np.float64) for k, v in g32.items()}


def ratios(g, g64, g32):
    """Per tensor: max|g - g64| / (4 max|g32 - g64| + 1e-6 max|g64|); the gradient passes when every ratio is <= 1."""
    out = {}
    for k in g64:
        err = float(np.abs(np.asarray(g[k], dtype=np.float64) - g64[k]).max())
        tol = 4 * float(np.abs(g32[k] - g64[k]).max()) + 1e-6 * float(np.abs(g64[k]).max())
        out[k] = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    return out


def check_backward(ctx, state, x, dl, what):
    """Load ``state`` (C from fc.weight), run the backward twice (bit-identical, every entry written) and check it against the
    pinned float64 oracle.  Returns (gradient dict, ratio dict)."""
    from oracle import dscnn as o_dscnn

    C = state["fc.weight"].shape[0]
    blob = o_dscnn.flatten_state(state)
    assert blob.size == N_BODY + 65 * C
    ctx.load_dscnn(blob, C)
    xd, dld = x.to(DEV), dl.to(DEV)
    a = _gpu_grad(ctx, xd, dld, C)
    b = _gpu_grad(ctx, xd, dld, C)
    assert torch.isfinite(a).all(), f"{what}: {int((~torch.isfinite(a)).sum())} gradient entries not written or not finite"
    assert torch.equal(a, b), f"{what}: two calls differ"
    _, _, stages = _gpu_forward(ctx, xd, C)
    del xd
    g64, g32 = _oracle_grads(state, x, dl, o_dscnn.relu_masks(stages))
    g = _split(a.cpu().numpy(), C)
    r = ratios(g, g64, g32)
    bad = {k: round(v, 2) for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1 for {bad}"
    return g, r


def _inputs(B, T, F, C, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, T, F, generator=gen), torch.randn(B, C, generator=gen) / B


# ------------------------------------------------------------------------------------------------------------ backward
MAPS = {  # (T, F): B
    (6, 6): 9,       # conv1 output 1 x 1
    (7, 7): 9,       # 1 x 1, conv1's last tap row inside the map
    (6, 40): 6,      # one spatial dimension of 1
    (40, 6): 6,
    (20, 20): 5,     # P0 = 64: exactly one conv1 / pointwise tile
    (22, 20): 5,     # one tile and a remainder
    (99, 10): 7,
    (61, 13): 7,
    (149, 10): 5,
    (125, 124): 2,   # padded plane 129 x 128 floats: over 64 KB of LDS
    (156, 252): 2,   # padded plane of exactly 40960 floats, P0 = 9424
}


@pytest.mark.parametrize("T,F", list(MAPS), ids=[f"{t}x{f}" for t, f in MAPS])
def test_backward_and_forward_on_every_map(native, ctx, T, F):
    """The backward against the pinned float64 oracle, and the composed forward it recomputes with against the plain float64
    oracle: stage outputs within LAYER_RTOL (the relu(bias) ring exact), logits within TOL, labels wherever the float64
    top-2 margin exceeds TOL."""
    from oracle import dscnn as o_dscnn

    B, C = MAPS[(T, F)], 12
    state = o_dscnn.random_state(T * 1000 + F, num_classes=C)
    x, dl = _inputs(B, T, F, C, T + F)
    check_backward(ctx, state, x, dl, f"{T}x{F}")
    _check_forward(ctx, state, x, f"{T}x{F}")


@pytest.mark.parametrize("C", [1, 2, 35, 64])
@pytest.mark.parametrize("T,F", [(99, 10), (22, 20)], ids=["99x10", "22x20"])
def test_backward_class_counts(native, ctx, T, F, C):
    """fc's gradient slice (65 C floats at o_fc) and the per-thread partial sums of kws_bwd_fc_kernel for every C."""
    from oracle import dscnn as o_dscnn

    state = o_dscnn.random_state(C, num_classes=C)
    x, dl = _inputs(33, T, F, C, 100 + C)
    check_backward(ctx, state, x, dl, f"{T}x{F} C={C}")
    _check_forward(ctx, state, x, f"{T}x{F} C={C}")


@pytest.mark.parametrize("B,T,F", [(1024, 20, 8), (1025, 20, 8), (3071, 20, 8), (4096, 99, 10)],
                         ids=["1024", "1025", "3071", "4096-99x10"])
def test_backward_batch_splits(native, ctx, B, T, F):
    """cpg = ceil(B / 1024) clips per group, G = ceil(B / cpg) groups: 1024 = 1024 x 1; 1025 = 512 x 2 + 1 (the last group
    holds one clip); 3071 = 1023 x 3 + 2; 4096 = 1024 x 4 at 99 x 10 (long per-group chains)."""
    from oracle import dscnn as o_dscnn

    state = o_dscnn.random_state(B, num_classes=12)
    x, dl = _inputs(B, T, F, 12, B)
    check_backward(ctx, state, x, dl, f"B={B} {T}x{F}")


def test_backward_clip_cap_chunks_add_in_order(native, ctx):
    """16421 clips at 6 x 6: one chunk of 16384 clips (the cap) and one of 37, added in that order, bit for bit; and the
    whole against the oracle."""
    from oracle import dscnn as o_dscnn

    B, C = 16421, 12
    state = o_dscnn.random_state(16421, num_classes=C)
    x, dl = _inputs(B, 6, 6, C, 16)
    check_backward(ctx, state, x, dl, "B=16421 6x6")
    xd, dld = x.to(DEV), dl.to(DEV)
    whole = _gpu_grad(ctx, xd, dld, C)
    first = _gpu_grad(ctx, xd[:16384], dld[:16384], C)
    rest = _gpu_grad(ctx, xd[16384:], dld[16384:], C)
    assert torch.equal(whole, first + rest)


@pytest.mark.parametrize("case", ["zero_and_constant_clips", "default_init", "dead_rings"])
@pytest.mark.parametrize("T,F", [(20, 20), (61, 13)], ids=["20x20", "61x13"])
def test_backward_relu_edges(native, ctx, case, T, F):
    """Inputs that put ReLU units exactly at zero or switch whole rings off: all-zero and constant clips among random ones,
    the reference's default init (zero biases: every ring is exactly 0 and passes nothing), negative pointwise biases."""
    from kws.libs.models import DepthwiseSeparableConv
    from oracle import dscnn as o_dscnn

    C, B = 12, 24
    x, dl = _inputs(B, T, F, C, 7)
    state = o_dscnn.random_state(77, num_classes=C)
    if case == "zero_and_constant_clips":
        x[::4] = 0.0
        x[1::6] = 0.75
        x[2::6] = -1.5
    elif case == "default_init":
        torch.manual_seed(5)
        state = {k: v.detach().clone() for k, v in DepthwiseSeparableConv(C).state_dict().items()}
        x[::5] = 0.0
    else:
        for i in range(1, 5):
            b = state[f"dsconv{i}.pointwise.bias"]
            state[f"dsconv{i}.pointwise.bias"] = -b.abs() - 0.01
    g, _ = check_backward(ctx, state, x, dl, f"{case} {T}x{F}")
    if case != "zero_and_constant_clips":  # no ring unit is on, so the pointwise bias gradients come from the interior only
        _, _, stages = _gpu_forward(ctx, x.to(DEV), C)
        assert all(float(stages[f"dsconv{i}"][:, :, 0, :].max()) <= 0 for i in range(1, 5))


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("C", [1, 35, 64])
@pytest.mark.parametrize("T,F", [(6, 6), (20, 20), (125, 124), (156, 252)], ids=["6x6", "20x20", "125x124", "156x252"])
def test_composed_forward_class_counts(native, ctx, T, F, C):
    from oracle import dscnn as o_dscnn

    B = 3 if T * F > 10000 else 17
    x, _ = _inputs(B, T, F, C, 300 + C)
    _check_forward(ctx, o_dscnn.random_state(400 + C, num_classes=C), x, f"{T}x{F} C={C}")


@pytest.mark.parametrize("mode", [0, 1, 4, 5])  # VALU cross-check, f32 MFMA, split-bf16 MFMA, f16-pair MFMA
@pytest.mark.parametrize("C", [1, 2, 35, 64])
def test_fused_kernel_class_counts(native, ctx, C, mode):
    """The fused 99 x 10 kernel puts class c on lane c of wavefront 0 and finds the first maximum by a DPP reduction over
    16-lane rows and a ballot: labels from every 16-lane row below C, and exact ties across rows."""
    from oracle import dscnn as o_dscnn

    _check_class_counts(native, ctx, C, mode, _fused_case(C))


@pytest.mark.parametrize("C", [1, 35, 64])
def test_softmax_class_counts(native, ctx, C):
    z = torch.randn(300, C, generator=torch.Generator().manual_seed(C)) * 6
    z[7] = 0.0
    z[8] = 80.0
    if C > 1:
        z[9, C - 1] = 90.0  # the maximum in the last class
    p = torch.empty((300, C), device=DEV)
    ctx.softmax_f32(z.to(DEV), p)
    ctx.sync()
    zn = z.numpy().astype(np.float64)
    e = np.exp(zn - zn.max(axis=1, keepdims=True))
    assert np.abs(p.cpu().numpy() - e / e.sum(axis=1, keepdims=True)).max() <= 1e-6


def test_depthwise_grid_stride_batch(native):
    """40 x 40 at 16384 clips: B * 64 * 18 * 18 > 2^28 elements, so the composed depthwise kernel's grid-stride loop wraps;
    the logits are those of the same clips in four batches of 4096, bit for bit."""
    from oracle import dscnn as o_dscnn

    c = native.Context(0)
    c.use_torch_stream()
    try:
        C = 12
        c.load_dscnn(o_dscnn.flatten_state(o_dscnn.random_state(40)), C)
        x = torch.randn(16384, 1, 40, 40, generator=torch.Generator().manual_seed(40)).to(DEV)
        whole = torch.empty((16384, C), device=DEV)
        c.forward_map_f32(x, whole, None)
        parts = torch.empty_like(whole)
        for b0 in range(0, 16384, 4096):
            c.forward_map_f32(x[b0:b0 + 4096], parts[b0:b0 + 4096], None)
        c.sync()
        assert torch.isfinite(whole).all() and torch.equal(whole, parts)
        want = o_dscnn.forward(o_dscnn.random_state(40), x[-3:].cpu().double()).numpy()
        assert np.abs(whole[-3:].cpu().double().numpy() - want).max() <= TOL
    finally:
        c.close()


def test_stage_dump_across_the_clip_cap(native, ctx):
    """16387 clips at 6 x 6, two classes: a chunk of 16384 clips (the cap) and one of 3.  The dumped stages and logits of
    clips 16380 .. 16386 -- the last four of the first chunk, all of the second -- are those of a debug call on these seven
    clips alone, bit for bit (no kernel of the composed path mixes clips), and every float of the dump is written."""
    from oracle import dscnn as o_dscnn

    B, C, T, F, lo = 16387, 2, 6, 6, 16380
    ctx.load_dscnn(o_dscnn.flatten_state(o_dscnn.random_state(16387, num_classes=C)), C)
    x = torch.randn(B, 1, T, F, generator=torch.Generator().manual_seed(16387)).to(DEV)
    sizes = [int(np.prod(s)) for s in _geometry(T, F)]

    def dump(xs):
        n = xs.shape[0]
        layers = torch.full((n * sum(sizes),), float("nan"), device=DEV)
        logits = torch.empty((n, C), device=DEV)
        labels = torch.empty((n,), dtype=torch.int32, device=DEV)
        ctx.forward_map_f32(xs, logits, labels, layers=layers)
        ctx.sync()
        ends = np.cumsum([n * s for s in sizes])
        return logits, labels, [layers[e - n * s:e].reshape(n, s) for e, s in zip(ends, sizes)], layers

    logits, labels, stages, layers = dump(x)
    assert torch.isfinite(layers).all()
    l7, b7, s7, _ = dump(x[lo:].clone())
    for k, (a, b) in enumerate(zip(stages, s7)):
        assert torch.equal(a[lo:], b), f"stage {k}"
    assert torch.equal(logits[lo:], l7) and torch.equal(labels[lo:], b7)


def test_accepted_domain_is_the_same_forward_and_backward(native, ctx):
    from kws.common.errors import ModelError
    from oracle import dscnn as o_dscnn

    C = 12
    ctx.load_dscnn(o_dscnn.flatten_state(o_dscnn.random_state(3)), C)
    dl = torch.zeros((1, C), device=DEV)
    g = torch.zeros((N_BODY + 65 * C,), device=DEV)
    lg = torch.empty((1, C), device=DEV)
    for T, F, code in [(156, 252, None), (157, 252, native.KWS_EUNSUPPORTED), (252, 157, native.KWS_EUNSUPPORTED),
                       (5, 10, native.KWS_EINVAL), (99, 5, native.KWS_EINVAL)]:
        x = torch.zeros((1, 1, T, F), device=DEV)
        calls = (lambda: ctx.forward_map_f32(x, lg, None), lambda: ctx.dscnn_backward_f32(x, T, F, dl, g))
        for call in calls:
            if code is None:
                call()
                ctx.sync()
            else:
                with pytest.raises(ModelError, match=rf"\(code {code}\)"):
                    call()
    assert torch.isfinite(g).all() and torch.isfinite(lg).all()


# ------------------------------------------------------------------------------------------------------------ autograd
def _model(state, C):
    from kws.libs.models import DepthwiseSeparableConv

    m = DepthwiseSeparableConv(num_classes=C)
    m.load_state_dict({k: v.clone() for k, v in state.items()})
    return m.to(DEV).train()


@pytest.mark.parametrize("T,F", [(61, 13), (149, 10)], ids=["61x13", "149x10"])
def test_autograd_35_classes_is_the_direct_call(native, T, F):
    """CrossEntropyLoss over a 35-class model: every .grad equals a direct kws_dscnn_backward_f32 call with the same dlogits,
    bit for bit; and it stays so when only some parameters are trainable or when the step runs on a side stream."""
    from oracle import dscnn as o_dscnn

    C = 35
    state = o_dscnn.random_state(35, num_classes=C)
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(40, 1, T, F, generator=gen).to(DEV)
    y = torch.randint(0, C, (40,), generator=gen).to(DEV)

    def step(m):
        logits = m(x)
        logits.retain_grad()
        torch.nn.CrossEntropyLoss()(logits, y).backward()
        return logits.grad.detach().clone(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}

    m = _model(state, C)
    dl, g = step(m)
    direct = native.Context(0)
    direct.use_torch_stream()
    direct.load_dscnn(o_dscnn.flatten_state(state), C)
    want = _split(_gpu_grad(direct, x, dl, C).cpu().numpy(), C)
    direct.close()
    for k in o_dscnn.STATE_KEYS:
        assert np.array_equal(g[k].cpu().numpy(), want[k]), k

    # frozen conv1: no .grad there, the rest unchanged
    mf = _model(state, C)
    mf.conv1.requires_grad_(False)
    _, gf = step(mf)
    assert gf["conv1.weight"] is None and gf["conv1.bias"] is None
    for k in o_dscnn.STATE_KEYS[2:]:
        assert torch.equal(gf[k], g[k]), k

    # forward and backward on a side stream
    ms = _model(state, C)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _, gs = step(ms)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in o_dscnn.STATE_KEYS:
        assert torch.equal(gs[k], g[k]), k


def test_autograd_uses_the_weights_the_forward_saw(native):
    """A parameter replaced by a new nn.Parameter between forward and backward: torch's version check does not fire (the
    saved tensor was not modified), so the backward must use the saved weights -- not the module's current ones."""
    from oracle import dscnn as o_dscnn

    C = 12
    state = o_dscnn.random_state(8, num_classes=C)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(16, 1, 61, 13, generator=gen).to(DEV)
    y = torch.randint(0, C, (16,), generator=gen).to(DEV)
    ref = _model(state, C)
    torch.nn.CrossEntropyLoss()(ref(x), y).backward()

    m = _model(state, C)
    old = {k: p for k, p in m.named_parameters()}
    loss = torch.nn.CrossEntropyLoss()(m(x), y)
    m.fc.weight = torch.nn.Parameter(m.fc.weight.detach() * -3.0)
    m.dsconv2.pointwise.weight = torch.nn.Parameter(m.dsconv2.pointwise.weight.detach() + 0.5)
    loss.backward()
    for k, p in ref.named_parameters():
        assert torch.equal(old[k].grad, p.grad), k
    assert m.fc.weight.grad is None and m.dsconv2.pointwise.weight.grad is None
    # and the next forward runs at the new weights
    with torch.no_grad():
        got = m(x)
    want = o_dscnn.forward({k: v.detach().cpu() for k, v in m.state_dict().items()}, x.cpu().double())
    assert np.abs(got.cpu().double().numpy() - want.numpy()).max() <= TOL
