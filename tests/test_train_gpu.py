"""Training on the GPU: kws_dscnn_backward_f32 against the reference's own gradients, determinism, the autograd wiring of
DepthwiseSeparableConv, and the reference trainer's step (zero_grad -> forward -> CrossEntropyLoss -> backward -> Adam).

Accuracy idiom of the project: a gradient is accepted when it lies within 4x of torch-f32's own error from the float64
answer (plus 1e-6 of the tensor's largest magnitude): max|g - g64| <= 4 max|g32_ref - g64| + 1e-6 max|g64|."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MAPS = {"m99x10": (99, 10), "m61x13": (61, 13)}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "train_golden.npz"))


def _state(golden, w):
    from oracle import dscnn as o_dscnn

    if w == "random":
        return o_dscnn.random_state(1)
    return {k: torch.from_numpy(golden[f"default.{k}"]) for k in o_dscnn.STATE_KEYS}


@pytest.fixture(scope="module")
def ctx():
    from kws import _native

    return _native.Context(0)


def _backward(ctx, state, x, dl):
    from oracle import dscnn as o_dscnn

    blob = o_dscnn.flatten_state(state)
    ctx.load_dscnn(blob, 12)
    grad = torch.full((blob.size,), float("nan"), dtype=torch.float32, device=DEV)
    ctx.dscnn_backward_f32(x, x.shape[2], x.shape[3], dl, grad)
    ctx.sync()
    return grad


def _split(grad):
    from oracle import dscnn as o_dscnn

    out, off = {}, 0
    for k, shp in o_dscnn.state_shapes(12).items():
        n = int(np.prod(shp))
        out[k] = grad[off:off + n].reshape(shp)
        off += n
    assert off == grad.numel()
    return out


def _check(g, g64, err32, what):
    for k in g64:
        got, want = np.asarray(g[k], dtype=np.float64), np.asarray(g64[k], dtype=np.float64)
        err = float(np.abs(got - want).max())
        tol = 4 * float(err32[k]) + 1e-6 * float(np.abs(want).max())
        assert err <= tol, f"{what} {k}: max|g - g64| = {err:.3e} > {tol:.3e} (torch-f32 error {float(err32[k]):.3e})"


@pytest.mark.parametrize("w", ["random", "default"])
@pytest.mark.parametrize("m", list(MAPS))
def test_gradient_parity_with_the_reference(golden, ctx, w, m):
    from oracle import dscnn as o_dscnn

    x = torch.from_numpy(golden[f"{m}.x"]).to(DEV)
    dl = torch.from_numpy(golden[f"{w}.{m}.dlogits"].astype(np.float32)).to(DEV)
    g = {k: v.cpu().numpy() for k, v in _split(_backward(ctx, _state(golden, w), x, dl)).items()}
    g64 = {k: golden[f"{w}.{m}.g64.{k}"] for k in o_dscnn.STATE_KEYS}
    err32 = dict(zip(o_dscnn.STATE_KEYS, golden[f"{w}.{m}.err32"]))
    _check(g, g64, err32, f"{w}/{m}")
    if w == "default":  # zero biases: the rings are exactly 0 and must pass no gradient, as in torch
        for i in range(1, 5):
            assert np.isfinite(g[f"dsconv{i}.pointwise.bias"]).all()


def _oracle_grads(state, x, dl, dtype):
    from oracle import dscnn as o_dscnn

    st = {k: v.detach().to(dtype).requires_grad_(True) for k, v in state.items()}
    o_dscnn.forward(st, x.to(dtype)).backward(dl.to(dtype))
    return {k: st[k].grad.detach().to(torch.float64).numpy() for k in o_dscnn.STATE_KEYS}


@pytest.mark.parametrize("B", [1, 7, 1028])
def test_gradient_parity_with_oracle_autograd(ctx, B):
    from oracle import dscnn as o_dscnn

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gen = torch.Generator().manual_seed(B)
    state = o_dscnn.random_state(5)
    x = torch.randn(B, 1, 99, 10, generator=gen)
    dl = torch.randn(B, 12, generator=gen) / B
    g64 = _oracle_grads(state, x, dl, torch.float64)
    g32 = _oracle_grads(state, x, dl, torch.float32)
    err32 = {k: np.abs(g32[k] - g64[k]).max() for k in g64}
    g = {k: v.cpu().numpy() for k, v in _split(_backward(ctx, state, x.to(DEV), dl.to(DEV))).items()}
    _check(g, g64, err32, f"B={B}")


def test_backward_is_deterministic(golden, ctx):
    from oracle import dscnn as o_dscnn

    gen = torch.Generator().manual_seed(11)
    x = torch.randn(1500, 1, 99, 10, generator=gen).to(DEV)
    dl = torch.randn(1500, 12, generator=gen).to(DEV)
    a = _backward(ctx, o_dscnn.random_state(1), x, dl).clone()
    b = _backward(ctx, o_dscnn.random_state(1), x, dl)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_chunks_add_in_order(ctx):
    """9000 clips at 99 x 10 exceed one workspace chunk (2^31 floats: 8388 clips): the call equals the sum of the two chunk
    calls, bit for bit."""
    from oracle import dscnn as o_dscnn

    gen = torch.Generator().manual_seed(12)
    state = o_dscnn.random_state(2)
    x = torch.randn(9000, 1, 99, 10, generator=gen).to(DEV)
    dl = (torch.randn(9000, 12, generator=gen) / 9000).to(DEV)
    whole = _backward(ctx, state, x, dl).clone()
    first = _backward(ctx, state, x[:8388], dl[:8388]).clone()
    rest = _backward(ctx, state, x[8388:], dl[8388:])
    assert torch.equal(whole, first + rest)


def test_backward_errors(ctx):
    from kws import _native
    from kws.common.errors import ModelError
    from oracle import dscnn as o_dscnn

    x = torch.zeros(2, 1, 99, 10, device=DEV)
    dl = torch.zeros(2, 12, device=DEV)
    g = torch.zeros(26444, device=DEV)
    fresh = _native.Context(0)
    with pytest.raises(ModelError, match=r"no model loaded.*\(code -4\)"):
        fresh.dscnn_backward_f32(x, 99, 10, dl, g)
    ctx.load_dscnn(o_dscnn.flatten_state(o_dscnn.random_state(1)), 12)
    with pytest.raises(ModelError, match=r"T >= 6"):
        ctx.dscnn_backward_f32(x, 5, 10, dl, g)
    multi = _native.Context(0)
    blob3 = np.zeros(6400 * 3 + 19264 + 65 * 12, dtype=np.float32)
    multi.load_dscnn(blob3, 12, 3)
    with pytest.raises(ModelError, match=r"input_channels == 1.*\(code -5\)"):
        multi.dscnn_backward_f32(torch.zeros(2, 3, 99, 10, device=DEV), 99, 10, dl, torch.zeros(blob3.size, device=DEV))


def _model(state, device="cpu"):
    from kws.libs.models import DepthwiseSeparableConv

    m = DepthwiseSeparableConv()
    m.load_state_dict({k: v.clone() for k, v in state.items()})
    return m.to(device).train()   # the reference trainers call model.train() every epoch


@pytest.mark.parametrize("param_dev", ["cpu", "cuda"])
@pytest.mark.parametrize("shape", [(99, 10), (61, 13)])
def test_forward_unchanged_under_grad_mode(param_dev, shape):
    from oracle import dscnn as o_dscnn

    m = _model(o_dscnn.random_state(1), param_dev)
    x = torch.randn(37, 1, *shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        l0, y0 = m(x, return_labels=True)
    l1, y1 = m(x, return_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and torch.equal(y0, y1)
    assert l1.device == x.device and y1.dtype == y0.dtype
    # after eval() (and on a model never switched with train()) the logits are plain tensors, as before
    l2, y2 = m.eval()(x, return_labels=True)
    assert l2.grad_fn is None and torch.equal(l0, l2) and torch.equal(y0, y2)


@pytest.mark.parametrize("param_dev", ["cpu", "cuda"])
def test_autograd_wiring(golden, param_dev):
    from kws.common.errors import ModelError
    from oracle import dscnn as o_dscnn

    state = _state(golden, "random")
    m = _model(state, param_dev)
    x = torch.from_numpy(golden["m99x10.x"]).to(DEV)
    labels = torch.from_numpy(golden["m99x10.labels"]).to(DEV)
    loss = torch.nn.CrossEntropyLoss()(m(x), labels)
    loss.backward()
    g1 = {k: p.grad.clone() for k, p in m.named_parameters()}
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.device == p.device and p.grad.shape == p.shape, k
    # the gradients are the reference's (the golden dlogits are those of this loss, at the float64 forward)
    g64 = {k: golden[f"random.m99x10.g64.{k}"] for k in o_dscnn.STATE_KEYS}
    err32 = dict(zip(o_dscnn.STATE_KEYS, golden["random.m99x10.err32"]))
    # the loss's dlogits come from the float32 forward here: allow torch-f32's forward error on top (1e-5 relative)
    for k in g64:
        got = g1[k].cpu().double().numpy()
        assert np.abs(got - g64[k]).max() <= 4 * err32[k] + 1e-5 * np.abs(g64[k]).max(), k
    # a second backward without zero_grad accumulates
    torch.nn.CrossEntropyLoss()(m(x), labels).backward()
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, 2 * g1[k]), k
    # a parameter modified in place between forward and backward is rejected by torch's version check
    loss = torch.nn.CrossEntropyLoss()(m(x), labels)
    with torch.no_grad():
        m.dsconv2.pointwise.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    # no gradient with respect to the input
    xr = x.clone().requires_grad_(True)
    with pytest.raises(ModelError, match="gradient with respect to the input features is not provided"):
        m(xr).sum().backward()


def test_reference_trainer_step():
    """20 steps of the reference trainer (training.py:286-297) on a fixed 64-clip batch, HIP model on the GPU against the
    float32 oracle on the CPU from the same init; tolerance: 4x the float32-vs-float64 oracle divergence, floor 1e-5
    relative."""
    from kws.libs.models import DepthwiseSeparableConv
    from oracle import dscnn as o_dscnn

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    torch.manual_seed(0)
    init = DepthwiseSeparableConv().state_dict()
    rs = np.random.RandomState(7)
    x = torch.from_numpy(rs.standard_normal((64, 1, 99, 10)).astype(np.float32))
    y = torch.from_numpy(rs.randint(0, 12, 64))
    crit = torch.nn.CrossEntropyLoss()

    def oracle_traj(dtype):
        st = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in init.items()}
        opt = torch.optim.Adam(list(st.values()), lr=1e-3)
        out = []
        for _ in range(20):
            opt.zero_grad()
            loss = crit(o_dscnn.forward(st, x.to(dtype)), y)
            loss.backward()
            opt.step()
            out.append(loss.item())
        return np.array(out)

    model = _model(init, "cuda")
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    xd, yd = x.to(DEV), y.to(DEV)
    hip = []
    for _ in range(20):
        opt.zero_grad()
        loss = crit(model(xd), yd)
        loss.backward()
        opt.step()
        hip.append(loss.item())
    hip = np.array(hip)
    l32, l64 = oracle_traj(torch.float32), oracle_traj(torch.float64)
    div = np.maximum.accumulate(np.abs(l32 - l64))
    tol = np.maximum(4 * div, 1e-5 * np.abs(l64))
    assert np.all(np.abs(hip - l32) <= tol), (hip - l32, tol)
    assert hip[-1] < hip[0] - 1e-3, hip
