"""Training the BatchNorm DS-CNN on the GPU: kws_dscnn_bn_train_forward_f32 / kws_dscnn_bn_backward_f32 against the float64
restatement of tests/_bn_train_ref.py (logits, batch statistics, all 38 gradients), determinism, the running statistics, the
trainer's step, the autograd wiring of DepthwiseSeparableConvBN, and the entries' refusals.

Every gradient comparison pins both CPU references' ReLU decisions to the GPU's own stages (kws_dscnn_bn_train_debug_f32): one
flipped unit is a visible share of a weight gradient.  Gate, per tensor: max|g - g64| <= 4 max|g32_ref - g64| + 1e-6 max|g64|;
for the nine convolution biases, whose exact gradient is zero, the floor is 1e-6 of the magnitude that cancels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import _bn_train_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = 1e-5
TRAINER_SEED = 0  # of ref.random_params and the batch: float32 and float64 CPU references make identical ReLU decisions on all three steps (asserted by the test)


@pytest.fixture(scope="module")
def native():
    from kws import _native

    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context(0)


def geometry(T, F):
    H1, W1 = (T - 6) // 2 + 1, (F - 6) // 2 + 1
    return [(64, H1 + 2 * k, W1 + 2 * k) for k in range(5)]


def gpu_forward(ctx, blob, num_classes, x, debug=True):
    """-> logits, labels, stats [9, 2, 64], [a0 .. a4] (debug entry; NaN-filled before the call) on the CPU."""
    B, _, T, F = x.shape
    shapes = geometry(T, F)
    sizes = [B * int(np.prod(s)) for s in shapes]
    layers = torch.full((sum(sizes),), float("nan"), device=DEV) if debug else None
    logits = torch.full((B, num_classes), float("nan"), device=DEV)
    labels = torch.empty((B,), dtype=torch.int32, device=DEV)
    stats = torch.full((9, 2, 64), float("nan"), device=DEV)
    ctx.dscnn_bn_train_forward_f32(blob, num_classes, x, EPS, logits, labels, stats, layers=layers)
    ctx.sync()
    acts, off = [], 0
    if debug:
        for shp, n in zip(shapes, sizes):
            acts.append(layers[off:off + n].reshape(B, *shp).cpu())
            off += n
    return logits.cpu(), labels.cpu(), stats.cpu(), acts


def gpu_backward(ctx, blob, num_classes, x, dl):
    grad = torch.full((blob.numel(),), float("nan"), device=DEV)
    ctx.dscnn_bn_backward_f32(blob, num_classes, x, EPS, dl, grad)
    ctx.sync()
    return grad.cpu()


def split(native, grad, num_classes):
    return {name: grad[off:off + n].double().numpy() for name, off, n in native.dscnn_bn_blob_layout(num_classes)}


@pytest.mark.parametrize("B,T,F,num_classes", [(2, 6, 6, 12), (1, 99, 10, 12), (3, 6, 9, 1), (7, 20, 7, 35), (130, 99, 10, 12),
                                                (1025, 8, 7, 12)])
def test_parity_of_logits_statistics_and_gradients(native, ctx, B, T, F, num_classes):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    params = ref.random_params(1000 + B + T, num_classes)
    gen = torch.Generator().manual_seed(B * T + F)
    x = torch.randn(B, 1, T, F, generator=gen)
    dl = torch.randn(B, num_classes, generator=gen)
    blob = torch.from_numpy(ref.flatten(params)).to(DEV)
    xd, dld = x.to(DEV), dl.to(DEV)
    logits, labels, stats, acts = gpu_forward(ctx, blob, num_classes, xd)
    assert all(torch.isfinite(a).all() for a in acts) and torch.isfinite(stats).all() and torch.isfinite(logits).all()
    masks = [a > 0 for a in acts]
    l64, a64, s64 = ref.forward(params, x.double(), EPS, masks)
    l32, a32, s32 = ref.forward(params, x, EPS, masks)
    # the product entry (no stage dump) gives the debug entry's bits, and the labels are the logits' first maximum
    l2, lab2, st2, _ = gpu_forward(ctx, blob, num_classes, xd, debug=False)
    assert torch.equal(l2, logits) and torch.equal(st2, stats) and torch.equal(lab2, labels)
    assert torch.equal(labels.long(), logits.argmax(dim=1))
    bad = []
    err, bound = ref.gate(logits, l32, l64)
    print(f"B={B} {T}x{F} C={num_classes}: logits err {err:.3e} bound {bound:.3e}")
    if err > bound:
        bad.append(("logits", err, bound))
    for i, layer in enumerate(ref.LAYERS):
        for j, what in enumerate(("mean", "var")):
            err, bound = ref.gate(stats[i, j], s32[i, j], s64[i, j])
            if err > bound:
                bad.append((f"{layer}.{what}", err, bound))
    for k in range(5):  # the stages the masks come from are the reference's, to the same rule
        err, bound = ref.gate(acts[k], a32[k], a64[k])
        if err > bound:
            bad.append((f"a{k}", err, bound))
    g = split(native, gpu_backward(ctx, blob, num_classes, xd, dld), num_classes)
    g64, cancels = ref.grads(params, x, dl, torch.float64, EPS, masks)
    g32, _ = ref.grads(params, x, dl, torch.float32, EPS, masks)
    bias_of = {ref.CONV_OF[layer] + ".bias": layer for layer in ref.LAYERS}
    assert list(g) == list(g64) and len(g) == 38
    for name in g:
        assert np.isfinite(g[name]).all(), name
        floor = 1e-6 * cancels[bias_of[name]] if name in bias_of else None
        err, bound = ref.gate(g[name], g32[name].reshape(-1), g64[name].reshape(-1), floor)
        if name in bias_of:
            print(f"  {name}: |g| {err:.3e} = {err / (1e-6 * cancels[bias_of[name]]):.3f} x floor (torch-f32: "
                  f"{np.abs(g32[name]).max() / (1e-6 * cancels[bias_of[name]]):.3f} x)")
        if err > bound:
            bad.append((name, err, bound))
    assert not bad, bad


def test_two_calls_give_the_same_bits(native, ctx):
    """Clip groups of 2 with a short last group (B = 1025): logits, statistics and gradients bit-identical from call to call, also
    after a call on other data in between."""
    params = ref.random_params(5, 12)
    gen = torch.Generator().manual_seed(11)
    x, dl = torch.randn(1025, 1, 8, 7, generator=gen).to(DEV), torch.randn(1025, 12, generator=gen).to(DEV)
    blob = torch.from_numpy(ref.flatten(params)).to(DEV)
    l1, lab1, s1, _ = gpu_forward(ctx, blob, 12, x, debug=False)
    g1 = gpu_backward(ctx, blob, 12, x, dl)
    gpu_backward(ctx, blob, 12, x.flip(0) * 0.5, dl)
    l2, lab2, s2, _ = gpu_forward(ctx, blob, 12, x, debug=False)
    g2 = gpu_backward(ctx, blob, 12, x, dl)
    assert torch.equal(l1, l2) and torch.equal(s1, s2) and torch.equal(lab1, lab2)
    assert torch.isfinite(g1).all() and torch.equal(g1, g2)


def _model(params, num_classes=12):
    from kws.libs.models import DepthwiseSeparableConvBN

    m = DepthwiseSeparableConvBN(num_classes=num_classes, eps=EPS)
    with torch.no_grad():
        for (name, p) in m.named_parameters():
            p.copy_(params[name])
    return m.to(DEV)


def test_running_statistics_and_the_fold_after_them(ctx):
    """Three train-mode forwards on different batches: the 18 buffers against a float64 chain of nn.BatchNorm2d's update rule,
    num_batches_tracked == 3; then eval(): the fold is rebuilt and its logits equal oracle.dscnn.forward_bn at those buffers."""
    from oracle import dscnn as o_dscnn

    params = ref.random_params(77, 12)
    m = _model(params)
    gen = torch.Generator().manual_seed(5)
    batches = [torch.randn(5, 1, 20, 7, generator=gen) * (1.0 + i) + 0.2 * i for i in range(3)]
    with torch.no_grad():
        before = m(batches[1].to(DEV))  # never switched: the fold at the initial buffers (mean 0, var 1)
    fold0 = m._folded
    assert all(int(b.num_batches_tracked) == 0 for b in m.bn_layers())
    m.train()
    for xb in batches:
        with torch.no_grad():
            out = m(xb.to(DEV))
        assert out.grad_fn is None
    run = {}
    for dtype in (torch.float32, torch.float64):
        mean, var = torch.zeros(9, 64, dtype=dtype), torch.ones(9, 64, dtype=dtype)
        for xb in batches:
            _, _, st = ref.forward(params, xb.to(dtype), EPS)
            mean, var = 0.9 * mean + 0.1 * st[:, 0], 0.9 * var + 0.1 * st[:, 1]
        run[dtype] = (mean, var)
    bad = []
    for i, (layer, mod) in enumerate(zip(ref.LAYERS, m.bn_layers())):
        assert int(mod.num_batches_tracked) == 3, layer
        for j, buf in enumerate((mod.running_mean, mod.running_var)):
            err, bound = ref.gate(buf.cpu(), run[torch.float32][j][i], run[torch.float64][j][i])
            if err > bound:
                bad.append((layer, j, err, bound))
    assert not bad, bad
    m.eval()
    x = batches[1]
    with torch.no_grad():
        got = m(x.to(DEV)).cpu()
    assert m._folded is not fold0, "the in-place buffer updates must invalidate the cached fold"
    state = {k[len("plain."):]: v for k, v in params.items() if k.startswith("plain.")}
    bn = {layer: (params[ref.BN_OF[layer] + ".weight"], params[ref.BN_OF[layer] + ".bias"], mod.running_mean.cpu(), mod.running_var.cpu())
          for layer, mod in zip(ref.LAYERS, m.bn_layers())}
    want = o_dscnn.forward_bn({k: v.double() for k, v in state.items()}, {k: tuple(t.double() for t in v) for k, v in bn.items()},
                              x.double(), eps=EPS)
    assert float((got.double() - want).abs().max()) <= 1e-4
    assert float((before.cpu().double() - want).abs().max()) > 1e-3, "the statistics must have moved the fold"


def _decisions(params, x, dtype):
    _, acts, _ = ref.forward(params, x.to(dtype), EPS)
    return [a > 0 for a in acts]


def test_three_trainer_steps_against_the_float64_trajectory():
    """zero_grad, forward, CrossEntropyLoss, backward, Adam (lr 1e-3), three times on one 8-clip batch, against the float64
    reference from the same init: |loss - loss64| <= max(4 x the float32/float64 reference divergence, 1e-5 |loss64|) on every
    step.  Nothing can be pinned here, so the seed is one for which the two CPU references take identical ReLU decisions on all
    three steps -- counted first.  The parameters are the seeded non-trivial ones of the parity cases, not the model's default
    init: with every beta and bias zero the mean of a pointwise output is W times the (zero) mean of the BatchNorm before it, so
    the whole ring sits on the ReLU threshold and half of its decisions differ between any two arithmetics."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    init = ref.random_params(TRAINER_SEED, 12)
    rs = np.random.RandomState(TRAINER_SEED)
    x = torch.from_numpy(rs.standard_normal((8, 1, 99, 10)).astype(np.float32))
    y = torch.from_numpy(rs.randint(0, 12, 8))
    crit = torch.nn.CrossEntropyLoss()

    def traj(dtype):
        st = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in init.items()}
        opt = torch.optim.Adam(list(st.values()), lr=1e-3)
        losses, decisions = [], []
        for _ in range(3):
            opt.zero_grad()
            logits, acts, _ = ref.forward(st, x.to(dtype), EPS)
            decisions.append([(a > 0).clone() for a in acts])
            loss = crit(logits, y)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return np.array(losses), decisions

    l32, d32 = traj(torch.float32)
    l64, d64 = traj(torch.float64)
    differing = sum(int((a != b).sum()) for s32, s64 in zip(d32, d64) for a, b in zip(s32, s64))
    assert differing == 0, f"{differing} ReLU decisions differ between the float32 and the float64 reference: choose another seed"
    model = _model(init).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    xd, yd = x.to(DEV), y.to(DEV)
    hip = []
    for _ in range(3):
        opt.zero_grad()
        loss = crit(model(xd), yd)
        loss.backward()
        opt.step()
        hip.append(loss.item())
    hip = np.array(hip)
    tol = np.maximum(4 * np.maximum.accumulate(np.abs(l32 - l64)), 1e-5 * np.abs(l64))
    print("trainer |hip - l64|:", np.abs(hip - l64), "tolerance:", tol)
    assert np.all(np.abs(hip - l64) <= tol), (hip - l64, tol)
    assert all(int(b.num_batches_tracked) == 3 for b in model.bn_layers())


def test_wiring(native, ctx):
    from kws.common.errors import ModelError

    params = ref.random_params(21, 12)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(6, 1, 20, 7, generator=gen).to(DEV)
    y = torch.randint(0, 12, (6,), generator=gen).to(DEV)
    blob = torch.from_numpy(ref.flatten(params)).to(DEV)
    direct, dlab, _, _ = gpu_forward(ctx, blob, 12, x, debug=False)
    # a model never switched: the fold's bits, whatever nn.Module.training says, and no statistics touched
    m = _model(params)
    assert m.training
    out = m(x)
    assert out.grad_fn is None and torch.equal(out, m.fold()(x)) and not torch.equal(out.cpu(), direct)
    assert all(int(b.num_batches_tracked) == 0 for b in m.bn_layers())
    # train() + no_grad: batch statistics, no graph
    m.train()
    with torch.no_grad():
        out, lab = m(x, return_labels=True)
    assert out.grad_fn is None and not out.requires_grad
    assert torch.equal(out.cpu(), direct) and torch.equal(lab.cpu(), dlab)
    assert all(int(b.num_batches_tracked) == 1 for b in m.bn_layers())
    # grad mode: every .grad equals a direct backward call at the same dlogits
    logits = m(x)
    assert logits.grad_fn is not None and torch.equal(logits.detach().cpu(), direct)
    logits.retain_grad()
    torch.nn.functional.cross_entropy(logits, y).backward()
    want = split(native, gpu_backward(ctx, blob, 12, x, logits.grad.contiguous()), 12)
    for name, p in m.named_parameters():
        assert p.grad is not None and np.array_equal(p.grad.cpu().double().numpy().reshape(-1), want[name]), name
    # frozen BatchNorm parameters still train the rest
    m.zero_grad(set_to_none=True)
    for name, p in m.named_parameters():
        p.requires_grad_(not name.startswith("bn_"))
    logits = m(x)
    logits.retain_grad()
    torch.nn.functional.cross_entropy(logits, y).backward()
    want = split(native, gpu_backward(ctx, blob, 12, x, logits.grad.contiguous()), 12)
    for name, p in m.named_parameters():
        if name.startswith("bn_"):
            assert p.grad is None, name
        else:
            assert np.array_equal(p.grad.cpu().double().numpy().reshape(-1), want[name]), name
    # everything frozen: no graph
    for p in m.parameters():
        p.requires_grad_(False)
    assert m(x).grad_fn is None
    for p in m.parameters():
        p.requires_grad_(True)
    # an input that requires grad is refused in backward
    xg = x.clone().requires_grad_(True)
    with pytest.raises(ModelError, match="gradient with respect to the input features is not provided"):
        m(xg).sum().backward()
    # eval() switches back to the fold
    m.eval()
    n = [int(b.num_batches_tracked) for b in m.bn_layers()]
    assert m(x).grad_fn is None and [int(b.num_batches_tracked) for b in m.bn_layers()] == n


def test_refusals(native):
    """Every refusal is issued on the host, before any allocation or launch: B above the limit is called with a 4-float feature
    buffer."""
    lib, ctx = native.lib(), native.Context(0)
    n12 = 25664 + 65 * 12 + 1152
    blob = torch.zeros(n12, device=DEV)
    small = torch.zeros(4, device=DEV)
    out = torch.zeros(64, device=DEV)
    grad = torch.zeros(n12, device=DEV)
    P = lambda t: t.data_ptr()  # noqa: E731

    def fwd(params=P(blob), n=n12, classes=12, feat=P(small), B=2, T=6, F=6, eps=EPS, logits=P(out)):
        return lib.kws_dscnn_bn_train_forward_f32(ctx._h, params, n, classes, feat, B, T, F, C.c_float(eps), logits, None, None)

    def bwd(params=P(blob), n=n12, classes=12, feat=P(small), B=2, T=6, F=6, eps=EPS, dl=P(out), g=P(grad)):
        return lib.kws_dscnn_bn_backward_f32(ctx._h, params, n, classes, feat, B, T, F, C.c_float(eps), dl, g)

    def msg():
        return lib.kws_last_error(ctx._h).decode()

    for call in (fwd, bwd):
        assert call(B=1) == native.KWS_EINVAL and "B * H1 * W1 >= 2" in msg()
        assert call(B=native.host_dscnn_bn_max_batch(99, 10) + 1, T=99, F=10) == native.KWS_EUNSUPPORTED and "kws_host_dscnn_bn_max_batch" in msg()
        assert call(n=n12 - 1) == native.KWS_EINVAL and "n_floats" in msg()
        assert call(n=25664 + 65 * 12) == native.KWS_EINVAL
        assert call(classes=11) == native.KWS_EINVAL and "n_floats" in msg()
        assert call(classes=0) == native.KWS_EUNSUPPORTED and call(classes=65) == native.KWS_EUNSUPPORTED
        assert call(params=None) == native.KWS_EINVAL and "d_params is NULL" in msg()
        assert call(feat=None) == native.KWS_EINVAL
        assert call(B=0) == native.KWS_EINVAL
        for eps in (0.0, -1e-5, float("inf"), float("nan")):
            assert call(eps=eps) == native.KWS_EINVAL and "eps" in msg(), eps
        assert call(T=5) == native.KWS_EINVAL and call(F=5) == native.KWS_EINVAL
        assert call(T=4100, F=6) == native.KWS_EUNSUPPORTED  # the padded map no longer fits the LDS
    assert fwd(logits=None) == native.KWS_EINVAL and "d_logits is NULL" in msg()
    assert bwd(dl=None) == native.KWS_EINVAL and "d_dlogits is NULL" in msg()
    assert bwd(g=None) == native.KWS_EINVAL and "d_grad is NULL" in msg()
    assert lib.kws_dscnn_bn_train_debug_f32(ctx._h, P(blob), n12, 12, P(small), 2, 6, 6, C.c_float(EPS), P(out), None, None,
                                            None) == native.KWS_EINVAL and "d_layers is NULL" in msg()
    # the entries need no loaded model and leave none behind
    assert lib.kws_forward_map_f32(ctx._h, P(small), 1, 6, 6, P(out), None) == native.KWS_ESTATE
    ctx.close()
