"""kws_dsblock_forward_f32, the drop-in for DepthwiseSeparableConvBlock.forward at any shape, away from the four recorded
shapes of test_standalone_block_forward (all with P = Ho * Wo < 64): the pointwise kernel's second and partial position tiles,
the ring writer beside more than one position tile, even kernels, stride 3, padding >= kernel, one row, more than
64 input channels, the batch in grid.z, and 1 x 1 everything.

The truth is oracle.dscnn.block_forward in float64.  Weights are N(0, 0.5), biases N(0, 0.3), inputs N(0, 2), seeded per case.
Gate: max|y - y64| <= LAYER_RTOL max|y64| (tests/test_gpu_parity.py); torch-f32's own relative error on these cases is at most
4e-7.  The ring -- all `pad` rows and columns on each side -- is relu(bias) bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _dscnn_forward import DEV, LAYER_RTOL
from oracle import dscnn as o_dscnn

pytestmark = pytest.mark.gpu

CASES = {  # (c_in, c_out, k, stride, pad, B, H, W): what it reaches
    (1, 1, 1, 1, 0, 1, 1, 1): "everything 1",
    (16, 64, 3, 1, 1, 1, 8, 8): "P = 64, exact tiles, one slab",
    (17, 65, 3, 1, 1, 2, 9, 8): "P = 72: second position tile partial, slab + 1, channel tile + 1",
    (33, 129, 3, 2, 1, 2, 13, 10): "three channel tiles, stride 2 with remainder",
    (5, 7, 2, 1, 0, 3, 5, 6): "even kernel, no padding",
    (4, 6, 4, 3, 2, 2, 11, 7): "even kernel, stride 3, rows left unused by the floor",
    (6, 10, 3, 1, 3, 2, 4, 5): "padding >= kernel: ring three wide, P = 72 with the ring writer",
    (3, 5, 7, 1, 3, 1, 2, 3): "kernel larger than the input, fits only through padding",
    (8, 8, 1, 2, 0, 2, 7, 7): "1 x 1 depthwise with stride",
    (64, 64, 3, 1, 1, 1, 30, 30): "P = 900: 15 tiles, last holds 4",
    (2, 3, 3, 1, 1, 1, 1, 40): "one row",
    (130, 20, 3, 1, 1, 1, 6, 6): "C_in over 64, nine slabs, last partial",
    (64, 64, 3, 1, 1, 70, 5, 25): "batch in grid.z, P = 125",
}
PAD3 = (6, 10, 3, 1, 3, 2, 4, 5)
VARIANTS = [(c, None) for c in CASES] + [(PAD3, "negative"), (PAD3, "positive")]  # pointwise biases all < 0 / all > 0
NAMES = ("depthwise.weight", "depthwise.bias", "pointwise.weight", "pointwise.bias")


def _id(v):
    return "-".join(str(n) for n in v[0]) + (f"-{v[1]}" if v[1] else "")


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


_BUILT = {}


def build(variant):
    """(params float32 on the CPU, x float32 on the CPU, y64 numpy float64) of a case, computed once."""
    if variant not in _BUILT:
        (ci, co, k, st, pd, B, H, W), bias = variant
        gen = torch.Generator().manual_seed((5 + sum(n * 31 ** i for i, n in enumerate(variant[0]))) % (1 << 31))
        params = {"depthwise.weight": torch.randn(ci, 1, k, k, generator=gen) * 0.5, "depthwise.bias": torch.randn(ci, generator=gen) * 0.3,
                  "pointwise.weight": torch.randn(co, ci, 1, 1, generator=gen) * 0.5, "pointwise.bias": torch.randn(co, generator=gen) * 0.3}
        if bias == "negative":
            params["pointwise.bias"] = -params["pointwise.bias"].abs() - 0.01
        elif bias == "positive":
            params["pointwise.bias"] = params["pointwise.bias"].abs() + 0.01
        x = torch.randn(B, ci, H, W, generator=gen) * 2.0
        y64 = o_dscnn.block_forward({n: v.double() for n, v in params.items()}, x.double(), k, st, pd).numpy()
        assert y64.max() > 0, "a case whose output is all zero checks nothing"
        _BUILT[variant] = (params, x, y64)
    return _BUILT[variant]


def out_shape(case):
    ci, co, k, st, pd, B, H, W = case
    return (B, co, (H + 2 * pd - k) // st + 1 + 2 * pd, (W + 2 * pd - k) // st + 1 + 2 * pd)


def raw(ctx, case, dev_params, xd):
    """kws_dsblock_forward_f32 into a NaN-filled buffer with one guard row beyond the end: every element written, the guard
    untouched.  Returns the output on the CPU."""
    shp = out_shape(case)
    n = int(np.prod(shp))
    buf = torch.full((n + shp[3],), float("nan"), device=DEV)
    ctx.dsblock_forward_f32(xd, *dev_params, case[2], case[3], case[4], buf)
    ctx.sync()
    assert torch.isnan(buf[n:]).all(), f"{case}: written beyond the output"
    out = buf[:n].reshape(shp).cpu()
    assert torch.isfinite(out).all(), f"{case}: {int((~torch.isfinite(out)).sum())} elements not written"
    return out


def on_device(params):
    return tuple(params[n].to(DEV).contiguous() for n in NAMES)


@pytest.mark.parametrize("variant", VARIANTS, ids=[_id(v) for v in VARIANTS])
def test_block_shape_against_float64(native, ctx, variant):
    """The module's forward and the raw entry (into a guarded NaN-filled buffer) give one set of bits, twice; they are within
    LAYER_RTOL of float64, and the whole ring is relu(bias)."""
    from kws.libs.models import DepthwiseSeparableConvBlock

    case, bias = variant
    ci, co, k, st, pd, B, H, W = case
    params, x, y64 = build(variant)
    blk = DepthwiseSeparableConvBlock(ci, co, kernel_size=k, stride=st, padding=pd)
    blk.load_state_dict(params)
    xd = x.to(DEV)
    y = blk(xd)
    assert tuple(y.shape) == out_shape(case) == y64.shape
    assert y.grad_fn is None
    y = y.cpu()
    got = raw(ctx, case, on_device(params), xd)
    assert torch.equal(got, y), "the module and the raw entry differ"
    assert torch.equal(raw(ctx, case, on_device(params), xd), got), "two calls differ"
    err, scale = float(np.abs(got.double().numpy() - y64).max()), float(np.abs(y64).max())
    print(f"dsblock {_id(variant)}: error/gate {err / (LAYER_RTOL * scale):.4f}")
    assert err <= LAYER_RTOL * scale, (case, err, scale)
    if pd:  # the ring: relu(bias) bit for bit, all pad rows and columns on each side
        ring = torch.relu(params["pointwise.bias"]).reshape(1, co, 1, 1)
        inner = torch.zeros(out_shape(case)[2:], dtype=torch.bool)
        inner[pd:-pd, pd:-pd] = True
        want = ring.expand(*out_shape(case))[..., ~inner]
        assert want.shape[-1] == out_shape(case)[2] * out_shape(case)[3] - (out_shape(case)[2] - 2 * pd) * (out_shape(case)[3] - 2 * pd)
        assert torch.equal(got[..., ~inner], want), case
        if bias == "negative":
            assert not got[..., ~inner].any()
        if bias == "positive":
            assert (got[..., ~inner] > 0).all()


def test_workspace_grows_and_is_reused(native):
    """The whole list twice on one fresh context, by ascending and then descending workspace size: the workspace grows case
    by case, then every smaller case runs in the grown one.  Same bits both times, and the float64 gate on the second."""
    order = sorted(CASES, key=lambda c: c[5] * c[0] * (out_shape(c)[2] - 2 * c[4]) * (out_shape(c)[3] - 2 * c[4]))  # B C_in Ho Wo
    c = native.Context(0)
    c.use_torch_stream()
    try:
        first = {}
        for case in order:
            params, x, _ = build((case, None))
            first[case] = raw(c, case, on_device(params), x.to(DEV))
        for case in reversed(order):
            params, x, y64 = build((case, None))
            again = raw(c, case, on_device(params), x.to(DEV))
            assert torch.equal(again, first[case]), f"{case}: the bits changed once the workspace had grown"
            assert np.abs(again.double().numpy() - y64).max() <= LAYER_RTOL * np.abs(y64).max(), case
    finally:
        c.close()


def test_block_refusals_leave_the_context_usable(native, ctx):
    """What the entry refuses it refuses before it launches or writes anything, and the next valid call gives the bits it
    gave before."""
    from kws.common.errors import ModelError
    from kws.libs.models import DepthwiseSeparableConvBlock

    case = (17, 65, 3, 1, 1, 2, 9, 8)
    params, x, _ = build((case, None))
    dev, xd = on_device(params), x.to(DEV)
    want = raw(ctx, case, dev, xd)

    def still_right(after):
        assert torch.equal(raw(ctx, case, dev, xd), want), f"after the refused {after}"

    out = torch.full((4096,), float("nan"), device=DEV)
    # a kernel larger than the padded input: 2 x 3 with padding 1 is 4 x 5 under a 5 x 5 kernel
    small = torch.zeros((1, 17, 2, 3), device=DEV)
    k5 = torch.zeros((17, 1, 5, 5), device=DEV)
    with pytest.raises(ModelError, match=rf"\(code {native.KWS_EINVAL}\)"):
        ctx.dsblock_forward_f32(small, k5, dev[1], dev[2], dev[3], 5, 1, 1, out)
    still_right("oversized kernel")
    blk = DepthwiseSeparableConvBlock(17, 65, kernel_size=5, stride=1, padding=1)
    with pytest.raises(ModelError, match="exceeds the padded input"):
        blk(small)
    # B = 65536 does not fit grid.z: refused by the check, before anything is sized or launched
    many = torch.randn((65536, 1, 1, 1), generator=torch.Generator().manual_seed(65536)).to(DEV)
    one = [torch.ones((1, 1, 1, 1), device=DEV), torch.zeros((1,), device=DEV), torch.ones((1, 1, 1, 1), device=DEV), torch.zeros((1,), device=DEV)]
    with pytest.raises(ModelError, match=rf"\(code {native.KWS_EUNSUPPORTED}\)"):
        ctx.dsblock_forward_f32(many, *one, 1, 1, 0, out)
    still_right("B = 65536")
    most = torch.full((65535,), float("nan"), device=DEV)
    ctx.dsblock_forward_f32(many[:65535], *one, 1, 1, 0, most)  # the largest accepted batch runs: weights 1, biases 0
    ctx.sync()
    assert torch.equal(most, torch.relu(many[:65535].reshape(-1)))
    # NULL weights, one pointer at a time
    ptrs = [int(t.data_ptr()) for t in dev]
    for missing in range(4):
        args = [ctypes.c_void_p(p) if i != missing else None for i, p in enumerate(ptrs)]
        rc = ctx._lib.kws_dsblock_forward_f32(ctx._h, ctypes.c_void_p(xd.data_ptr()), 2, 17, 9, 8, *args, 65, 3, 1, 1,
                                              ctypes.c_void_p(out.data_ptr()))
        assert rc == native.KWS_EINVAL, (missing, rc)
    still_right("NULL weights")
    assert torch.isnan(out).all(), "a refused call wrote to its output"
    # the module: a CPU tensor and a wrong channel count
    blk = DepthwiseSeparableConvBlock(17, 65)
    blk.load_state_dict(params)
    with pytest.raises(ModelError, match="no CPU fallback"):
        blk(x)
    with pytest.raises(ModelError, match=r"expected input \[B,17,H,W\]"):
        blk(torch.zeros(2, 16, 9, 8, device=DEV))
    assert torch.equal(blk(xd).cpu(), want)
