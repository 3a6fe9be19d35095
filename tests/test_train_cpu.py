"""CPU tests of the training path (kws_dscnn_backward_f32): the backward unit is hazard-free at the ISA level and puts its
GEMMs on the f32-input matrix cores, the C ABI declares and binds the entry, and the Python model keeps its CPU contract."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_hazard_lint as lint  # noqa: E402

UNIT = os.path.join(REPO, "keyword-spotting_amd", "csrc", "kws_dscnn_bwd.hip")
PROTO = ("int kws_dscnn_backward_f32(kws_ctx* ctx, const float* d_feat, int B, int T, int F, const float* d_dlogits, "
         "float* d_grad);")


@pytest.mark.skipif(not os.path.exists(lint.HIPCC), reason="hipcc not installed")
def test_backward_unit_is_hazard_free_and_uses_f32_mfma():
    findings, _, isa = lint.lint_file(UNIT)
    flat = [(fn[:60], line, rule, msg) for fn, fs in findings.items() for line, rule, msg in fs]
    assert not flat, flat[:5]
    body = open(isa).read()
    assert re.search(r"v_mfma_f32_(32x32x2|16x16x4)_f32", body), "the pointwise GEMMs must run on an f32-input MFMA"
    for k in ("kws_bwd_fc_kernel", "kws_bwd_pointwise_kernel", "kws_bwd_depthwise_kernel", "kws_bwd_conv1_kernel",
              "kws_bwd_reduce_kernel"):
        assert k in body, f"kernel {k} missing (rocprofv3 attributes time by these names)"


def test_header_declares_the_backward_entry():
    text = open(os.path.join(REPO, "include", "kws_hip.h")).read()
    assert PROTO in re.sub(r"\s+", " ", text)
    assert "#define KWS_ABI_VERSION 1" in text


def test_backward_entry_is_bound():
    native = pytest.importorskip("kws._native")
    assert native.SIGNATURES["kws_dscnn_backward_f32"][1][2:5] == [native.C.c_int] * 3
    assert hasattr(native.Context, "dscnn_backward_f32")
    if os.path.exists(native.LIB_PATH):
        assert hasattr(native.lib(), "kws_dscnn_backward_f32")


def test_packed_weights_match_the_oracle_blob():
    from kws.libs.models import DepthwiseSeparableConv
    from oracle import dscnn as o_dscnn

    torch.manual_seed(3)
    m = DepthwiseSeparableConv()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    a = m.packed_weights()
    b = o_dscnn.flatten_state(m.state_dict())
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()


def test_training_forward_without_gpu_still_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kws.common.errors import ModelError
    from kws.libs.models import DepthwiseSeparableConv

    m = DepthwiseSeparableConv()
    assert torch.is_grad_enabled() and all(p.requires_grad for p in m.parameters())
    with pytest.raises(ModelError, match="no CPU fallback"):
        m(torch.zeros(2, 1, 99, 10))
    assert m.train()._autograd  # the autograd dispatch refuses the CPU tensor as the plain one does
    with pytest.raises(ModelError, match=r"DepthwiseSeparableConv\.forward needs a CUDA/ROCm tensor.*no CPU fallback"):
        m(torch.zeros(2, 1, 99, 10))
    with pytest.raises(ModelError, match=r"DepthwiseSeparableConv\.infer_pcm16 needs a CUDA/ROCm tensor.*no CPU fallback"):
        m.infer_pcm16(torch.zeros(2, 16000, dtype=torch.int16))


def test_both_trainable_models_dispatch_to_one_function(monkeypatch):
    """After train(), under grad mode, the forward of either model hands itself, the input and its parameters to the same
    torch.autograd.Function -- the only one of the module."""
    from kws.libs import models

    fns = [v for v in vars(models).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function)]
    assert fns == [models._NativeTrainFunction]

    class OnGpu:  # what forward looks at before it dispatches
        is_cuda = True
        shape = (2, 1, 99, 10)

        def dim(self):
            return 4

    calls = []
    monkeypatch.setattr(models._NativeTrainFunction, "apply",
                        staticmethod(lambda model, x, *params: calls.append((model, x, params)) or ("logits", "labels")))
    x = OnGpu()
    for cls in (models.DepthwiseSeparableConv, models.CnnTradFpool3):
        m = cls().train()
        assert m(x) == "logits" and m(x, return_labels=True) == ("logits", "labels")
        model, got, params = calls[-1]
        mine = list(m.parameters())
        assert model is m and got is x and len(params) == len(mine) and all(a is b for a, b in zip(params, mine))
    assert len(calls) == 4


def test_split_flat_grad_pieces_are_the_slices():
    from kws.libs.models import split_flat_grad

    params = [torch.zeros(2, 3), torch.zeros(4, dtype=torch.float64), torch.zeros(1, 1, 2)]
    flat = torch.arange(12, dtype=torch.float32) * 0.37 - 2.0
    pieces = split_flat_grad(flat, params)
    assert len(pieces) == 3
    off = 0
    for g, p in zip(pieces, params):
        assert g.shape == p.shape and g.dtype == p.dtype and g.device == p.device
        assert torch.equal(g.reshape(-1), flat[off:off + p.numel()].to(p.dtype))
        off += p.numel()
    assert off == flat.numel()


@pytest.mark.parametrize("T,F,C", [(99, 10, 12), (20, 8, 35), (7, 7, 1)])
def test_pinned_relu_oracle_equals_the_unpinned_one(T, F, C):
    """The float64 oracle with its ReLU decisions pinned to those of its own forward gives the same logits, stage outputs
    and gradients, bit for bit; a mask taken from elsewhere is honoured (a unit switched off passes nothing)."""
    from oracle import dscnn as o_dscnn

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gen = torch.Generator().manual_seed(T * F + C)
    state = o_dscnn.random_state(9, num_classes=C)
    x = torch.randn(5, 1, T, F, generator=gen, dtype=torch.float64)
    x[1] = 0.0  # all-zero clip: conv1 is its bias everywhere
    dl = torch.randn(5, C, generator=gen, dtype=torch.float64)
    logits, layers = o_dscnn.forward(state, x, return_layers=True)
    masks = o_dscnn.relu_masks(layers)
    assert all(0 < int(m.sum()) < m.numel() for m in masks.values())
    pl, players = o_dscnn.forward(state, x, return_layers=True, masks=masks)
    assert torch.equal(pl, logits)
    for k in layers:
        assert torch.equal(players[k], layers[k]), k
    g, gp = o_dscnn.grads(state, x, dl), o_dscnn.grads(state, x, dl, masks=masks)
    for k in o_dscnn.STATE_KEYS:
        assert np.array_equal(g[k], gp[k]), k
    # the masks decide: switch every unit of block 2 off -> blocks 3, 4 see only their biases and nothing flows below
    off = dict(masks, dsconv2=torch.zeros_like(masks["dsconv2"]))
    gd = o_dscnn.grads(state, x, dl, masks=off)
    for k in ("conv1.weight", "conv1.bias", "dsconv1.depthwise.weight", "dsconv2.pointwise.weight", "dsconv2.pointwise.bias"):
        assert not gd[k].any(), k
    with pytest.raises(ValueError, match="mask conv1"):
        o_dscnn.forward(state, x, masks=dict(masks, conv1=masks["conv1"][:, :, 1:]))
