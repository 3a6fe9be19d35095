"""CPU tests of the BatchNorm DS-CNN's training path (kws_dscnn_bn_train_forward_f32 / kws_dscnn_bn_backward_f32): the blob layout
against ``DepthwiseSeparableConvBN.parameters()``, the tests' own reference against the oracle, the host-only batch limit, the
binding, and the model's CPU contract."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import _bn_train_ref as ref  # noqa: E402
import isa_hazard_lint as lint  # noqa: E402

ENTRIES = ("kws_dscnn_bn_train_forward_f32", "kws_dscnn_bn_backward_f32", "kws_dscnn_bn_train_debug_f32", "kws_host_dscnn_bn_max_batch")


@pytest.mark.parametrize("C", [1, 12, 64])
def test_blob_layout_is_parameters_order(C):
    """Offsets and sizes of the entries' blob = named_parameters() of the model, tensor by tensor; n_floats = 25664 + 65 C + 1152.
    The C++ side (DscnnBnLayout) states the same offsets: plain blob first, then nine (weight, bias) pairs, conv1, dw 0..3, pw 0..3."""
    native = pytest.importorskip("kws._native")
    from kws.libs.models import DepthwiseSeparableConvBN

    m = DepthwiseSeparableConvBN(num_classes=C)
    layout = native.dscnn_bn_blob_layout(C)
    named = list(m.named_parameters())
    assert [n for n, _, _ in layout] == [n for n, _ in named] == list(ref.param_shapes(C))
    off = 0
    for (name, o, n), (_, p) in zip(layout, named):
        assert (o, n) == (off, p.numel()), name
        assert tuple(p.shape) == ref.param_shapes(C)[name], name
        off += n
    assert off == 25664 + 65 * C + 1152 == sum(p.numel() for p in m.parameters())
    assert layout[20][:2] == ("bn_conv1.weight", 25664 + 65 * C)
    # the order of the statistics (data flow) against the blob's module order
    assert [mod for mod in m.bn_layers()] == [m.bn_conv1, m.bn_dw[0], m.bn_pw[0], m.bn_dw[1], m.bn_pw[1], m.bn_dw[2], m.bn_pw[2],
                                               m.bn_dw[3], m.bn_pw[3]]
    pack = open(os.path.join(REPO, "keyword-spotting_amd", "csrc", "kws_pack.h")).read()
    assert "struct DscnnBnLayout" in pack and "BN_FLOATS = N_BN * 2 * CO" in pack


def test_reference_in_train_mode_equals_the_oracle_at_batch_statistics():
    """The tests' restatement, train mode, against oracle.dscnn.forward_bn given the batch statistics as running ones (the biased
    variance: what the normalisation uses)."""
    from oracle import dscnn as o_dscnn

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for seed, (B, T, F, C) in enumerate([(5, 20, 7, 12), (3, 6, 9, 1), (2, 99, 10, 35)]):
        p = ref.random_params(40 + seed, C)
        x = torch.randn(B, 1, T, F, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        logits, acts, stats = ref.forward(p, x, eps=1e-5)
        assert len(acts) == 5 and stats.shape == (9, 2, 64)
        state = {k[len("plain."):]: v.double() for k, v in p.items() if k.startswith("plain.")}
        H1, W1 = (T - 6) // 2 + 1, (F - 6) // 2 + 1
        bn = {}
        for i, layer in enumerate(ref.LAYERS):
            k = (i + 1) // 2  # positions of the layer: conv1 and dw_k see H(k-1) x W(k-1), pw_k its ringed output
            n = B * (H1 + 2 * k) * (W1 + 2 * k) if layer.startswith("pw") else B * (H1 + 2 * max(k - 1, 0)) * (W1 + 2 * max(k - 1, 0))
            biased = stats[i, 1] * ((n - 1) / n)
            bn[layer] = (p[ref.BN_OF[layer] + ".weight"].double(), p[ref.BN_OF[layer] + ".bias"].double(), stats[i, 0], biased)
        want = o_dscnn.forward_bn(state, bn, x, eps=1e-5)
        assert float((logits - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())), (B, T, F)
        # pinning the ReLU decisions to the forward's own changes nothing
        l2, a2, s2 = ref.forward(p, x, eps=1e-5, masks=[a > 0 for a in acts])
        assert torch.equal(l2, logits) and torch.equal(s2, stats) and all(torch.equal(u, v) for u, v in zip(a2, acts))


def test_exact_conv_bias_gradients_vanish_and_the_floor_is_positive():
    """Under a train-mode BatchNorm the gradient of the bias before it is zero: float64 gives rounding noise far below the floor
    the GPU test grants (1e-6 of the magnitude that cancels)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    p = ref.random_params(3, 12)
    gen = torch.Generator().manual_seed(1)
    x, dl = torch.randn(4, 1, 20, 7, generator=gen), torch.randn(4, 12, generator=gen)
    g, cancels = ref.grads(p, x, dl, torch.float64)
    for layer in ref.LAYERS:
        assert cancels[layer] > 0
        assert np.abs(g[ref.CONV_OF[layer] + ".bias"]).max() <= 1e-9 * cancels[layer], layer
        assert np.abs(g[ref.CONV_OF[layer] + ".weight"]).max() > 0


@pytest.mark.skipif(not os.path.exists(lint.HIPCC), reason="hipcc not installed")
def test_unit_is_hazard_free_and_names_its_kernels():
    findings, _, isa = lint.lint_file(os.path.join(REPO, "keyword-spotting_amd", "csrc", "kws_dscnn_bn.hip"))
    flat = [(fn[:60], line, rule, msg) for fn, fs in findings.items() for line, rule, msg in fs]
    assert not flat, flat[:5]
    body = open(isa).read()
    for k in ("kws_bn_stats_kernel", "kws_bn_finish_kernel", "kws_bn_apply_kernel", "kws_bn_bwd_stats_kernel", "kws_bn_bwd_finish_kernel",
              "kws_bn_bwd_apply_kernel", "kws_bn_c1_transpose_kernel"):
        assert k in body, f"kernel {k} missing (rocprofv3 attributes time by these names)"
    assert "v_add_f64" in body or "v_fma_f64" in body, "the batch sums are taken in float64"
    assert "atomic" not in body, "no atomics: partial rows are reduced in a fixed order"
    # the switched kernels live beside their originals, under their own names
    for unit, names in (("kws_dsblock.hip", ("kws_conv1_any_pre_kernel", "kws_dsblock_pointwise_pre_kernel")),
                        ("kws_dscnn_bwd.hip", ("kws_bwd_pointwise_dz_kernel", "kws_bwd_conv1_dz_kernel"))):
        text = open(lint.compile_to_isa(os.path.join(REPO, "keyword-spotting_amd", "csrc", unit))).read()
        assert all(n in text for n in names), unit


def test_max_batch_and_bindings():
    native = pytest.importorskip("kws._native")
    for n in ENTRIES:
        assert n in native.SIGNATURES, n
    assert native.SIGNATURES["kws_dscnn_bn_backward_f32"][1][2] is native.C.c_size_t
    assert native.SIGNATURES["kws_dscnn_bn_backward_f32"][1][8] is native.C.c_float
    assert hasattr(native.Context, "dscnn_bn_train_forward_f32") and hasattr(native.Context, "dscnn_bn_backward_f32")
    text = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "kws_hip.h")).read())
    assert ("int kws_dscnn_bn_backward_f32(kws_ctx* ctx, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, "
            "int B, int T, int F, float eps, const float* d_dlogits, float* d_grad);") in text
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("library not built")
    assert 4096 <= native.host_dscnn_bn_max_batch(99, 10) <= 16384
    assert native.host_dscnn_bn_max_batch(6, 6) == 16384       # small maps: the composed path's clip limit
    assert native.host_dscnn_bn_max_batch(5, 10) == 0 and native.host_dscnn_bn_max_batch(99, 5) == 0  # maps the entries refuse
    big = native.host_dscnn_bn_max_batch(156, 252)
    assert 1 <= big < native.host_dscnn_bn_max_batch(99, 10)


def test_cpu_tensor_is_refused_in_both_modes():
    from kws.common.errors import ModelError
    from kws.libs.models import DepthwiseSeparableConvBN

    m = DepthwiseSeparableConvBN()
    assert m.training and not m._autograd  # nn.Module's default alone switches nothing
    if not torch.cuda.is_available():
        with pytest.raises(ModelError, match="no CPU fallback"):
            m(torch.zeros(2, 1, 99, 10))
    assert m.train()._autograd and not m.eval()._autograd and m.train()._autograd
    with pytest.raises(ModelError, match=r"DepthwiseSeparableConvBN\.forward needs a CUDA/ROCm tensor.*no CPU fallback"):
        m(torch.zeros(2, 1, 99, 10))
    assert all(int(b.num_batches_tracked) == 0 for b in m.bn_layers())
    assert not m.train(False)._autograd


def test_unsupported_batchnorm_settings_raise():
    from kws.common.errors import ModelError
    from kws.libs.models import DepthwiseSeparableConvBN

    m = DepthwiseSeparableConvBN().train()
    m.bn_pw[2].momentum = None
    with pytest.raises(ModelError, match="momentum=None"):
        m._eps()
    m = DepthwiseSeparableConvBN().train()
    m.bn_dw[1] = torch.nn.BatchNorm2d(64, track_running_stats=False)
    with pytest.raises(ModelError, match="track_running_stats=False"):
        m._eps()
    m = DepthwiseSeparableConvBN(eps=1e-3).train()
    assert m._eps() == 1e-3
