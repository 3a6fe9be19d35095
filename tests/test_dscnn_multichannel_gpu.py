"""DepthwiseSeparableConv(input_channels > 1) at its edges.  Two routes compute it: the composed path (kws_conv1_any_kernel with
the padded plane restaged per channel, then the block kernels) and, at 99 x 10, kws_conv1_general_kernel into the workspace
followed by the fused kernel's PRECONV instantiations ({4, F_PRECONV} and {5, F_PRECONV} of kFwdVariants).  The f16-pair one
measures conv1's largest output while staging it and derives block 1's scale from that, in true units, which no
single-channel variant does.

The truth is oracle.dscnn.forward in float64; e_f32 is the same oracle in float32.  The gates are the suite's own:
LAYER_RTOL / TOL for the composed path (tests/_dscnn_forward.py), and per clip, for the fused kernels, the rule of
test_dscnn_f16_pair_arithmetic_holds_over_range: e <= max(4 e_f32, 2e-6 scale), two f32-grade results (pair and triple, fused
and composed) within max(3e-6 scale, 8 e_f32) of each other, scale = max(1, max|float64 logits of the clip|)."""
import os

import numpy as np
import pytest
import torch

from _dscnn_forward import DEV, check_class_counts, check_forward, fused_case, geometry, he_scale, load_state
from oracle import dscnn as o_dscnn

pytestmark = pytest.mark.gpu

MATHS = [4, 5]  # KWS_PW_SPLIT_BF16, KWS_PW_PAIR_F16
MATH_IDS = ["bf16_triple", "f16_pair"]


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
    c.set_pointwise_math(native.PW_DEFAULT)
    c.close()


def he_state(seed, C, cin, fc_std=0.5, bias_gain=0.1):
    """N(0, 1) parameters, the convolutions He-scaled (conv1 by its 100 cin taps: stage magnitudes do not grow with cin), biases
    N(0, bias_gain), fc.weight N(0, fc_std)."""
    state = he_scale(o_dscnn.random_state(seed, num_classes=C, std=1.0, input_channels=cin), bias_gain)
    state["fc.weight"] = state["fc.weight"] * fc_std
    return state


def fused(ctx, xd, C, math, guard=False):
    """kws_forward_f32 under ``math`` -> (logits, labels) on the CPU.  ``guard``: the logits go into a NaN-filled [B + 1, C]
    buffer, whose last row must stay NaN."""
    B = xd.shape[0]
    logits = torch.full((B + 1, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ctx.set_pointwise_math(math)
    ctx.forward_f32(xd, logits, labels)
    ctx.sync()
    if guard:
        assert torch.isnan(logits[B]).all(), "logits were written beyond [B, C]"
    return logits[:B].cpu(), labels.cpu()


def composed(ctx, xd, C):
    """The composed path at 99 x 10 (kws_forward_map_debug_f32 runs it whatever the map) -> logits on the CPU."""
    B, _, T, F = xd.shape
    layers = torch.empty((B * sum(int(np.prod(s)) for s in geometry(T, F)),), device=DEV)
    logits = torch.empty((B, C), device=DEV)
    ctx.forward_map_f32(xd, logits, None, layers=layers)
    ctx.sync()
    return logits.cpu()


def range_rule(out, ref64, ref32, what):
    """The suite's per-clip rule on ``out`` = {name: float64 logits}; 'pair' and 'triple' against float64, every other pair of
    entries against each other.  Returns the worst error / gate ratio of each kind."""
    worst = {"f64": 0.0, "mutual": 0.0}
    names = list(out)
    for k, v in out.items():
        assert torch.isfinite(v).all(), (what, k)
    for i in range(ref64.shape[0]):
        scale = max(1.0, float(ref64[i].abs().max()))
        e_f32 = float((ref32[i].double() - ref64[i]).abs().max())
        for k in ("pair", "triple"):
            e = float((out[k][i] - ref64[i]).abs().max())
            gate = max(4.0 * e_f32, 2e-6 * scale)
            worst["f64"] = max(worst["f64"], e / gate)
            assert e <= gate, (what, k, i, e, e_f32, scale)
        for a in range(len(names)):
            for b in range(a + 1, len(names)):
                d = float((out[names[a]][i] - out[names[b]][i]).abs().max())
                gate = max(3e-6 * scale, 8.0 * e_f32)
                worst["mutual"] = max(worst["mutual"], d / gate)
                assert d <= gate, (what, names[a], names[b], i, d, e_f32, scale)
    return worst


# ------------------------------------------------------------------------------------------------- 1. composed path
@pytest.mark.parametrize("cin,T,F,B", [(2, 99, 10, 5), (3, 6, 6, 17), (17, 22, 20, 5), (64, 20, 8, 3), (2, 125, 124, 2)],
                         ids=["2ch-99x10", "3ch-6x6", "17ch-22x20", "64ch-20x8", "2ch-125x124"])
def test_composed_path_stage_by_stage(native, ctx, cin, T, F, B):
    """kws_conv1_any_kernel with the plane restaged per channel -- conv1's output 1 x 1 at 6 x 6, a tile and a remainder at
    22 x 20, the full 64 channels, and 125 x 124, whose padded plane (129 x 128 floats) is over 64 KB of dynamic LDS -- then
    the blocks: check_forward's rules unchanged, and every float of the NaN-filled stage dump written."""
    state = he_state(1000 * cin + T, 12, cin)
    x = torch.randn(B, cin, T, F, generator=torch.Generator().manual_seed(cin + T + F))
    x[B - 1, cin - 1] = 0.0  # one silent channel
    _, _, stages, _ = check_forward(ctx, state, x, f"{cin}ch {T}x{F}")
    for k, v in stages.items():
        assert torch.isfinite(v).all(), f"stage {k}: {int((~torch.isfinite(v)).sum())} floats not written"


# ------------------------------------------------------------------------------------------------- 2. PRECONV kernels
@pytest.mark.parametrize("cin", [2, 3, 7, 64])
def test_fused_preconv_kernels_against_float64(native, ctx, cin):
    """kws_conv1_general_kernel + both PRECONV instantiations at 99 x 10 against float64, per clip, and against the composed
    path's logits for the same clips: two independent routes to one function."""
    B, C = 24, 12
    state = he_state(2000 + cin, C, cin)
    x = torch.randn(B, cin, 99, 10, generator=torch.Generator().manual_seed(20 + cin))
    x *= torch.tensor([1.0, 0.1, 5.0, 30.0]).repeat(B // 4).reshape(B, 1, 1, 1)
    x[3] = 0.0
    x[5, 0] = 0.0          # a silent first channel
    x[6, cin - 1] = 0.0    # a silent last channel
    x[7] = x[7].abs()
    ref64 = o_dscnn.forward(state, x.double())
    ref32 = o_dscnn.forward(state, x)
    load_state(ctx, state)
    xd = x.to(DEV)
    out = {"pair": fused(ctx, xd, C, native.PW_PAIR_F16, guard=True)[0].double(),
           "triple": fused(ctx, xd, C, native.PW_SPLIT_BF16, guard=True)[0].double(),
           "composed": composed(ctx, xd, C).double()}
    worst = range_rule(out, ref64, ref32, f"cin={cin}")
    print(f"PRECONV kernels, cin={cin}: worst error/gate vs float64 {worst['f64']:.3f}, mutual {worst['mutual']:.3f}")


# ------------------------------------------------------------------------------------------------- 3. class counts
_CASES = {}


def _case3(C):
    if C not in _CASES:
        _CASES[C] = fused_case(C, input_channels=3)
    return _CASES[C]


@pytest.mark.parametrize("mode", MATHS, ids=MATH_IDS)
@pytest.mark.parametrize("C", [1, 2, 35, 64])
def test_preconv_class_counts(native, ctx, C, mode):
    """The classifier wavefront of the PRECONV instantiations: class c on lane c, the first maximum over 16-lane rows -- with
    the assertions (and the asserted preconditions) of test_fused_kernel_class_counts on a three-channel model."""
    check_class_counts(native, ctx, C, mode, _case3(C))


# ------------------------------------------------------------------------------------------------- 4. range
def _range_clips():
    torch.manual_seed(43)
    x = torch.randn(24, 3, 99, 10) * 6.0
    x[0] = 0.0
    x[1] *= 1e-3
    x[2] *= 1e3
    x[3] *= 40.0
    x[4, :, 50:] = 0.0
    x[5] = torch.randn(3, 99, 10) * 0.01
    x[5, 1, 40, 3] = 3000.0
    x[6] = 7.5
    x[7] = -x[7].abs()
    x[8, 1] = 0.0          # one channel silent, the others large
    x[8, 0] *= 100.0
    x[8, 2] *= 100.0
    x[9, 0] = 0.0
    x[9, 1] = 0.0          # only the last channel carries anything
    return x


RANGE_CASES = [(1.0, 1.0), (6.0, 1.0), (0.1, 1.0), (1.0, 200.0), (1.0, 0.0), (1e-9, 0.0), (300.0, 1e6), (-5.0, 1.0),
               "conv1_dead", "conv1_dead_no_bias"]


@pytest.mark.parametrize("case", RANGE_CASES, ids=[str(c).replace(" ", "") for c in RANGE_CASES])
def test_preconv_arithmetic_holds_over_range(native, ctx, case):
    """The range test's clips (three channels) and weight / bias gains on the PRECONV kernels.  The f16-pair kernel measures
    conv1's output, so two cases exist only here: conv1 biases all <= 0 under the all-zero clip (conv1's output is exactly zero,
    the measured maximum is 0), and the same with every later bias zero (the bound on block 1 is 0: the exponent clamps)."""
    x = _range_clips()
    state = he_state(4000, 12, 3)
    if isinstance(case, tuple):
        w_gain, b_gain = case
        cancel = w_gain < 0
        for k in state:
            if k.endswith("weight") and not k.startswith("fc") and not cancel:
                state[k] = state[k] * (w_gain if "pointwise" in k or k.startswith("conv1") else 1.0)
            if k.endswith("bias") and not k.startswith("fc"):
                state[k] = (state[k] + 0.01) * b_gain
        if cancel:  # every pointwise row alternates +5, -5 plus the random part: sum|w| is far above |sum w|
            for i in range(1, 5):
                alt = torch.tensor([1.0, -1.0]).repeat(32).reshape(1, 64, 1, 1) * abs(w_gain)
                state[f"dsconv{i}.pointwise.weight"] = alt.expand(64, 64, 1, 1).clone() + state[f"dsconv{i}.pointwise.weight"]
    else:
        state["conv1.bias"] = -state["conv1.bias"].abs() - 0.01
        if case == "conv1_dead_no_bias":
            for k in state:
                if k.endswith("bias") and k.startswith("dsconv"):
                    state[k] = torch.zeros_like(state[k])
    ref64, layers = o_dscnn.forward(state, x.double(), return_layers=True)
    ref32 = o_dscnn.forward(state, x)
    if not isinstance(case, tuple):
        assert float(layers["conv1"][0].abs().max()) == 0.0, "the zero clip must leave conv1's output exactly zero"
    load_state(ctx, state)
    xd = x.to(DEV)
    out = {"pair": fused(ctx, xd, 12, native.PW_PAIR_F16, guard=True)[0].double(),
           "triple": fused(ctx, xd, 12, native.PW_SPLIT_BF16, guard=True)[0].double()}
    worst = range_rule(out, ref64, ref32, str(case))
    print(f"PRECONV range {case}: worst error/gate vs float64 {worst['f64']:.3f}, pair vs triple {worst['mutual']:.3f}")


# ------------------------------------------------------------------------------------------------- 5. clip independence
POOL = 13  # distinct clips; batch position i holds clip (7 i + shift) % POOL, as tests/test_dscnn_persistent_gpu.py


@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((POOL, 3, 99, 10)).astype(np.float32) * 8.0
    x[1] *= 3.0e4    # huge
    x[4] = 0.0       # all zero: every stage is bias only
    x[6] *= 1.0e-20  # tiny
    x[9] = 0.0
    x[9, 2, 50, 5] = -1.0e3  # one spike
    x[11] *= 2.0e3
    return torch.from_numpy(x).to(DEV)


@pytest.mark.parametrize("math", MATHS, ids=MATH_IDS)
def test_preconv_every_clip_matches_itself_alone(native, ctx, pool, math):
    """A workgroup's measured maximum, scale slots and tables belong to its clip alone: every clip's logits and label are
    bit-identical to the same clip run alone, at batch sizes around the CU count, and again at a smaller batch after the
    workspace has grown."""
    C = load_state(ctx, he_state(5000, 12, 3))
    alone = [fused(ctx, pool[i:i + 1].contiguous(), C, math, guard=True) for i in range(POOL)]
    ref_logits = np.concatenate([a[0].numpy() for a in alone])
    ref_labels = np.concatenate([a[1].numpy() for a in alone])
    assert np.isfinite(ref_logits).all()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for B, shift in [(1, 3), (2, 0), (n_cu - 1, 1), (n_cu, 2), (n_cu + 1, 5), (2 * n_cu + 3, 4), (n_cu - 3, 6)]:
        idx = (7 * np.arange(B) + shift) % POOL
        logits, labels = fused(ctx, pool[torch.from_numpy(idx).to(DEV)].contiguous(), C, math, guard=True)
        bad = np.flatnonzero((logits.numpy().view(np.uint32) != ref_logits[idx].view(np.uint32)).any(axis=1))
        assert bad.size == 0, f"B={B}: {bad.size} clips differ from the same clip alone, first at {bad[:5]} (pool {idx[bad[:5]]})"
        np.testing.assert_array_equal(labels.numpy(), ref_labels[idx], err_msg=f"B={B}")


# ------------------------------------------------------------------------------------------------- 6. model swaps
def test_model_swaps_on_one_context(native, ctx):
    """input_channels 3 -> 1 -> 2 -> 3 with different class counts on one context, by kws_load_dscnn and kws_load_dscnn_device in
    turn: after each load the fused kernels (both maths) and the composed path give the bits of a fresh context that only
    ever held that model -- no conv1 image, channel count or weight image of the previous model survives."""
    def run(c, state, x):
        C = int(state["fc.weight"].shape[0])
        xd = x.to(DEV)
        small = xd[:, :, :22, :].contiguous()
        lm = torch.full((x.shape[0], C), float("nan"), device=DEV)
        c.forward_map_f32(small, lm, None)
        c.sync()
        return [fused(c, xd, C, m, guard=True) for m in MATHS] + [(lm.cpu(), None)]

    for step, (cin, C, device) in enumerate([(3, 12, False), (1, 5, True), (2, 35, False), (3, 7, True)]):
        state = he_state(6000 + step, C, cin)
        x = torch.randn(5, cin, 99, 10, generator=torch.Generator().manual_seed(60 + step)) * 3.0
        load_state(ctx, state, device=device)
        got = run(ctx, state, x)
        fresh = native.Context(0)
        fresh.use_torch_stream()
        try:
            load_state(fresh, state)
            want = run(fresh, state, x)
        finally:
            fresh.close()
        for k, ((gl, gb), (wl, wb)) in enumerate(zip(got, want)):
            assert torch.isfinite(wl).all()
            assert torch.equal(gl, wl), f"step {step} (cin {cin}, C {C}) route {k}: logits differ from a fresh context"
            assert gb is None or torch.equal(gb, wb), (step, k)


# ------------------------------------------------------------------------------------------------- 7. surface
def test_multichannel_refusals_leave_the_context_usable(native, ctx):
    """What exists for one input channel only returns KWS_EUNSUPPORTED under a multi-channel model, and the next product call
    on the same context gives the bits it gave before."""
    from kws.common.errors import ModelError

    C, B = 12, 4
    load_state(ctx, he_state(7000, C, 3))
    xd = torch.randn(B, 3, 99, 10, generator=torch.Generator().manual_seed(70)).to(DEV)
    before = fused(ctx, xd, C, native.PW_PAIR_F16)
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    act = torch.zeros((B, native.ACT_FLOATS_PER_CLIP), device=DEV)
    stamps = torch.zeros((B, 16), dtype=torch.int64, device=DEV)
    wav = torch.zeros((B, 16000), dtype=torch.int16, device=DEV)
    pcm = torch.zeros((1, 32000), dtype=torch.int16, device=DEV)
    n_win = native.host_scan_shape(32000, 400, 160, 99, 10)[1]
    scan_logits = torch.full((1, n_win, C), float("nan"), device=DEV)
    grad = torch.full((6400 * 3 + 64 + 4 * 4800 + 65 * C,), float("nan"), device=DEV)
    dl = torch.zeros((B, C), device=DEV)

    def f32_math():
        ctx.set_pointwise_math(native.PW_F32)
        try:
            ctx.forward_f32(xd, logits, labels)
        finally:
            ctx.set_pointwise_math(native.PW_DEFAULT)

    ctx.stream_open(B)
    try:
        calls = {
            "forward_debug_f32": lambda: ctx.forward_debug_f32(xd, logits, labels, act, use_mfma=native.PW_SPLIT_BF16),
            "forward_stamps_f32": lambda: ctx.forward_stamps_f32(xd, logits, stamps, native.PW_PAIR_F16),
            "forward_f32 under PW_F32": f32_math,
            "infer_i16": lambda: ctx.infer_i16(wav, logits, labels),
            "infer_f32": lambda: ctx.infer_f32(wav.float(), logits, labels),
            "stream_push_i16": lambda: ctx.stream_push_i16(wav[:, :160].contiguous(), logits, labels),
            "scan_i16": lambda: ctx.scan_i16(pcm, 10, scan_logits),
            "dscnn_backward_f32": lambda: ctx.dscnn_backward_f32(xd, 99, 10, dl, grad),
        }
        for name, call in calls.items():
            with pytest.raises(ModelError, match=rf"\(code {native.KWS_EUNSUPPORTED}\)"):
                call()
            ctx.sync()
            after = fused(ctx, xd, C, native.PW_PAIR_F16)
            assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]), f"after the refused {name}"
    finally:
        ctx.stream_close()
    # nothing was launched into the callers' buffers
    assert torch.isnan(logits).all() and (labels == -1).all() and torch.isnan(scan_logits).all() and torch.isnan(grad).all()
    assert not act.any() and not stamps.any()


def test_multichannel_python_surface(native):
    from kws.common.errors import ModelError
    from kws.libs.models import DepthwiseSeparableConv

    for bad in (0, 65):
        with pytest.raises(ModelError, match="input_channels"):
            DepthwiseSeparableConv(num_classes=5, input_channels=bad)
    torch.manual_seed(8)
    m = DepthwiseSeparableConv(num_classes=5, input_channels=4)
    with torch.no_grad():
        for p in m.parameters():  # the default init has zero biases
            if p.dim() == 1:
                p.normal_(0.0, 0.1)
    m = m.to(DEV).eval()
    x = torch.randn(6, 4, 99, 10, generator=torch.Generator().manual_seed(9)).to(DEV)
    logits, labels = m(x, return_labels=True)
    assert logits.grad_fn is None and not logits.requires_grad
    direct = native.Context(0)
    direct.use_torch_stream()
    try:
        direct.load_dscnn(m.packed_weights(), 5, 4)
        want = fused(direct, x, 5, native.PW_DEFAULT, guard=True)
    finally:
        direct.close()
    assert torch.equal(logits.cpu(), want[0]) and torch.equal(labels.cpu(), want[1])
    ref = o_dscnn.forward({k: v.detach().cpu() for k, v in m.state_dict().items()}, x.cpu().double())
    assert float((logits.cpu().double() - ref).abs().max()) <= 1e-4
    # the wrong channel count is refused before any launch (no context call is reached)
    for shape in ((2, 1, 99, 10), (2, 3, 99, 10), (2, 5, 20, 20)):
        with pytest.raises(ModelError, match=r"expected input \[B,4,T,F\]"):
            m(torch.zeros(shape, device=DEV))
    # train(): the forward works and gives the same bits; the backward names what it cannot do
    m.train()
    out = m(x)
    assert out.grad_fn is not None and torch.equal(out.detach().cpu(), want[0])
    with pytest.raises(ModelError, match="input_channels"):
        out.sum().backward()
    m.eval()
    assert torch.equal(m(x).cpu(), want[0])  # and the model is still usable
