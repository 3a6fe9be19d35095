"""cnn-trad-fpool3 inference (kws_forward_cnn_trad_f32: kws_cnntrad_conv_kernel + kws_cnntrad_dense_kernel) stage by stage, through
the parity aid kws_forward_cnn_trad_debug_f32, which runs the product's two launches and copies out what sits between them: conv2
after ReLU and, under the f16-pair arithmetic, the per-clip power-of-two scale.  Reference: oracle/cnn_trad.py in float64 on the CPU.

Accuracy rule of the project (test_cnn_trad_f16_pair_arithmetic_holds_over_range, test_cnntrad_f16_pair_sim.py), applied per clip
and per stage: err <= max(4 e_f32, 2e-6 scale), e_f32 = the error of torch's own float32 CPU evaluation of the same stage against
float64, scale = max(1, max|ref64|).  Every comparison prints its worst err / tol.  Unless a test says otherwise it runs under both
arithmetics, KWS_CT_F16_PAIR and KWS_CT_BF16_TRIPLE."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kws import _native
from oracle import cnn_trad as o_ct

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PAIR, TRIPLE = _native.KWS_CT_F16_PAIR, _native.KWS_CT_BF16_TRIPLE
MATHS = [pytest.param(PAIR, id="f16_pair"), pytest.param(TRIPLE, id="bf16_triple")]
SENTINEL = -7.0  # what the scale buffer holds before a call: no power of two


@pytest.fixture(scope="module")
def ctx():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    c = _native.Context(0)
    yield c
    c.close()


def _state(kind, C=12, seed=1):
    from kws.libs.models import CnnTradFpool3

    if kind == "random":
        return o_ct.random_state(seed, num_classes=C)
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in CnnTradFpool3(C).state_dict().items()}


def _run(ctx, math, x, C, want_label=True):
    """The debug entry under `math` on the loaded model: (logits, labels or None, conv2, clip scales) on the CPU."""
    B = x.shape[0]
    xd = x.to(DEV).contiguous()
    logits = torch.full((B, C), float("nan"), device=DEV)
    label = torch.full((B,), -1, dtype=torch.int32, device=DEV) if want_label else None
    conv2 = torch.full((B, 64, 99, 3), float("nan"), device=DEV)
    scale = torch.full((B,), SENTINEL, device=DEV)
    ctx.set_cnn_trad_math(math)
    try:
        ctx.forward_cnn_trad_debug_f32(xd, logits, label, conv2, scale)
        ctx.sync()
    finally:
        ctx.set_cnn_trad_math(PAIR)
    assert torch.isfinite(logits).all() and torch.isfinite(conv2).all()
    if math == TRIPLE:
        assert bool((scale == SENTINEL).all()), "the scale buffer is left untouched under KWS_CT_BF16_TRIPLE"
    if want_label:
        assert int(label.min()) >= 0 and int(label.max()) < C
    return logits.cpu(), (label.cpu() if want_label else None), conv2.cpu(), scale.cpu()


def _ratios(got, ref64, ref32):
    """Per clip err / tol of the project's rule; every argument [B, ...]."""
    B = got.shape[0]
    got, ref64, ref32 = (t.reshape(B, -1).double() for t in (got, ref64, ref32))
    err = (got - ref64).abs().amax(1)
    e32 = (ref32 - ref64).abs().amax(1)
    scale = ref64.abs().amax(1).clamp_min(1.0)
    tol = torch.maximum(4.0 * e32, 2e-6 * scale)
    return (err / tol).numpy(), tol.numpy()


def _check(what, got, ref64, ref32):
    r, tol = _ratios(got, ref64, ref32)
    print(f"{what}: worst err/tol = {r.max():.3f} (clip {int(r.argmax())})")
    assert r.max() <= 1.0, f"{what}: clip {int(r.argmax())} err/tol = {r.max():.3f} (tol {tol[int(r.argmax())]:.3e})"
    return tol


def _tail(state, conv2):
    """lin -> dnn + ReLU -> fc on a conv2 output, in the dtype of `state`."""
    h = F.linear(conv2.flatten(1), state["lin.weight"], state["lin.bias"])
    d = F.relu(F.linear(h, state["dnn.weight"], state["dnn.bias"]))
    return F.linear(d, state["fc.weight"], state["fc.bias"])


def _f64(state):
    return {k: v.double() for k, v in state.items()}


_stage_cache = {}


def _stage_case(kind):
    """Weights, 21 clips (clip 0 all-zero) and their float64 / float32 CPU stages, computed once per weight kind."""
    if kind not in _stage_cache:
        state = _state(kind)
        x = torch.randn(21, 1, 99, 10, generator=torch.Generator().manual_seed(8)) * 3.0
        x[0] = 0.0
        lg64, st64 = o_ct.forward(_f64(state), x.double(), return_layers=True)
        lg32, st32 = o_ct.forward(state, x, return_layers=True)
        _stage_cache[kind] = (state, x, lg64, st64["conv2"], lg32, st32["conv2"])
    return _stage_cache[kind]


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("kind", ["random", "default"])
def test_conv2_and_dense_tail_match_float64(ctx, kind, math):
    """a. The convolution kernel's output against the oracle's conv2, whole and on the subsets where SAME padding (4/5 time rows,
    1/2 frequency columns) and the zero-region reads act: the first 4 and last 5 time rows, frequency column 0, frequency column 2.
    b. The dense kernel alone: lin -> dnn + ReLU -> fc evaluated in float64 (float32 for e_f32) on the GPU's own conv2 against the
    GPU logits, so that neither kernel's error hides behind the other's.  The end-to-end logits are checked as well."""
    state, x, lg64, c64, lg32, c32 = _stage_case(kind)
    ctx.load_cnn_trad(o_ct.flatten_state(state), 12)
    logits, _, conv2, _ = _run(ctx, math, x, 12)
    tag = f"{kind} math={math}"
    _check(f"{tag} conv2", conv2, c64, c32)
    rows = lambda t: torch.cat([t[:, :, :4], t[:, :, 94:]], dim=2)
    _check(f"{tag} conv2 time rows 0-3,94-98", rows(conv2), rows(c64), rows(c32))
    for f in (0, 2):
        _check(f"{tag} conv2 frequency column {f}", conv2[..., f], c64[..., f], c32[..., f])
    _check(f"{tag} dense tail on the GPU's conv2", logits, _tail(_f64(state), conv2.double()), _tail(state, conv2))
    _check(f"{tag} logits", logits, lg64, lg32)


def _exp_for(bound) -> int:
    """The kernel's pow2_exp_for, as test_cnntrad_f16_pair_sim._exp_for states it: k with bound * 2^k < 2^15, clamped to +-100."""
    if not bound > 0.0:
        return 100
    return int(np.clip(15 - int(np.frexp(np.float32(bound))[1]), -100, 100))


@pytest.mark.parametrize("kind", ["random", "default"])
def test_clip_scale_is_the_power_of_two_of_the_bound(ctx, kind):
    """c. (f16 pair only) Every clip's scale is an exact power of two, keeps the clip's conv2 below 2^15, and is 2^k2 with k2 from
    bound2 = (w2_abs * bound1 + b2_max) * 1.001, bound1 = (w1_abs * m0 + b1_max) * 1.001, evaluated in float32 like the kernel."""
    state = _state(kind)
    blob = o_ct.flatten_state(state)
    ctx.load_cnn_trad(blob, 12)
    g = torch.Generator().manual_seed(5)
    f = torch.randn(1, 99, 10, generator=g) * 3.0
    x = torch.stack([torch.zeros(1, 99, 10), f * 1e-3, f * 1e3, torch.randn(1, 99, 10, generator=g) * 0.01])
    x[3, 0, 40, 3] = 5000.0
    _, _, conv2, scale = _run(ctx, PAIR, x, 12)
    _, sc = _native.host_cnn_trad_image(blob, 12)  # 1/sw of conv1, conv2, lin; w1_abs, b1_max, w2_abs, b2_max
    w1_abs, b1_max, w2_abs, b2_max = (np.float32(v) for v in sc[3:7])
    for b in range(x.shape[0]):
        s = float(scale[b])
        mant, _ = np.frexp(s)
        assert mant == 0.5, (b, s)
        peak = float(conv2[b].abs().max())
        assert peak * s < 2.0 ** 15, (b, peak, s)
        m0 = np.float32(x[b].abs().max())
        bound1 = np.float32(np.float32(np.float32(w1_abs * m0) + b1_max) * np.float32(1.001))
        bound2 = np.float32(np.float32(np.float32(w2_abs * bound1) + b2_max) * np.float32(1.001))
        assert peak <= float(bound2), (b, peak, bound2)
        assert s == 2.0 ** _exp_for(bound2), (b, s, bound2)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("kind,C", [("random", 1), ("default", 2), ("random", 35), ("default", 64)])
def test_class_counts(ctx, kind, C, math):
    """d. The dense kernel's fc and argmax loops depend on C (i < 16 C, s = i / C): logits against float64 under the rule, labels
    equal to the float64 argmax wherever its top-2 margin exceeds twice the tolerance, label 0 everywhere for C = 1, and the same
    logits bits when no labels are asked for."""
    state = _state(kind, C, seed=2)
    x = torch.randn(5, 1, 99, 10, generator=torch.Generator().manual_seed(40 + C)) * 3.0
    ctx.load_cnn_trad(o_ct.flatten_state(state), C)
    logits, label, _, _ = _run(ctx, math, x, C)
    ref64 = o_ct.forward(_f64(state), x.double())
    tol = _check(f"{kind} C={C} math={math} logits", logits, ref64, o_ct.forward(state, x))
    if C == 1:
        assert bool((label == 0).all())
    else:
        top2 = torch.topk(ref64, 2, dim=1).values
        clear = ((top2[:, 0] - top2[:, 1]).numpy() > 2.0 * tol)
        assert np.array_equal(label.numpy()[clear], ref64.argmax(1).numpy()[clear])
    nolabel, none, _, _ = _run(ctx, math, x, C, want_label=False)
    assert none is None and torch.equal(nolabel, logits)


@pytest.mark.parametrize("math", MATHS)
def test_argmax_ties_first_maximum_wins(ctx, math):
    """e. Two identical fc rows lo < hi that win every clip: bit-identical logits and the label is lo, never hi.  Then fc.weight = 0
    with a constant bias: all logits equal, label 0."""
    lo, hi, B = 3, 7, 17
    state = _state("random", seed=6)
    state["fc.weight"][hi] = state["fc.weight"][lo]
    state["fc.bias"][lo] = state["fc.bias"][hi] = 50.0  # far above any other logit of these fan-in scaled weights
    x = torch.randn(B, 1, 99, 10, generator=torch.Generator().manual_seed(17)) * 3.0
    ctx.load_cnn_trad(o_ct.flatten_state(state), 12)
    logits, label, _, _ = _run(ctx, math, x, 12)
    assert torch.equal(logits[:, lo], logits[:, hi])
    assert bool((logits.argmax(1) == lo).all()), "the tied pair was meant to win every clip"
    assert not bool((label == hi).any())
    assert bool((label == lo).all())
    state["fc.weight"].zero_()
    state["fc.bias"].fill_(0.25)
    ctx.load_cnn_trad(o_ct.flatten_state(state), 12)
    logits, label, _, _ = _run(ctx, math, x, 12)
    assert bool((logits == 0.25).all())
    assert bool((label == 0).all())


@pytest.mark.parametrize("math", MATHS)
def test_batch_slot_invariance(ctx, math):
    """f. A clip's conv2, scale, logits and label do not depend on its slot: the dense kernel packs 16 clips per workgroup into
    MFMA rows and pads a ragged tail by repeating clip B - 1, and each row depends only on its own clip and scale.  Slices of a
    33-clip pool run as their own batches give the pool's bits; so does the pool again after kws_dsblock_forward_f32 has used the
    workspace the two kernels share."""
    state = _state("random", seed=9)
    g = torch.Generator().manual_seed(33)
    level = torch.tensor([0.1, 1.0, 10.0, 100.0]).repeat(9)[:33].reshape(33, 1, 1, 1)
    x = torch.randn(33, 1, 99, 10, generator=g) * level
    x[7] = 0.0
    x[20] *= 1e3
    ctx.load_cnn_trad(o_ct.flatten_state(state), 12)
    base = _run(ctx, math, x, 12)
    assert len(set(base[1].tolist())) > 1, "the pool must not get one label throughout"
    for a, b in ((0, 1), (0, 15), (0, 16), (0, 17), (5, 22), (16, 33)):
        got = _run(ctx, math, x[a:b], 12)
        for name, t, w in zip(("logits", "label", "conv2", "scale"), got, base):
            assert torch.equal(t, w[a:b]), f"slice [{a}:{b}] {name} differs from the whole batch"
    # 3 -> 5 channels, 3 x 3, stride 1, no padding on a 4 x 4 map: a shape test_standalone_block_forward covers
    blk = [torch.randn(s, generator=g).to(DEV) for s in ((1, 3, 4, 4), (3, 1, 3, 3), (3,), (5, 3, 1, 1), (5,))]
    out = torch.full((1, 5, 2, 2), float("nan"), device=DEV)
    ctx.dsblock_forward_f32(*blk, 3, 1, 0, out)
    ctx.sync()
    assert torch.isfinite(out).all()
    again = _run(ctx, math, x, 12)
    for name, t, w in zip(("logits", "label", "conv2", "scale"), again, base):
        assert torch.equal(t, w), f"{name} changed after the workspace was used by kws_dsblock_forward_f32"


def _sparse_int(g, shape, density, amp=1):
    mask = torch.rand(shape, generator=g) < density
    mag = torch.randint(1, amp + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mask * mag * sign).double()


def _integer_network():
    """Sparse integer weights, integer biases, integer features in [-3, 3]; clip 0 is zero but for its four corners, clip 1 is
    non-zero only in frequency column 9, which the pool drops.  Returns (float64 state, x, logits, conv2), after asserting that
    every intermediate stays below 2^22 when evaluated with |w| and |x| -- a bound on every partial sum in any order."""
    g = torch.Generator().manual_seed(7)
    state = {"conv1.weight": _sparse_int(g, (64, 1, 20, 8), 0.3, 2), "conv1.bias": _sparse_int(g, (64,), 1.0, 3),
             "conv2.weight": _sparse_int(g, (64, 64, 10, 4), 0.05), "conv2.bias": _sparse_int(g, (64,), 1.0, 50),
             "lin.weight": _sparse_int(g, (32, o_ct.FLAT), 0.002), "lin.bias": _sparse_int(g, (32,), 1.0, 100),
             "dnn.weight": _sparse_int(g, (128, 32), 0.04), "dnn.bias": _sparse_int(g, (128,), 1.0, 100),
             "fc.weight": _sparse_int(g, (12, 128), 0.02), "fc.bias": _sparse_int(g, (12,), 1.0, 100)}
    x = torch.randint(-3, 4, (6, 1, 99, 10), generator=g).double()
    x[0] = 0.0
    x[0, 0, 0, 0], x[0, 0, 0, 9], x[0, 0, 98, 0], x[0, 0, 98, 9] = 3.0, -2.0, 1.0, 3.0
    col9 = x[1, 0, :, 9].clone()
    x[1] = 0.0
    x[1, 0, :, 9] = col9
    assert float(col9.abs().max()) > 0
    bound_lg, bound = o_ct.forward({k: v.abs() for k, v in state.items()}, x.abs(), return_layers=True)
    for k, v in list(bound.items()) + [("logits", bound_lg)]:
        assert float(v.max()) < 2.0 ** 22, f"{k}: |w|,|x| evaluation reaches {float(v.max()):.0f}"
    logits, layers = o_ct.forward(state, x, return_layers=True)
    for k, v in layers.items():
        assert float(v.abs().max()) > 0, f"{k} is identically zero: the network checks nothing behind it"
    assert float(logits.abs().max()) > 0
    return state, x, logits, layers["conv2"]


@pytest.mark.parametrize("math", MATHS)
def test_integer_network_is_exact(ctx, math):
    """g. An input with an exactly known answer.  All values are integers and, by _integer_network's assertion, every partial sum
    of every stage is an integer below 2^22 in magnitude whatever the summation order.  An f16 pair holds 22 significant bits
    after its exact power-of-two scaling and f16 x f16 products accumulate exactly in f32 below 2^24; the bf16 triple holds all
    24 bits of an f32 and the three piece products it drops pair two non-leading pieces, one of which belongs to a weight in
    {-2..2} and is zero.  So both arithmetics must return conv2 and logits EQUAL to the float64 reference: any difference is a
    whole integer (an indexing error: a wrong tap, border, lane or clip) or a rounding step this argument missed.  On the CPU
    the NumPy model of the pair arithmetic (test_cnntrad_f16_pair_sim._forward_pair) returns these logits exactly; the equality
    had not been observed on a GPU when this test was written."""
    state, x, want, want_c2 = _integer_network()
    ctx.load_cnn_trad(o_ct.flatten_state(state), 12)
    logits, label, conv2, _ = _run(ctx, math, x.float(), 12)
    d2 = (conv2.double() - want_c2).abs()
    dl = (logits.double() - want).abs()
    print(f"integer network math={math}: max|conv2 - ref| = {float(d2.max())}, max|logits - ref| = {float(dl.max())}")
    assert float(d2.max()) == 0.0, f"conv2 differs at {int((d2 > 0).sum())} of {d2.numel()} values, by up to {float(d2.max())}"
    assert float(dl.max()) == 0.0, f"logits differ by up to {float(dl.max())}"
    assert torch.equal(label.long(), want.argmax(1))  # torch's argmax returns the first maximum on the CPU


def test_errors():
    """h. KWS_ESTATE with no model loaded, KWS_EINVAL for B <= 0 and NULL d_feat / d_logits (and NULL d_conv2 for the debug
    entry), from both entries; KWS_EUNSUPPORTED from kws_infer_cnn_trad_i16 when the front end's map is not 99 x 10."""
    c = _native.Context(0)
    try:
        lib, h = c._lib, c._h
        x = torch.zeros(2, 1, 99, 10, device=DEV)
        lg = torch.zeros(2, 12, device=DEV)
        lb = torch.zeros(2, dtype=torch.int32, device=DEV)
        c2 = torch.zeros(2, 64, 99, 3, device=DEV)
        sc = torch.zeros(2, device=DEV)
        xp, lgp, lbp, c2p, scp = (t.data_ptr() for t in (x, lg, lb, c2, sc))
        assert lib.kws_forward_cnn_trad_f32(h, xp, 2, lgp, lbp) == _native.KWS_ESTATE
        assert lib.kws_forward_cnn_trad_debug_f32(h, xp, 2, lgp, lbp, c2p, scp) == _native.KWS_ESTATE
        c.load_cnn_trad(o_ct.flatten_state(_state("random")), 12)
        for B in (0, -1):
            assert lib.kws_forward_cnn_trad_f32(h, xp, B, lgp, lbp) == _native.KWS_EINVAL
            assert lib.kws_forward_cnn_trad_debug_f32(h, xp, B, lgp, lbp, c2p, scp) == _native.KWS_EINVAL
        assert lib.kws_forward_cnn_trad_f32(h, None, 2, lgp, lbp) == _native.KWS_EINVAL
        assert lib.kws_forward_cnn_trad_f32(h, xp, 2, None, lbp) == _native.KWS_EINVAL
        assert lib.kws_forward_cnn_trad_debug_f32(h, None, 2, lgp, lbp, c2p, scp) == _native.KWS_EINVAL
        assert lib.kws_forward_cnn_trad_debug_f32(h, xp, 2, None, lbp, c2p, scp) == _native.KWS_EINVAL
        assert lib.kws_forward_cnn_trad_debug_f32(h, xp, 2, lgp, lbp, None, scp) == _native.KWS_EINVAL
        assert lib.kws_forward_cnn_trad_debug_f32(h, xp, 2, lgp, None, c2p, None) == _native.KWS_OK  # both optional outputs absent
        c.sync()
        c.set_frontend(numcep=13)
        wav = torch.zeros(2, 16000, dtype=torch.int16, device=DEV)
        assert lib.kws_infer_cnn_trad_i16(h, wav.data_ptr(), 2, lgp, lbp) == _native.KWS_EUNSUPPORTED
    finally:
        c.close()
