"""The persistent DS-CNN kernels run their block phases under a per-block wavefront-priority schedule (s_setprio at unit
boundaries, csrc/kws_dscnn_stages.h "Wavefront priority").  Priority moves issue slots between the two wavefronts of a SIMD and
nothing else, so every result must be the same bits as before -- unless the new timing exposes an ordering that only the old
timing hid.  The places where wavefronts meet without a barrier are the staging of the next clip into the Z2 plane in block 4's
tail and the arrival counter of the K-split leftover tiles of blocks 1 and 2; a race there shows as a launch that differs from
its repeat, or as a clip that differs from the same map run alone on the one-clip kernel (which holds no s_setprio).

Feature maps: the 56 golden maps (8 random + the oracle MFCC of 48 diverse clips), golden weights, both product arithmetics.
Batch sizes: 3 (one-clip kernel), CU count + 1 (one workgroup carries two clips, the others one) and 3 * CU count + 2 (workgroups
0 and 1 carry four clips, the others three: a first, middle and last clip of a workgroup)."""
import numpy as np
import pytest
import torch

from oracle import psf_mfcc as o_mfcc
from test_gpu_parity import LAYER_RTOL, TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
MATHS = pytest.mark.parametrize("math", [4, 5], ids=["bf16_triple", "f16_pair"])
SIZES = pytest.mark.parametrize("size", ["3", "n_cu+1", "3n_cu+2"])
PLANES = {"conv1": (0, 141), "dsconv1": (141, 141), "dsconv2": (282, 245), "dsconv3": (527, 357)}  # (first position, positions) in the dump


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def batch_size(size):
    return {"3": 3, "n_cu+1": _n_cu() + 1, "3n_cu+2": 3 * _n_cu() + 2}[size]


@pytest.fixture(scope="module")
def native():
    from kws import _native

    return _native


@pytest.fixture(scope="module")
def ctx(native, e2e_golden):
    c = native.Context(0)
    c.use_torch_stream()
    c.load_dscnn(e2e_golden["he.blob"], C)
    yield c
    c.set_pointwise_math(native.PW_DEFAULT)
    c.close()


@pytest.fixture(scope="module")
def pool(e2e_golden):
    """The golden maps with the reference model's logits and labels."""
    g = e2e_golden
    x = np.concatenate([g["x_rand"], o_mfcc.collate_pcm16(g["clips"])]).astype(np.float32)
    return {"dev": torch.from_numpy(x).to(DEV), "n": len(x), "logits": g["he.logits"], "label": g["he.label"]}


def batch_of(pool, B, shift=0):
    idx = (3 * np.arange(B) + shift) % pool["n"]  # neighbours differ; 3 and 56 are coprime: every map is used
    return idx, pool["dev"][torch.from_numpy(idx).to(DEV)].contiguous()


def run_product(ctx, feat, math):
    ctx.set_pointwise_math(math)
    B = feat.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ctx.forward_f32(feat, logits, labels)
    torch.cuda.synchronize()
    return logits, labels


def run_debug(ctx, native, feat, math):
    """(logits, labels, {layer: [B, 64, positions]}) of the diagnostics entry."""
    B = feat.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    act = torch.zeros((B, native.ACT_FLOATS_PER_CLIP), dtype=torch.float32, device=DEV)
    ctx.forward_debug_f32(feat, logits, labels, act, use_mfma=math)
    torch.cuda.synchronize()
    return logits, labels, {k: act[:, 64 * p0:64 * (p0 + n)].reshape(B, 64, n) for k, (p0, n) in PLANES.items()}


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_alone = {}


def alone(ctx, pool, math):
    """Every golden map run alone (B = 1: the one-clip kernel), once per arithmetic: ([56, C] logits, [56] labels)."""
    if math not in _alone:
        outs = [run_product(ctx, pool["dev"][k:k + 1].contiguous(), math) for k in range(pool["n"])]
        _alone[math] = (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]))
    return _alone[math]


@MATHS
@SIZES
def test_ten_launches_give_the_same_bits(ctx, pool, math, size):
    _, feat = batch_of(pool, batch_size(size), shift=1)
    first = run_product(ctx, feat, math)
    assert torch.isfinite(first[0]).all() and int(first[1].min()) >= 0
    for rep in range(9):
        again = run_product(ctx, feat, math)
        assert bits_equal(first[0], again[0]) and torch.equal(first[1], again[1]), f"launch {rep + 2} differs from the first"


@MATHS
@SIZES
def test_every_clip_equals_the_same_map_alone(ctx, pool, math, size):
    want_logits, want_labels = alone(ctx, pool, math)
    idx, feat = batch_of(pool, batch_size(size), shift=2)
    logits, labels = run_product(ctx, feat, math)
    sel = torch.from_numpy(idx).to(DEV)
    differ = (logits.view(torch.int32) != want_logits[sel].view(torch.int32)).any(dim=1) | (labels != want_labels[sel])
    assert not bool(differ.any()), f"clips {torch.nonzero(differ).flatten()[:8].tolist()} differ from their maps run alone"


@MATHS
def test_plane_dump_equals_the_one_clip_kernels(ctx, native, pool, math):
    """A map at index 0 (a workgroup's first clip) and at index CU count (its second, staged in the first one's block-4 tail, its
    conv1 windows and Z1 / Z2 planes written where the first clip's lay): every dumped plane as from the one-clip kernel."""
    n_cu = _n_cu()
    for k in (0, pool["n"] - 1):
        one = pool["dev"][k:k + 1].contiguous()
        _, feat = batch_of(pool, n_cu + 1, shift=4)
        feat[0] = one[0]
        feat[n_cu] = one[0]
        a, b = run_debug(ctx, native, one, math), run_debug(ctx, native, feat, math)
        assert torch.isfinite(a[0]).all()
        for at in (0, n_cu):
            for name in PLANES:
                assert bits_equal(a[2][name][0], b[2][name][at]), f"map {k} at index {at}: plane {name} differs from the one-clip kernel's"
            assert bits_equal(a[0][0], b[0][at]) and int(a[1][0]) == int(b[1][at]), (k, at)


@MATHS
@SIZES
def test_golden_logits(ctx, pool, math, size):
    """The logits gate of test_gpu_parity.test_dscnn_layers_and_logits, and the reference's labels."""
    idx, feat = batch_of(pool, batch_size(size), shift=5)
    logits, labels = run_product(ctx, feat, math)
    ref = pool["logits"][idx]
    err = float(np.abs(logits.cpu().numpy() - ref).max())
    gate = min(TOL, LAYER_RTOL * max(float(np.abs(pool["logits"]).max()), 1e-30) * 4)
    print(f"B={feat.shape[0]} math={math}: logits err {err:.3e}, gate {gate:.3e}")
    assert err <= gate
    assert np.array_equal(labels.cpu().numpy(), pool["label"][idx])


@MATHS
def test_results_return_after_a_model_switch(ctx, pool, e2e_golden, math):
    sizes = [batch_size(s) for s in ("3", "n_cu+1", "3n_cu+2")]
    try:
        before = [run_product(ctx, batch_of(pool, B, shift=3)[1], math) for B in sizes]
        ctx.load_dscnn(e2e_golden["tie_all.blob"], C)
        other = [run_product(ctx, batch_of(pool, B, shift=3)[1], math) for B in sizes]
        ctx.load_dscnn(e2e_golden["he.blob"], C)
        after = [run_product(ctx, batch_of(pool, B, shift=3)[1], math) for B in sizes]
    finally:
        ctx.load_dscnn(e2e_golden["he.blob"], C)
    for B, b, o, a in zip(sizes, before, other, after):
        assert not bits_equal(b[0], o[0]), f"B={B}: the second model gave the first one's logits"
        assert bits_equal(b[0], a[0]) and torch.equal(b[1], a[1]), f"B={B}: results changed across the model switch"
