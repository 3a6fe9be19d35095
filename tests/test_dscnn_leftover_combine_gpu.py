"""The K-split leftover tiles of DS-CNN blocks 1 and 2 (the fifth tile of block 1, positions 120..140; the ninth of block 2,
positions 240..244) are combined by whichever of their four quarter wavefronts stores its partial sums last (leftover_arrive,
csrc/kws_dscnn_stages.h: an arrival counter in LDS, nobody waits).  Which wavefront that is changes from launch to launch, so:
the results must not depend on it, the counter must be clean for a workgroup's next clip, the combined positions must be the
oracle's, and (f16 pairs) the combine's maximum must reach the scale of the block after the next.

12 classes, the golden signal-preserving weights, both product arithmetics, the one-clip kernel (3 clips) and the persistent
kernel (CU count + 1 clips: workgroup 0 carries two).

Two inputs carry a maximum through the combine.  The loud-burst clip (silence but for a burst in its last 100 ms): its largest
block-1 output lies in the leftover tile.  Block 2's leftover tile is the last row of its 49 x 5 plane, which sees one row of
block 1 and the relu(bias) ring, and with the golden weights no burst reaches the plane's maximum there (400 PCM bursts: at most
0.70 of it), so a second input, tests/golden/dscnn_leftover_max_map.npy (found on the oracle by make_leftover_max_map.py), has
the largest output of block 1 AND of block 2 in the leftover tiles, each more than twice the rest of its plane.  Both
properties are asserted on the oracle before the inputs are used."""
import os

import numpy as np
import pytest
import torch

from oracle import dscnn as o_dscnn
from oracle import psf_mfcc as o_mfcc
from test_gpu_parity import LAYER_RTOL, TOL, split_act, state_from_blob

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
LAUNCHES = 10
L1 = slice(120, 141)  # block 1's leftover tile
L2 = slice(240, 245)  # block 2's
MATHS = pytest.mark.parametrize("math", [4, 5], ids=["bf16_triple", "f16_pair"])


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


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


def burst_clip():
    """Digital silence but for a loud 700 Hz square wave in the last 100 ms."""
    clip = np.zeros((1, 16000), np.int16)
    n = 16000 - 14400
    clip[0, 14400:] = (30000 * np.sign(np.sin(2 * np.pi * 700 * np.arange(n) / 16000))).astype(np.int16)
    return clip


@pytest.fixture(scope="module")
def pool(e2e_golden):
    """Distinct feature maps (random maps, the MFCC of diverse clips, the searched map last but one, the burst clip last) and the
    oracle's layers for them, computed once."""
    g = e2e_golden
    searched = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dscnn_leftover_max_map.npy"))
    x = np.concatenate([g["x_rand"], o_mfcc.collate_pcm16(g["clips"][:14]), searched, o_mfcc.collate_pcm16(burst_clip())]).astype(np.float32)
    assert len(x) % 5 != 0  # (batch_of strides by 5)
    state = state_from_blob(g["he.blob"])
    logits, layers = o_dscnn.forward(state, torch.from_numpy(x), return_layers=True)
    z1 = layers["dsconv1"].numpy()[:, :, 1:-1, 1:-1].reshape(len(x), 64, -1)
    z2 = layers["dsconv2"].numpy()[:, :, 1:-1, 1:-1].reshape(len(x), 64, -1)
    ref64 = o_dscnn.forward({k: v.double() for k, v in state.items()}, torch.from_numpy(x).double()).numpy()
    return {"x": torch.from_numpy(x).to(DEV), "logits": logits.numpy(), "ref64": ref64, "z1": z1, "z2": z2, "n": len(x)}


def batch_of(pool, B, shift=0):
    idx = (5 * np.arange(B) + shift) % pool["n"]  # neighbours differ, every map moves around
    return idx, pool["x"][torch.from_numpy(idx).to(DEV)].contiguous()


def run_product(ctx, feat, math):
    ctx.set_pointwise_math(math)
    B = feat.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ctx.forward_f32(feat, logits, labels)
    torch.cuda.synchronize()
    return logits, labels


def run_debug(ctx, native, feat, math):
    """(logits, labels, Z1 [B, 64, 141], Z2 [B, 64, 245]) of the diagnostics entry, on the device."""
    B = feat.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    act = torch.zeros((B, native.ACT_FLOATS_PER_CLIP), dtype=torch.float32, device=DEV)
    ctx.forward_debug_f32(feat, logits, labels, act, use_mfma=math)
    torch.cuda.synchronize()
    z1 = act[:, 64 * 141:64 * 282].reshape(B, 64, 141).clone()
    z2 = act[:, 64 * 282:64 * (282 + 245)].reshape(B, 64, 245).clone()
    return logits, labels, z1, z2


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_plane_offsets_are_split_acts():
    """run_debug slices the dump the way test_gpu_parity.split_act does."""
    act = np.arange(2 * (64 * (141 + 141 + 245 + 357) + 64 + 64 * 477), dtype=np.float32).reshape(2, -1)
    s = split_act(act)
    assert np.array_equal(s["dsconv1"], act[:, 64 * 141:64 * 282].reshape(2, 64, 141))
    assert np.array_equal(s["dsconv2"], act[:, 64 * 282:64 * (282 + 245)].reshape(2, 64, 245))


@MATHS
@pytest.mark.parametrize("kernel", ["persistent", "one_clip"])
def test_who_arrives_last_does_not_matter(ctx, native, pool, math, kernel):
    B = _n_cu() + 1 if kernel == "persistent" else 3
    _, feat = batch_of(pool, B, shift=2)
    first = run_debug(ctx, native, feat, math)
    assert torch.isfinite(first[0]).all()
    first_p = run_product(ctx, feat, math)
    assert bits_equal(first_p[0], first[0]) and torch.equal(first_p[1], first[1]), "product and diagnostics instantiations differ"
    for n in range(1, LAUNCHES):
        got = run_debug(ctx, native, feat, math)
        for name, a, b in zip(("logits", "labels", "Z1", "Z2"), first, got):
            assert bits_equal(a, b), f"launch {n}: {name} differs from the first launch"
        got_p = run_product(ctx, feat, math)
        assert bits_equal(first_p[0], got_p[0]) and torch.equal(first_p[1], got_p[1]), f"product launch {n} differs from the first"


@MATHS
def test_position_in_the_batch_does_not_matter(ctx, native, pool, math):
    """The same map as a workgroup's first clip, as its second (index n_cu: behind another clip's combines) and alone."""
    n_cu = _n_cu()
    for k in (0, pool["n"] - 2, pool["n"] - 1):  # a random map, the searched map, the burst clip
        one = pool["x"][k:k + 1].contiguous()
        _, feat = batch_of(pool, n_cu + 1, shift=1)
        feat[0] = one[0]
        feat[n_cu] = one[0]
        alone = run_debug(ctx, native, one, math)
        both = run_debug(ctx, native, feat, math)
        alone_p, both_p = run_product(ctx, one, math), run_product(ctx, feat, math)
        for at in (0, n_cu):
            for name, a, b in zip(("logits", "labels", "Z1", "Z2"), alone, both):
                assert bits_equal(a[0], b[at]), f"map {k} at index {at}: {name} differs from the map alone"
            assert bits_equal(alone_p[0][0], both_p[0][at]) and int(alone_p[1][0]) == int(both_p[1][at]), (k, at)
        assert bits_equal(alone_p[0], alone[0])


@MATHS
@pytest.mark.parametrize("kernel", ["persistent", "one_clip"])
def test_leftover_positions_match_the_oracle(ctx, native, pool, math, kernel):
    B = _n_cu() + 1 if kernel == "persistent" else 3
    idx, feat = batch_of(pool, B, shift=pool["n"] - 1)  # (index 0 is the burst clip)
    _, _, z1, z2 = run_debug(ctx, native, feat, math)
    for name, got, want, where in (("dsconv1", z1.cpu().numpy(), pool["z1"][idx], L1), ("dsconv2", z2.cpu().numpy(), pool["z2"][idx], L2)):
        scale = float(np.abs(want).max())  # the per-layer gate of test_gpu_parity: LAYER_RTOL of the layer's largest activation
        err = float(np.abs(got[:, :, where] - want[:, :, where]).max())
        print(f"{name} leftover positions: max abs err {err:.3e}, gate {LAYER_RTOL * scale:.3e}")
        assert err <= LAYER_RTOL * scale, f"{name} positions {where.start}..{where.stop - 1}: max abs err {err:.3e} (scale {scale:.3e})"
        err_all = float(np.abs(got - want).max())
        assert err_all <= LAYER_RTOL * scale, f"{name}: max abs err {err_all:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("which", ["burst_clip", "searched_map"])
def test_the_combines_maximum_reaches_the_scale(ctx, native, pool, which):
    """The largest stored output of a block lies in its leftover tile, by more than a factor of two over the rest of the plane:
    were the combine's maximum not folded into the stage maximum, the measured bound -- and with it the power-of-two scale of
    the block after the next -- would come out lower.  The burst clip has this for block 1, the searched map for blocks 1 and 2."""
    k = pool["n"] - 1 if which == "burst_clip" else pool["n"] - 2
    z1, z2 = pool["z1"][k], pool["z2"][k]
    p1 = int(np.unravel_index(z1.argmax(), z1.shape)[1])
    p2 = int(np.unravel_index(z2.argmax(), z2.shape)[1])
    r1 = float(z1[:, L1].max() / z1[:, :120].max())
    r2 = float(z2[:, L2].max() / z2[:, :240].max())
    print(f"{which}: maxima at positions {p1} (block 1), {p2} (block 2); leftover maximum / rest of the plane = {r1:.3f}, {r2:.3f}")
    assert p1 >= 120 and r1 > 2.0, "choose another input: block 1's largest output must lie in its leftover tile"
    if which == "searched_map":
        assert p2 >= 240 and r2 > 2.0, "choose another input: block 2's largest output must lie in its leftover tile"
    n_cu = _n_cu()
    one = pool["x"][k:k + 1].contiguous()
    _, many = batch_of(pool, n_cu + 1, shift=1)
    many[n_cu] = one[0]
    out = {}
    for math in (native.PW_PAIR_F16, native.PW_SPLIT_BF16):
        a, _ = run_product(ctx, one, math)
        b, _ = run_product(ctx, many, math)
        assert bits_equal(a[0], b[n_cu])
        out[math] = a[0].cpu().double().numpy()
    pair, triple = out[native.PW_PAIR_F16], out[native.PW_SPLIT_BF16]
    assert np.isfinite(pair).all() and np.isfinite(triple).all()
    scale = max(1.0, float(np.abs(pool["ref64"][k]).max()))
    e_mut = float(np.abs(pair - triple).max())
    e_or = max(float(np.abs(pair - pool["logits"][k]).max()), float(np.abs(triple - pool["logits"][k]).max()))
    # the logits gate of test_gpu_parity.test_dscnn_layers_and_logits, with this input's own reference logits
    gate_or = min(TOL, LAYER_RTOL * max(float(np.abs(pool["logits"][k]).max()), 1e-30) * 4)
    print(f"{which}: |pair - triple| = {e_mut:.3e} (gate {3e-6 * scale:.3e}), |gpu - oracle| = {e_or:.3e} (gate {gate_or:.3e})")
    assert e_mut <= 3e-6 * scale  # the f16-pair gate of test_dscnn_f16_pair_arithmetic_holds_over_range
    assert e_or <= gate_or


@MATHS
def test_one_pass_after_switching_model_and_back(ctx, pool, dscnn_golden, e2e_golden, math):
    _, feat = batch_of(pool, _n_cu() + 1, shift=4)
    first = run_product(ctx, feat, math)
    try:
        ctx.load_dscnn(dscnn_golden["n01.blob"], C)
        other = run_product(ctx, feat, math)
        assert torch.isfinite(other[0]).all() and not bits_equal(other[0], first[0])
    finally:
        ctx.load_dscnn(e2e_golden["he.blob"], C)
    again = run_product(ctx, feat, math)
    assert bits_equal(first[0], again[0]) and torch.equal(first[1], again[1])
