"""The depthwise weights of the DS-CNN block phases reach the stencil by row broadcast: lane l of a 16-lane row reads the one
(channel c, channel c + 1) pair at 8 * (l & 15) bytes into the pair's 96-byte record and every tap is taken from its lane of
the row (stencil3x3_row, csrc/kws_dscnn_stages.h).  What can go wrong is a tap, a channel of the pair, a record or a table
buffer taken for another, so the weights here make each of them show as a wrong plane, not as a small error:

* one-hot taps: in one block, tap t of every channel c is v(c) (distinct per channel, some negative), every other tap and the
  bias are 0 and the pointwise layer is the identity: the block's output is relu(v(c) * input plane shifted by the tap);
* bias only: all taps 0, bias c + 1;
* the channels at the edges of the lane mapping (0, 7, 8, 15, 16, 31, 32, 62, 63: first / last of a half-wave's eight, of a
  k-block, of the two tap-address bases; 62 / 63 own the last record, whose row read runs past it), each with its own tap.

Blocks 1 and 2 carry the patterns: they read table buffer 0 and buffer 1, and both have a K-split leftover tile (positions
120..140 and 240..244), so the full units, the leftover quarters and both buffers are covered.  Every case runs at B = 3 (the
one-clip kernel) and B = CU count + 1 (the persistent kernel, workgroup 0 carries two clips), on both product arithmetics,
against oracle/dscnn.py at the per-layer gate of tests/test_gpu_parity.py, through the diagnostics dump."""
import numpy as np
import pytest
import torch

from oracle import dscnn as o_dscnn
from oracle import psf_mfcc as o_mfcc
from test_gpu_parity import LAYER_RTOL, TOL, split_act, state_from_blob

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
MATHS = pytest.mark.parametrize("math", [4, 5], ids=["bf16_triple", "f16_pair"])
BLOCKS = pytest.mark.parametrize("block", [1, 2], ids=["block1_buffer0", "block2_buffer1"])
EDGE_CHANNELS = [0, 7, 8, 15, 16, 31, 32, 62, 63]
PLANES = {"conv1": (0, 141), "dsconv1": (141, 141), "dsconv2": (282, 245), "dsconv3": (527, 357)}  # (first position, positions) in the dump


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def v_of(c):
    """The value channel c carries: distinct per channel, every fifth negative (its plane is then all ReLU)."""
    return (1.0 + c / 64.0) * (-1.0 if c % 5 == 4 else 1.0)


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
def maps(e2e_golden):
    """Seven distinct feature maps: random maps and the oracle MFCC of diverse clips."""
    g = e2e_golden
    x = np.concatenate([g["x_rand"][:3], o_mfcc.collate_pcm16(g["clips"][:4])]).astype(np.float32)
    return {"cpu": torch.from_numpy(x), "dev": torch.from_numpy(x).to(DEV), "n": len(x)}


def patterned_state(golden_state, block, dw_weight, dw_bias):
    """The golden model with `block`'s depthwise layer replaced and its pointwise layer the identity (bias 0)."""
    st = {k: v.clone() for k, v in golden_state.items()}
    st[f"dsconv{block}.depthwise.weight"] = torch.from_numpy(np.asarray(dw_weight, np.float32).reshape(64, 1, 3, 3))
    st[f"dsconv{block}.depthwise.bias"] = torch.from_numpy(np.asarray(dw_bias, np.float32))
    st[f"dsconv{block}.pointwise.weight"] = torch.eye(64, dtype=torch.float32).reshape(64, 64, 1, 1)
    st[f"dsconv{block}.pointwise.bias"] = torch.zeros(64, dtype=torch.float32)
    return st


def one_hot_weights(tap):
    w = np.zeros((64, 9), np.float32)
    w[:, tap] = [v_of(c) for c in range(64)]
    return w, np.zeros(64, np.float32)


def edge_weights():
    """Channel EDGE_CHANNELS[i] carries tap i alone, with its own value and a bias of its own; every other channel is zero."""
    w, b = np.zeros((64, 9), np.float32), np.zeros(64, np.float32)
    for i, c in enumerate(EDGE_CHANNELS):
        w[c, i] = v_of(c)
        b[c] = 0.125 * (i + 1)
    return w, b


_oracle_cache = {}


def oracle_layers(key, state, maps):
    """(logits, {layer: [n, 64, positions] interior planes}) of the oracle for the seven maps, computed once per model."""
    if key not in _oracle_cache:
        logits, layers = o_dscnn.forward(state, maps["cpu"], return_layers=True)
        planes = {"conv1": layers["conv1"].numpy().reshape(maps["n"], 64, -1)}
        for i in range(1, 4):
            planes[f"dsconv{i}"] = layers[f"dsconv{i}"].numpy()[:, :, 1:-1, 1:-1].reshape(maps["n"], 64, -1)
        full = {"conv1": layers["conv1"].numpy(), "dsconv1": layers["dsconv1"].numpy()}  # a block's input, ring included
        _oracle_cache[key] = (logits.numpy(), planes, full)
    return _oracle_cache[key]


def batch_of(maps, B, shift=0):
    idx = (3 * np.arange(B) + shift) % maps["n"]  # neighbours differ
    return idx, maps["dev"][torch.from_numpy(idx).to(DEV)].contiguous()


def run_debug(ctx, native, feat, math):
    """(logits, labels, {layer: [B, 64, positions]}) of the diagnostics entry, on the device."""
    B = feat.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    act = torch.zeros((B, native.ACT_FLOATS_PER_CLIP), dtype=torch.float32, device=DEV)
    ctx.forward_debug_f32(feat, logits, labels, act, use_mfma=math)
    torch.cuda.synchronize()
    planes = {k: act[:, 64 * p0:64 * (p0 + n)].reshape(B, 64, n) for k, (p0, n) in PLANES.items()}
    return logits, labels, planes


def run_product(ctx, feat, math):
    ctx.set_pointwise_math(math)
    B = feat.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ctx.forward_f32(feat, logits, labels)
    torch.cuda.synchronize()
    return logits, labels


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_block_against_oracle(ctx, native, maps, key, state, block, math, what):
    """Load `state`, run B = 3 and B = CU count + 1 and hold the block's dumped plane (and the planes before it) to the oracle's."""
    ctx.load_dscnn(o_dscnn.flatten_state(state), C)
    ref_logits, ref, _ = oracle_layers(key, state, maps)
    for B in (3, _n_cu() + 1):
        idx, feat = batch_of(maps, B, shift=B % 7)
        logits, _, planes = run_debug(ctx, native, feat, math)
        assert torch.isfinite(logits).all()
        for name in ["conv1"] + [f"dsconv{i}" for i in range(1, block + 1)]:
            want = torch.from_numpy(ref[name]).to(DEV)[torch.from_numpy(idx).to(DEV)]
            scale = float(want.abs().max())
            err = (planes[name] - want).abs()
            worst = int(err.amax(dim=(0, 2)).argmax())
            print(f"{what} B={B} math={math} {name}: max abs err {float(err.max()):.3e} (channel {worst}), gate {LAYER_RTOL * scale:.3e}")
            assert float(err.max()) <= LAYER_RTOL * scale, f"{what} B={B} {name}: max abs err {float(err.max()):.3e} in channel {worst} (scale {scale:.3e})"
    return ref_logits


def test_plane_offsets_are_split_acts():
    act = np.arange(2 * (64 * (141 + 141 + 245 + 357) + 64 + 64 * 477), dtype=np.float32).reshape(2, -1)
    s = split_act(act)
    for k, (p0, n) in PLANES.items():
        assert np.array_equal(s[k], act[:, 64 * p0:64 * (p0 + n)].reshape(2, 64, n))


@MATHS
@BLOCKS
def test_one_hot_taps(ctx, native, maps, e2e_golden, block, math):
    golden = state_from_blob(e2e_golden["he.blob"])
    try:
        for tap in range(9):
            w, b = one_hot_weights(tap)
            state = patterned_state(golden, block, w, b)
            _, ref, full = oracle_layers(("tap", block, tap), state, maps)
            # the oracle's plane is what the pattern says: relu(v(c) * the zero-padded input shifted by the tap), exactly
            x_in = full["conv1" if block == 1 else "dsconv1"]
            H, W = x_in.shape[2], x_in.shape[3]
            xp = np.pad(x_in, ((0, 0), (0, 0), (1, 1), (1, 1)))
            v = np.array([v_of(c) for c in range(64)], np.float32).reshape(1, 64, 1, 1)
            shifted = np.maximum(v * xp[:, :, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W], 0).reshape(maps["n"], 64, -1)
            assert np.array_equal(shifted, ref[f"dsconv{block}"]), f"tap {tap}: the oracle's plane is not the shifted input"
            assert float(shifted.max()) > 0
            check_block_against_oracle(ctx, native, maps, ("tap", block, tap), state, block, math, f"block {block} tap {tap}")
    finally:
        ctx.load_dscnn(e2e_golden["he.blob"], C)


@MATHS
@BLOCKS
def test_bias_only(ctx, native, maps, e2e_golden, block, math):
    golden = state_from_blob(e2e_golden["he.blob"])
    state = patterned_state(golden, block, np.zeros((64, 9), np.float32), np.arange(1, 65, dtype=np.float32))
    try:
        _, ref, _ = oracle_layers(("bias", block), state, maps)
        assert np.array_equal(ref[f"dsconv{block}"], np.broadcast_to(np.arange(1, 65, dtype=np.float32).reshape(1, 64, 1), ref[f"dsconv{block}"].shape))
        check_block_against_oracle(ctx, native, maps, ("bias", block), state, block, math, f"block {block} bias only")
    finally:
        ctx.load_dscnn(e2e_golden["he.blob"], C)


def edge_state(e2e_golden, blocks):
    state = state_from_blob(e2e_golden["he.blob"])
    for block in blocks:
        state = patterned_state(state, block, *edge_weights())
    return state


@MATHS
@BLOCKS
def test_channels_at_the_edges_of_the_lane_mapping(ctx, native, maps, e2e_golden, block, math):
    state = edge_state(e2e_golden, [block])
    try:
        _, ref, _ = oracle_layers(("edge", block), state, maps)
        plane = ref[f"dsconv{block}"]
        others = [c for c in range(64) if c not in EDGE_CHANNELS]
        assert not plane[:, others].any() and all(plane[:, c].any() for c in EDGE_CHANNELS)
        check_block_against_oracle(ctx, native, maps, ("edge", block), state, block, math, f"block {block} edge channels")
    finally:
        ctx.load_dscnn(e2e_golden["he.blob"], C)


@MATHS
def test_one_map_gives_the_same_bits_on_every_route(ctx, native, maps, e2e_golden, math):
    """One map as a workgroup's first clip (index 0), as its second (index CU count) and alone: logits, labels and dumped planes
    equal bit for bit, with the edge patterns in blocks 1 and 2 and with the golden weights."""
    n_cu = _n_cu()
    try:
        for blob in (o_dscnn.flatten_state(edge_state(e2e_golden, [1, 2])), e2e_golden["he.blob"]):
            ctx.load_dscnn(blob, C)
            for k in (0, maps["n"] - 1):
                one = maps["dev"][k:k + 1].contiguous()
                _, feat = batch_of(maps, n_cu + 1, shift=1)
                feat[0] = one[0]
                feat[n_cu] = one[0]
                alone, both = run_debug(ctx, native, one, math), run_debug(ctx, native, feat, math)
                alone_p, both_p = run_product(ctx, one, math), run_product(ctx, feat, math)
                assert torch.isfinite(alone[0]).all()
                for at in (0, n_cu):
                    assert bits_equal(alone[0][0], both[0][at]) and int(alone[1][0]) == int(both[1][at]), (k, at)
                    for name in PLANES:
                        assert bits_equal(alone[2][name][0], both[2][name][at]), f"map {k} at index {at}: {name} differs from the map alone"
                    assert bits_equal(alone_p[0][0], both_p[0][at]) and int(alone_p[1][0]) == int(both_p[1][at]), (k, at)
                assert bits_equal(alone_p[0], alone[0])
    finally:
        ctx.load_dscnn(e2e_golden["he.blob"], C)


@MATHS
def test_golden_weights_logits(ctx, native, maps, e2e_golden, math):
    """The golden weights at the logits gate of test_gpu_parity.test_dscnn_layers_and_logits, on both kernels."""
    ctx.load_dscnn(e2e_golden["he.blob"], C)
    ref_logits, _, _ = oracle_layers("golden", state_from_blob(e2e_golden["he.blob"]), maps)
    gate = min(TOL, LAYER_RTOL * max(float(np.abs(ref_logits).max()), 1e-30) * 4)
    for B in (3, _n_cu() + 1):
        idx, feat = batch_of(maps, B, shift=2)
        logits, labels = run_product(ctx, feat, math)
        err = float(np.abs(logits.cpu().numpy() - ref_logits[idx]).max())
        print(f"B={B} math={math}: logits err {err:.3e}, gate {gate:.3e}")
        assert err <= gate
        top2 = np.sort(ref_logits[idx], axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 2 * gate  # (a margin inside the gate may fall either way)
        assert clear.any() and np.array_equal(labels.cpu().numpy()[clear], ref_logits[idx].argmax(axis=1)[clear])
