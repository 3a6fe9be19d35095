"""The persistent batched DS-CNN forward with f16 pairs reads each block-phase unit's geometry from the unit descriptor table
behind the weight image (csrc/kws_dscnn_units.h) instead of computing it, and both arithmetics read the weight argument again
in every phase.  One clip alone (B = 1) runs the one-clip kernel, which computes its geometry and holds one copy of the weights:
every clip of a persistent launch must give the same logits and label bit for bit.  B = n_cu + 1 is the smallest
persistent launch (one workgroup carries two clips), B = 2 n_cu + 3 has workgroups with two and with three clips.  The table is
written by every load, host or device: after a second model and back, the results follow the model loaded.

The clip pool is the one of tests/test_dscnn_persistent_gpu.py (ordinary, x 3e4, all-zero, x 1e-20, one spike)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
C = 12
POOL = 13


@pytest.fixture(scope="module")
def blob():
    sys.path.insert(0, ROOT)
    import bench

    return np.ascontiguousarray(bench.bench_weights()[0], dtype=np.float32)


@pytest.fixture(scope="module")
def ctx(blob):
    from kws import _native

    c = _native.Context(0)
    c.use_torch_stream()
    c.load_dscnn(blob, C)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((POOL, 1, 99, 10)).astype(np.float32) * 8.0
    x[1] *= 3.0e4    # huge: the largest feature sets the clip's power-of-two units
    x[4] = 0.0       # all zero: every stage is bias only
    x[6] *= 1.0e-20  # tiny
    x[9] = 0.0
    x[9, 0, 50, 5] = -1.0e3  # one spike
    x[11] *= 2.0e3
    return torch.from_numpy(x).to(DEV)


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(ctx, feat):
    B = feat.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ctx.forward_f32(feat, logits, labels)
    torch.cuda.synchronize()
    return logits.cpu().numpy(), labels.cpu().numpy()


def _alone(ctx, pool):
    out = [_run(ctx, pool[i:i + 1].contiguous()) for i in range(POOL)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _check_batch(ctx, pool, ref, B, shift):
    ref_logits, ref_labels = ref
    idx = (7 * np.arange(B) + shift) % POOL
    logits, labels = _run(ctx, pool[torch.from_numpy(idx).to(DEV)].contiguous())
    bad = np.flatnonzero((logits.view(np.uint32) != ref_logits[idx].view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"B={B}: {bad.size} clips differ from the same clip alone, first at {bad[:5]} (pool {idx[bad[:5]]})"
    np.testing.assert_array_equal(labels, ref_labels[idx], err_msg=f"B={B}")


@pytest.fixture(scope="module")
def alone(ctx, pool):
    """Every pool clip alone under both arithmetics, computed once."""
    refs = {}
    for math in (4, 5):
        ctx.set_pointwise_math(math)
        refs[math] = _alone(ctx, pool)
        assert np.isfinite(refs[math][0]).all()
    ctx.set_pointwise_math(5)
    return refs


@pytest.mark.parametrize("math", [4, 5], ids=["KWS_PW_SPLIT_BF16", "KWS_PW_PAIR_F16"])
@pytest.mark.parametrize("which", ["n_cu+1", "2n_cu+3"])
def test_persistent_launch_matches_each_clip_alone(ctx, pool, alone, math, which):
    B = _n_cu() + 1 if which == "n_cu+1" else 2 * _n_cu() + 3
    ctx.set_pointwise_math(math)
    try:
        _check_batch(ctx, pool, alone[math], B, 3)
    finally:
        ctx.set_pointwise_math(5)


@pytest.mark.parametrize("math", [4, 5], ids=["KWS_PW_SPLIT_BF16", "KWS_PW_PAIR_F16"])
@pytest.mark.parametrize("loader", ["host", "device"])
def test_table_follows_the_model_loaded(ctx, pool, alone, blob, math, loader):
    """Second model, then the first again: each load rewrites image and table, and the persistent launch matches the one-clip
    kernel under the model that is loaded."""
    other = np.ascontiguousarray(blob * np.float32(0.75))

    def load(b):
        if loader == "host":
            ctx.load_dscnn(b, C)
        else:
            ctx.load_dscnn_device(torch.from_numpy(b).to(DEV), C)

    B = _n_cu() + 1
    ctx.set_pointwise_math(math)
    try:
        load(other)
        ref_other = _alone(ctx, pool)
        assert (ref_other[0].view(np.uint32) != alone[math][0].view(np.uint32)).any(), "the second model must differ"
        _check_batch(ctx, pool, ref_other, B, 5)
        load(blob)
        _check_batch(ctx, pool, alone[math], B, 5)
    finally:
        ctx.load_dscnn(blob, C)
        ctx.set_pointwise_math(5)
