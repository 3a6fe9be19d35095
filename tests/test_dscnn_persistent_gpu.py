"""Persistent DS-CNN workgroups (kws_dscnn_fwd_kernel, PERSIST): above the CU count a workgroup carries several clips and
stages the next one in block 4's tail, so LDS planes, stage-maxima slots and pool partials outlive a clip.  Every clip's logits
and label must be bit-identical to the same clip run alone, wherever it sits in a batch and whatever clip ran before it on the
same workgroup.  The clip pool mixes ordinary, huge, tiny and all-zero maps: with f16 pairs a stale scale slot or pool
buffer from the previous clip changes the bits."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
C = 12
POOL = 13  # distinct clips; batch position i holds clip (7 i + shift) % POOL, so neighbours differ and every clip moves around


@pytest.fixture(scope="module")
def ctx():
    sys.path.insert(0, ROOT)
    import bench
    from kws import _native

    c = _native.Context(0)
    c.use_torch_stream()
    c.load_dscnn(bench.bench_weights()[0], C)
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


@pytest.mark.parametrize("math", [4, 5], ids=["bf16_triple", "f16_pair"])
def test_every_clip_matches_itself_alone(ctx, pool, math):
    ctx.set_pointwise_math(math)
    try:
        ref_logits, ref_labels = _alone(ctx, pool)
        assert np.isfinite(ref_logits).all()
        n_cu = _n_cu()
        for B, shift in [(1, 3), (255, 0), (256, 5), (257, 1), (1023, 2), (4096, 0), (4097, 4), (16 * n_cu + 5, 6),
                         (n_cu - 1, 1), (n_cu, 2), (n_cu + 1, 3)]:
            idx = (7 * np.arange(B) + shift) % POOL
            logits, labels = _run(ctx, pool[torch.from_numpy(idx).to(DEV)].contiguous())
            bad = np.flatnonzero((logits.view(np.uint32) != ref_logits[idx].view(np.uint32)).any(axis=1))
            assert bad.size == 0, f"B={B}: {bad.size} clips differ from the same clip alone, first at {bad[:5]} (pool {idx[bad[:5]]})"
            np.testing.assert_array_equal(labels, ref_labels[idx], err_msg=f"B={B}")
    finally:
        ctx.set_pointwise_math(5)


@pytest.mark.parametrize("math", [4, 5], ids=["bf16_triple", "f16_pair"])
def test_stamps_instantiation_matches_product(ctx, pool, math):
    """The diagnostics instantiation (stamps) runs persistent too: same logits, and every clip's stamps are in order."""
    ctx.set_pointwise_math(math)
    try:
        B = 3 * _n_cu() + 17
        idx = (7 * np.arange(B) + 1) % POOL
        feat = pool[torch.from_numpy(idx).to(DEV)].contiguous()
        ref_logits, _ = _run(ctx, feat)
        logits = torch.full((B, C), float("nan"), device=DEV)
        stamps = torch.zeros((B, 16), dtype=torch.int64, device=DEV)
        ctx.forward_stamps_f32(feat, logits, stamps, math)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(logits.cpu().numpy().view(np.uint32), ref_logits.view(np.uint32))
        st = stamps.cpu().numpy()
        assert (np.diff(st[:, :13], axis=1) >= 0).all(), "phase stamps out of order"
        assert (st[:, 13] > st[:, 10]).all(), "pool + fc of every clip ran after its block 4"
    finally:
        ctx.set_pointwise_math(5)
