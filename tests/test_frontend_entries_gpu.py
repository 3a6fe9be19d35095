"""The three MFCC entries -- kws_mfcc_i16, kws_mfcc_f32, kws_mfcc_augment_i16 -- run one host flow over three sources
(kws_frontend.hip, run_frontend): the same clips through each give the same bits and move the front end's counters alike."""
import os

import numpy as np
import pytest
import torch

from oracle import psf_mfcc as o_mfcc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def native():
    from kws import _native

    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture()
def ctx(native):
    c = native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


@pytest.fixture(scope="module")
def audit_clips():
    """The eight clips of the precision audit (tests/golden/make_audit_fixture.py): each has frames the float32 kernel flags."""
    return np.ascontiguousarray(np.concatenate(
        [np.load(os.path.join(GOLDEN, name))["clips"] for name in ("audit_hard_clips.npz", "audit_exception_clips.npz")]).astype(np.int16))


def run_entry(ctx, dev, entry, clips):
    """(features, rc, frontend_stats deltas: total frames, refined frames; rows the call refined) of one entry over clips."""
    B = len(clips)
    pcm = torch.from_numpy(clips).to(dev)
    out = torch.full((B, 1) + ctx.frontend_shape(), float("nan"), dtype=torch.float32, device=dev)
    before = ctx.frontend_stats()
    rc = 0
    if entry == "i16":
        ctx.mfcc_i16(pcm, out)
    elif entry == "f32":
        ctx.mfcc_f32(torch.from_numpy(o_mfcc.pcm16_to_float(clips)).to(dev), out)
    else:  # the fused loader entry over the same clips as the resident split: identity index, nothing else
        rc = ctx.mfcc_augment_i16(pcm, torch.arange(B, dtype=torch.int32, device=dev), out)
    ctx.sync()
    after = ctx.frontend_stats()
    return out.cpu().numpy(), rc, (after[0] - before[0], after[1] - before[1], after[2])


@pytest.mark.parametrize("refine", [True, False], ids=["refine", "no_refine"])
def test_flagged_frames_same_bits_and_same_accounting_from_every_source(native, ctx, dev, audit_clips, refine):
    assert audit_clips.shape == (8, 16000) and ctx.frontend_shape() == (99, 10)
    ctx.set_frontend_refine(native.FE_REFINE_SPAN_DEFAULT if refine else 0.0)
    got = {entry: run_entry(ctx, dev, entry, audit_clips) for entry in ("i16", "f32", "augment")}
    feat, rc, stats = got["i16"]
    assert rc == 0 and not np.isnan(feat).any()
    assert stats[0] == 8 * 99 and stats[1] == stats[2]
    assert stats[2] > 0 if refine else stats[2] == 0
    for entry in ("f32", "augment"):
        f, r, s = got[entry]
        assert r == 0
        assert np.array_equal(f.view(np.uint32), feat.view(np.uint32)), f"{entry}: {(f != feat).sum()} values differ from kws_mfcc_i16"
        assert s == stats, (entry, s, stats)


def test_float64_route_same_bits_no_frame_count_and_the_fused_entry_refuses(native, ctx, dev, audit_clips):
    ctx.set_frontend_math(native.FE_F64)
    a, _, sa = run_entry(ctx, dev, "i16", audit_clips)
    b, _, sb = run_entry(ctx, dev, "f32", audit_clips)
    assert not np.isnan(a).any()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sa[0] == 0 and sb[0] == 0
    _, rc, sc = run_entry(ctx, dev, "augment", audit_clips)
    assert rc == native.KWS_EUNSUPPORTED and sc[0] == 0


@pytest.mark.parametrize("frame_len", [320, 512])
def test_any_length_kernels_same_bits_from_float_and_int16(ctx, dev, frame_len):
    """Frame lengths outside (384, 448] take the *_any kernels; the shapes of test_mfcc_frame_length_boundaries."""
    n = 16000 // 2 + 37
    ctx.set_frontend(sample_rate=16000, n_samples=n, frame_len=frame_len, frame_step=160, nfft=512)
    clips = np.random.default_rng(frame_len).integers(-20000, 20000, size=(5, n), dtype=np.int16)
    clips[3, : n // 2] = 0  # leading silence: all-zero frames beside live ones
    a, _, sa = run_entry(ctx, dev, "i16", clips)
    b, _, sb = run_entry(ctx, dev, "f32", clips)
    assert not np.isnan(a).any()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{(a != b).sum()} of {a.size} values differ"
    assert sa == sb
