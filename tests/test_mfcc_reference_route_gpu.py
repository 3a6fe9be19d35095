"""The wavefront-resident MFCC kernel compiled for the reference geometry (kws_mfcc_i16_ref_kernel, KWS_FE_ROUTE_AUTO) against the
generic wavefront-resident kernel it specialises (KWS_FE_ROUTE_GENERIC), inside one process.

The two run the same float32 operations in the same order, so the claim is equality of every output WORD (np.array_equal on the
raw uint32, no tolerance) and of the frames the precision flag lists, with the refinement on and off (the reference route has
an instantiation for each).  Inputs: batches of 1, 3 and 5 clips (5 wavefronts per clip: wavefront counts that are no multiple
of the workgroup's four, idle wavefronts in the last workgroup), an all-zero clip, a clip that is silent for its first half and
full-scale noise after it (a zero frame packed with a loud one), a +-1 LSB dither, and the 48 golden clips (flagged frames; every
clip has the partnerless 99th frame and the three-frame last chunk).  One call at 448 / 192 checks against the float64 oracle
that another wavefront-resident geometry is not captured by the reference route."""
import numpy as np
import pytest
import torch

from oracle import psf_mfcc as o_mfcc

pytestmark = pytest.mark.gpu

N = 16000


@pytest.fixture(scope="module")
def native():
    from kws import _native

    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(0)  # kws_create configures the reference front end: 16 kHz, 16000 samples, 400 / 160 / 512 / 26 / 10
    c.use_torch_stream()
    yield c
    c.close()


def _noise(batch, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(batch, N), dtype=np.int16)


def _half_silent():
    clip = _noise(1, 11)
    clip[0, : N // 2] = 0
    return clip


CASES = {
    "noise_b1": lambda g: _noise(1, 1),
    "noise_b3": lambda g: _noise(3, 3),
    "noise_b5": lambda g: _noise(5, 5),
    "all_zero": lambda g: np.zeros((1, N), dtype=np.int16),
    "half_silent_then_full_scale": lambda g: _half_silent(),
    "dither_1lsb": lambda g: np.random.default_rng(13).integers(-1, 2, size=(1, N)).astype(np.int16),
    "golden_48": lambda g: np.ascontiguousarray(g["clips"]),
}


def _run(ctx, native, dev, pcm, route):
    ctx.set_frontend_route(route)
    out = torch.full((pcm.shape[0], 1, 99, 10), float("nan"), dtype=torch.float32, device=dev)
    ctx.mfcc_i16(pcm, out)
    ctx.sync()
    total, refined, last = ctx.frontend_stats()
    return out.cpu().numpy(), refined, last


@pytest.mark.parametrize("refine", [True, False], ids=["refine_on", "refine_off"])
@pytest.mark.parametrize("case", list(CASES))
def test_reference_route_matches_the_generic_kernel_bit_for_bit(native, ctx, dev, e2e_golden, case, refine):
    clips = CASES[case](e2e_golden)
    assert clips.dtype == np.int16 and clips.shape[1] == N
    pcm = torch.from_numpy(clips).to(dev)
    ctx.set_frontend_refine(native.FE_REFINE_SPAN_DEFAULT if refine else 0.0)
    try:
        gen, refined0, last_gen = _run(ctx, native, dev, pcm, native.FE_ROUTE_GENERIC)
        ref, refined1, last_ref = _run(ctx, native, dev, pcm, native.FE_ROUTE_AUTO)
    finally:
        ctx.set_frontend_route(native.FE_ROUTE_AUTO)
        ctx.set_frontend_refine(native.FE_REFINE_SPAN_DEFAULT)
    print(f"[ref route] {case} refine={refine}: frames listed generic {last_gen} / reference {last_ref}, "
          f"differing words {int((gen.view(np.uint32) != ref.view(np.uint32)).sum())} of {gen.size}")
    assert not np.isnan(gen).any() and not np.isnan(ref).any(), "a row was not written"
    assert np.array_equal(gen.view(np.uint32), ref.view(np.uint32))
    assert last_ref == last_gen
    if refine:
        assert refined1 - refined0 == last_ref  # the reference route's own call rewrote exactly the frames it listed
        if case == "golden_48":
            assert last_ref > 0, "the golden clips hold flagged frames: the flag path of the reference kernel did not run"
    else:
        assert refined1 == refined0


def test_set_frontend_route_rejects_other_values(native, ctx):
    from kws.common.errors import AudioProcessingError

    with pytest.raises(AudioProcessingError):
        ctx.set_frontend_route(2)
    ctx.set_frontend_route(native.FE_ROUTE_AUTO)


def test_another_resident_geometry_keeps_the_generic_kernel(native, dev):
    """448 / 192 is a wavefront-resident geometry (a chunk's span is exactly the 1024 floats of the wavefront's buffer) but not the
    reference's: under KWS_FE_ROUTE_AUTO it must still run the kernel that reads the geometry at run time -- the reference
    kernel's constants (400 / 160) would give wrong frames.  The existing gate of the float32 front end against the float64 oracle."""
    n_samples = 4400
    spec = o_mfcc.FrontendSpec(sample_rate=16000, n_samples=n_samples, winlen=448 / 16000, winstep=192 / 16000, nfft=512, nfilt=26,
                               numcep=10, preemph=0.97, ceplifter=22)
    assert spec.frame_len == 448 and spec.frame_step == 192
    clips = np.random.default_rng(7).integers(-20000, 20000, size=(6, n_samples)).astype(np.int16)
    clips[3, : n_samples // 2] = 0
    want = np.stack([o_mfcc.mfcc(o_mfcc.pcm16_to_float(c), spec) for c in clips])
    c = native.Context(0)
    c.use_torch_stream()
    try:
        c.set_frontend(sample_rate=16000, n_samples=n_samples, frame_len=448, frame_step=192, nfft=512, nfilt=26, numcep=10,
                       preemph=0.97, ceplifter=22)
        assert c.frontend_shape() == (spec.num_frames, 10)
        c.set_frontend_route(native.FE_ROUTE_AUTO)
        out = torch.full((6, 1, spec.num_frames, 10), float("nan"), dtype=torch.float32, device=dev)
        c.mfcc_i16(torch.from_numpy(clips).to(dev), out)
        c.sync()
        got = out.cpu().numpy()[:, 0]
    finally:
        c.close()
    assert not np.isnan(got).any(), "a row was not written"
    err = float(np.abs(got - want).max())
    print(f"[ref route] 448/192 under AUTO: max err {err:.3e} against the float64 oracle")
    assert err <= 1e-4
