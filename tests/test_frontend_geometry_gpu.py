"""The MFCC front end across its configuration space: every kernel kws_set_frontend can route to -- the wavefront-resident int16
kernel, the fused loader kernel, the four tile kernels, the float64 kernel, the refinement kernel, the streaming frame kernel --
at filterbanks, cepstrum counts, hops, clip lengths and scalars other than the reference's 26 / 10 / 400 / 160 / 0.97 / 22.

The reference is always oracle/psf_mfcc.py in float64 (FrontendSpec + mfcc(pcm16_to_float(clip), spec)), and every case asserts
that the spec's frame_len / frame_step are the ones handed to set_frontend.

Gates.  The float32 kernels get the project's 1e-4 and the float64 kernel its 1e-5, both times the lifter's largest gain relative
to the default's: g = max(1, max(lifter_vector(numcep, L)) / 12) -- the lifter multiplies the cepstral error and 12 is the gain
of the default L = 22.  A structural error (a dropped chunk, a wrong lane, a missed pad column) is of order 0.1 .. 10.

Every test prints its measured figures ([geometry] lines, visible with -s) before it asserts."""
import functools

import numpy as np
import pytest
import torch

from oracle import psf_mfcc as o_mfcc
from speechlike import speechlike_clip

pytestmark = pytest.mark.gpu

TOL = 1e-4           # float32 front end against the float64 oracle (tests/test_gpu_parity.py)
PRECISE_TOL = 1e-5   # float64 front end: the float32 rounding of cepstra of magnitude <= 64 is 3.8e-6
FLAG_BAND = 0.01     # the flag is formed in float32: frames within this of the threshold may fall on either side


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


# ------------------------------------------------------------------------------------------------ shared helpers
def make_spec(sample_rate=16000, n_samples=4400, frame_len=400, frame_step=160, nfilt=26, numcep=10, preemph=0.97, ceplifter=22):
    """The oracle's spec of a geometry given in samples: winlen = frame_len / sample_rate must round back (psf rounds half up)."""
    spec = o_mfcc.FrontendSpec(sample_rate=sample_rate, n_samples=n_samples, winlen=frame_len / sample_rate,
                               winstep=frame_step / sample_rate, nfft=512, nfilt=nfilt, numcep=numcep, preemph=preemph,
                               ceplifter=ceplifter)
    assert spec.frame_len == frame_len and spec.frame_step == frame_step, (spec.frame_len, spec.frame_step)
    return spec


def configure(ctx, spec):
    ctx.set_frontend(sample_rate=spec.sample_rate, n_samples=spec.n_samples, frame_len=spec.frame_len, frame_step=spec.frame_step,
                     nfft=spec.nfft, nfilt=spec.nfilt, numcep=spec.numcep, preemph=spec.preemph, ceplifter=spec.ceplifter)
    assert ctx.frontend_shape() == (spec.num_frames, spec.numcep)


def gate(spec, tol):
    return tol * max(1.0, float(o_mfcc.lifter_vector(spec.numcep, spec.ceplifter).max()) / 12.0)


@functools.lru_cache(maxsize=None)
def noise_clips(n_samples, batch=6, dc=0, seed=7):
    """Uniform integer noise in [-20000, 20000) (+ a DC offset); clip 3 has a leading half of zeros.  Read-only."""
    clips = (np.random.default_rng(seed).integers(-20000, 20000, size=(batch, n_samples)) + dc).astype(np.int16)
    if batch > 3:
        clips[3, : n_samples // 2] = 0
    clips.setflags(write=False)
    return clips


@functools.lru_cache(maxsize=None)
def oracle_of(spec, dc=0, batch=6, seed=7):
    """float64 [B, frames, numcep] of noise_clips under spec, and the flag quantity [B, frames]; computed once per (spec, input)."""
    clips = noise_clips(spec.n_samples, batch, dc, seed)
    want = np.stack([o_mfcc.mfcc(o_mfcc.pcm16_to_float(c), spec) for c in clips])
    ratio = np.stack([peak_ratio(c, spec) for c in clips])
    want.setflags(write=False)
    ratio.setflags(write=False)
    return want, ratio


def peak_ratio(clip, spec):
    """log(largest bin power) - min log(mel energy) per frame, from the oracle's float64 spectrum: the quantity the float32 kernel's
    precision flag measures (include/kws_hip.h, kws_set_frontend_refine).  An all-zero frame gives -inf (never flagged)."""
    sig = o_mfcc.pcm16_to_float(clip)
    feat, _ = o_mfcc.fbank(sig, spec)
    ps = o_mfcc.powspec(o_mfcc.framesig(o_mfcc.preemphasis(sig, spec.preemph), spec.frame_len, spec.frame_step), spec.nfft)
    with np.errstate(divide="ignore"):
        return np.log(ps.max(axis=1)) - np.log(feat).min(axis=1)


def run_entry(ctx, dev, entry, clips, pcm=None):
    """(features [B, frames, numcep], rc, frames listed by the call) of one MFCC entry over clips; pcm: a device view to read
    the int16 samples from (an unaligned one, say) instead of a fresh copy."""
    B = len(clips)
    if pcm is None:
        pcm = torch.from_numpy(np.array(clips)).to(dev)
    out = torch.full((B, 1) + ctx.frontend_shape(), float("nan"), dtype=torch.float32, device=dev)
    rc = 0
    if entry == "i16":
        ctx.mfcc_i16(pcm, out)
    elif entry == "f32":
        ctx.mfcc_f32(torch.from_numpy(o_mfcc.pcm16_to_float(clips)).to(dev), out)
    else:  # the fused loader entry over the clips as a resident split: identity index, no augmentation
        rc = ctx.mfcc_augment_i16(pcm, torch.arange(B, dtype=torch.int32, device=dev), out)
    ctx.sync()
    return out.cpu().numpy()[:, 0], rc, ctx.frontend_stats()[2]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def worst(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any(), "a row was not written"
    return float(np.abs(got - want).max())


# ------------------------------------------------------------------------------------------------ A. filterbank and cepstrum sweep
FAST_BANKS = [  # (sample_rate, nfilt, numcep)
    (16000, 10, 10),  # 8-chunk segments (the row_shl:4 step), numcep == nfilt
    (16000, 9, 9),    # smallest fast-path filterbank at 16 kHz
    (16000, 13, 13),  # 6-chunk segments
    (48000, 26, 10),  # deep (5 chunks) at the default filter count
    (16000, 25, 10),  # nfp == 28 with a pad column
    (16000, 28, 10),  # nfp == 28 without
    (16000, 32, 32),  # top of the one-log branch, numcep at its limit
    (16000, 33, 10),  # first of the two-log branch, nfp 36
    (16000, 54, 32),  # all 64 lanes in use
    (8000, 59, 32),   # largest fast-path filterbank (63 lanes)
    (44100, 32, 13),  # zero-width segments, one-log branch
    (44100, 39, 13),  # zero-width segments, two-log branch
    (22050, 47, 20),  # zero-width segments at many filters
    (16000, 26, 1),   # energy only
]
# A zero-width segment BETWEEN filters (edges 0, 0, 1, 1, 2, ...: segments 0 and 2 are empty, at 48 kHz segment 6 too): filter 1 has
# no falling side (the nq select of mfcc_pair) and a rising side of one bin at weight 0, so psf's filter 1 is identically zero and
# floors to eps -- every live frame is over the refinement threshold.  The banks above have only segment 0 empty (the nr select).
INNER_GAP_BANKS = [(44100, 47, 20), (48000, 48, 13)]
SLOW_BANKS = [(16000, 8, 8), (16000, 55, 10), (16000, 64, 10)]  # a 9-chunk segment; more than 64 chunks; 65 segments
bank_id = lambda b: f"{b[0]}-{b[1]}-{b[2]}"


@pytest.mark.parametrize("bank", FAST_BANKS, ids=bank_id)
def test_filterbank_float32_kernels_on_their_own_bits(native, ctx, dev, bank):
    """Pass 1: preemph 0 and noise over a DC offset keep every frame's flag quantity under 9.8 (threshold 10.2), so the refinement
    lists nothing -- asserted -- and what is compared is the float32 kernels' own output: the wavefront-resident kernel
    (mfcc_i16) against the oracle, the tile kernel (mfcc_f32) and the fused loader kernel against it bit for bit.  26 frames: the
    resident kernel's last chunk holds two."""
    sr, nfilt, numcep = bank
    spec = make_spec(sample_rate=sr, nfilt=nfilt, numcep=numcep, preemph=0.0)
    configure(ctx, spec)
    assert ctx.frontend_math() == native.FE_F32, "the case fell to the float64 kernel"
    clips = noise_clips(spec.n_samples, dc=1200)
    want, ratio = oracle_of(spec, dc=1200)
    assert ratio.max() < native.FE_REFINE_SPAN_DEFAULT - 0.4, float(ratio.max())  # the input's side of the condition below
    got, _, listed = run_entry(ctx, dev, "i16", clips)
    assert listed == 0, f"{listed} frames listed: the input does not isolate the float32 kernel"
    err = worst(got, want)
    print(f"[geometry] A1 {bank_id(bank)}: float32 kernel alone, max err {err:.3e} (gate {gate(spec, TOL):.2e}), max flag ratio {ratio.max():.2f}")
    assert err <= gate(spec, TOL)
    f32, _, listed = run_entry(ctx, dev, "f32", clips)
    assert listed == 0 and same_bits(f32, got), f"tile kernel: {(f32 != got).sum()} values differ from the wavefront-resident kernel"
    aug, rc, listed = run_entry(ctx, dev, "augment", clips)
    assert rc == native.KWS_OK and listed == 0 and same_bits(aug, got), f"fused loader kernel: {(aug != got).sum()} values differ"


@pytest.mark.parametrize("bank", INNER_GAP_BANKS, ids=bank_id)
def test_filterbank_with_an_empty_segment_between_filters_float32_alone(native, ctx, dev, bank):
    """With the refinement on these banks list every live frame (pass 2 below), so the float32 kernels are isolated by switching
    it off: the identically-zero filter is exact in float32 too (zero weights), the other bands are ordinary noise bands."""
    sr, nfilt, numcep = bank
    spec = make_spec(sample_rate=sr, nfilt=nfilt, numcep=numcep, preemph=0.0)
    edges = o_mfcc.mel_bin_edges(nfilt, 512, sr)
    assert (np.diff(edges)[1:] == 0).any(), "no empty segment between two filters"
    configure(ctx, spec)
    assert ctx.frontend_math() == native.FE_F32
    ctx.set_frontend_refine(0.0)
    clips = noise_clips(spec.n_samples, dc=1200)
    want, _ = oracle_of(spec, dc=1200)
    got, _, listed = run_entry(ctx, dev, "i16", clips)
    err = worst(got, want)
    print(f"[geometry] A1 {bank_id(bank)}: float32 kernel alone (refinement off), max err {err:.3e} (gate {gate(spec, TOL):.2e})")
    assert listed == 0 and err <= gate(spec, TOL)
    f32, _, _ = run_entry(ctx, dev, "f32", clips)
    assert same_bits(f32, got), f"tile kernel: {(f32 != got).sum()} values differ from the wavefront-resident kernel"
    aug, rc, _ = run_entry(ctx, dev, "augment", clips)
    assert rc == native.KWS_OK and same_bits(aug, got), f"fused loader kernel: {(aug != got).sum()} values differ"


@pytest.mark.parametrize("bank", FAST_BANKS + INNER_GAP_BANKS, ids=bank_id)
def test_filterbank_with_refinement_and_in_float64(native, ctx, dev, bank):
    """Pass 2: the default preemph 0.97 on noise without the offset: narrow first filters push up to half the frames over the
    threshold.  Every frame within the gate; the listed count between the oracle's counts of frames over 10.2 + 0.01 and over
    10.2 - 0.01 (the band of test_mfcc_diverse_clips_incl_level_steps).  Pass 3: the same under KWS_FE_F64."""
    sr, nfilt, numcep = bank
    spec = make_spec(sample_rate=sr, nfilt=nfilt, numcep=numcep)
    configure(ctx, spec)
    assert ctx.frontend_math() == native.FE_F32
    clips = noise_clips(spec.n_samples)
    want, ratio = oracle_of(spec)
    thr = native.FE_REFINE_SPAN_DEFAULT
    lo, hi = int((ratio > thr + FLAG_BAND).sum()), int((ratio > thr - FLAG_BAND).sum())
    got, _, listed = run_entry(ctx, dev, "i16", clips)
    err = worst(got, want)
    print(f"[geometry] A2 {bank_id(bank)}: refined {listed} of {ratio.size} frames ({100.0 * listed / ratio.size:.1f} %, oracle {lo}..{hi}), "
          f"max err {err:.3e} (gate {gate(spec, TOL):.2e})")
    assert err <= gate(spec, TOL)
    assert lo <= listed <= hi, (lo, listed, hi)
    f32, _, listed_f32 = run_entry(ctx, dev, "f32", clips)
    assert listed_f32 == listed and same_bits(f32, got)
    ctx.set_frontend_math(native.FE_F64)
    assert ctx.frontend_math() == native.FE_F64
    p64, _, _ = run_entry(ctx, dev, "i16", clips)
    err64 = worst(p64, want)
    print(f"[geometry] A3 {bank_id(bank)}: float64 kernel, max err {err64:.3e} (gate {gate(spec, PRECISE_TOL):.2e})")
    assert err64 <= gate(spec, PRECISE_TOL)
    q64, _, _ = run_entry(ctx, dev, "f32", clips)
    assert same_bits(q64, p64)


@pytest.mark.parametrize("bank", SLOW_BANKS, ids=bank_id)
def test_filterbank_the_lane_layout_cannot_hold_runs_in_float64(native, ctx, dev, bank):
    sr, nfilt, numcep = bank
    spec = make_spec(sample_rate=sr, nfilt=nfilt, numcep=numcep)
    configure(ctx, spec)
    assert ctx.frontend_math() == native.FE_F64
    clips = noise_clips(spec.n_samples)
    want, _ = oracle_of(spec)
    before = ctx.frontend_stats()[0]
    got, _, _ = run_entry(ctx, dev, "i16", clips)
    err = worst(got, want)
    print(f"[geometry] A  {bank_id(bank)}: rerouted to float64, max err {err:.3e}")
    assert err <= gate(spec, PRECISE_TOL)
    f32, _, _ = run_entry(ctx, dev, "f32", clips)
    assert same_bits(f32, got)
    _, rc, _ = run_entry(ctx, dev, "augment", clips)
    assert rc == native.KWS_EUNSUPPORTED and ctx.frontend_stats()[0] == before  # no frame went through the float32 front end


@pytest.mark.parametrize("nfilt,numcep", [(26, 10), (13, 13)])
@pytest.mark.parametrize("preemph,ceplifter", [(0.0, 22), (0.5, 22), (1.0, 22), (0.97, 0), (0.97, 1), (0.97, 40)])
def test_preemphasis_and_lifter_scalars(native, ctx, dev, nfilt, numcep, preemph, ceplifter):
    spec = make_spec(nfilt=nfilt, numcep=numcep, preemph=preemph, ceplifter=ceplifter)
    configure(ctx, spec)
    assert ctx.frontend_math() == native.FE_F32
    clips = noise_clips(spec.n_samples)
    want, ratio = oracle_of(spec)
    thr = native.FE_REFINE_SPAN_DEFAULT
    got, _, listed = run_entry(ctx, dev, "i16", clips)
    err = worst(got, want)
    print(f"[geometry] A  scalars {nfilt}/{numcep} preemph {preemph} lifter {ceplifter}: max err {err:.3e} (gate {gate(spec, TOL):.2e}), {listed} refined")
    assert err <= gate(spec, TOL)
    assert (ratio > thr + FLAG_BAND).sum() <= listed <= (ratio > thr - FLAG_BAND).sum()
    f32, _, _ = run_entry(ctx, dev, "f32", clips)
    assert same_bits(f32, got)
    ctx.set_frontend_math(native.FE_F64)
    p64, _, _ = run_entry(ctx, dev, "i16", clips)
    assert worst(p64, want) <= gate(spec, PRECISE_TOL)


# ------------------------------------------------------------------------------------------------ B. clip length, hop, alignment
def check_geometry(native, ctx, dev, spec, resident, f32_first=False):
    """mfcc_i16 and mfcc_f32 against the oracle at the float32 gate and against each other bit for bit; the fused loader entry
    accepts exactly the wavefront-resident geometries (what mfcc_i16 then runs), with the same bits."""
    configure(ctx, spec)
    assert ctx.frontend_math() == native.FE_F32
    clips = noise_clips(spec.n_samples)
    want, _ = oracle_of(spec)
    a, _, listed = run_entry(ctx, dev, "f32" if f32_first else "i16", clips)
    err = worst(a, want)
    print(f"[geometry] B  {spec.frame_len}/{spec.frame_step} n {spec.n_samples} ({spec.num_frames} frames): max err {err:.3e}, {listed} refined")
    assert err <= gate(spec, TOL)
    b, _, listed_b = run_entry(ctx, dev, "i16" if f32_first else "f32", clips)
    assert listed_b == listed and same_bits(a, b), f"{(a != b).sum()} values differ between mfcc_i16 and mfcc_f32"
    aug, rc, _ = run_entry(ctx, dev, "augment", clips)
    if resident:
        assert rc == native.KWS_OK and same_bits(aug, a)
    else:
        assert rc == native.KWS_EUNSUPPORTED
    return a


@pytest.mark.parametrize("frame_len,frame_step,resident", [
    (400, 160, True), (385, 2, True), (448, 192, True),  # 448/192: a chunk's span is exactly the 1024 floats of the wavefront's buffer
    (448, 190, True), (400, 8, True),
    (448, 194, False), (400, 161, False),                 # span over 1024; 4 hops no multiple of 8 samples: the tile kernel
])
def test_wavefront_resident_hops_and_their_neighbours(native, ctx, dev, frame_len, frame_step, resident):
    check_geometry(native, ctx, dev, make_spec(frame_len=frame_len, frame_step=frame_step), resident)


@pytest.mark.parametrize("n_samples", [4240, 4400, 4560, 4720,  # 25 .. 28 frames: the last chunk holds 1, 2, 3, 4
                                       4408,                    # the last frame has 8 real samples
                                       400, 392, 8])            # one frame: exact, zero-padded, the whole clip one vector
def test_wavefront_resident_clip_lengths(native, ctx, dev, n_samples):
    check_geometry(native, ctx, dev, make_spec(n_samples=n_samples), True)


def test_unaligned_clips_take_the_tile_kernel_scalar_loads(native, ctx, dev):
    """n_samples 4401: no clip but the first starts on a 16-byte boundary.  And an aligned geometry read through a pointer one
    sample off: mfcc_i16 gives the same bits as from the aligned copy, the fused loader refuses."""
    check_geometry(native, ctx, dev, make_spec(n_samples=4401), False)
    spec = make_spec()
    aligned = check_geometry(native, ctx, dev, spec, True)
    clips = noise_clips(spec.n_samples)
    buf = torch.zeros(clips.size + 1, dtype=torch.int16, device=dev)
    view = buf[1:].view(clips.shape)
    view.copy_(torch.from_numpy(np.array(clips)))
    off, _, _ = run_entry(ctx, dev, "i16", clips, pcm=view)
    assert same_bits(off, aligned)
    _, rc, _ = run_entry(ctx, dev, "augment", clips, pcm=view)
    assert rc == native.KWS_EUNSUPPORTED


@pytest.mark.parametrize("frame_len,frame_step,n_samples", [
    (400, 160, 4080), (400, 160, 4240), (400, 160, 7760), (400, 160, 7920), (400, 160, 8080),  # 24, 25, 47, 48, 49 frames
    (400, 500, 4400),   # samples between frames are never used
    (400, 400, 4400),
    (512, 1000, 8000),  # the *_any kernels with more than 64 KB of LDS: the opt-in path
])
def test_tile_kernels_frame_counts_and_hops(native, ctx, dev, frame_len, frame_step, n_samples):
    spec = make_spec(n_samples=n_samples, frame_len=frame_len, frame_step=frame_step)
    check_geometry(native, ctx, dev, spec, frame_step == 160, f32_first=True)


@pytest.mark.parametrize("frame_step", [1600, 4000])
def test_large_hops_are_decided_at_configuration_time(native, ctx, dev, frame_step):
    """The tile kernels stage 23 hops + one frame in LDS; beyond 160 KB they cannot be launched.  Either kws_set_frontend refuses
    the geometry, or kws_frontend_math reports the arithmetic in use and both entries are oracle-correct with it: nothing fails
    at call time.  (It routes to the float64 kernel; the float32-only entries refuse.)"""
    from kws.common.errors import AudioProcessingError

    spec = make_spec(n_samples=400 + 5 * frame_step, frame_step=frame_step)
    try:
        configure(ctx, spec)
    except AudioProcessingError as e:
        assert f"(code {native.KWS_EUNSUPPORTED})" in str(e)
        return
    math = ctx.frontend_math()
    clips = noise_clips(spec.n_samples)
    want, _ = oracle_of(spec)
    a, _, _ = run_entry(ctx, dev, "i16", clips)
    b, _, _ = run_entry(ctx, dev, "f32", clips)
    err = worst(a, want)
    print(f"[geometry] B  400/{frame_step}: math {math}, max err {err:.3e}")
    assert err <= gate(spec, PRECISE_TOL if math == native.FE_F64 else TOL)
    assert same_bits(a, b)
    if math == native.FE_F64:
        _, rc, _ = run_entry(ctx, dev, "augment", clips)
        assert rc == native.KWS_EUNSUPPORTED
        with pytest.raises(AudioProcessingError, match=f"code {native.KWS_EUNSUPPORTED}"):
            ctx.stream_open(2)


# ------------------------------------------------------------------------------------------------ C. chunks per wavefront
@pytest.fixture(scope="module")
def pool64():
    """64 distinct clips of 4400 samples: 32 of noise, 32 cut from speech-like clips (dense flags)."""
    speech = [speechlike_clip(500 + i, -6.0 - 4.0 * i, "zeros" if i % 2 == 0 else "dither") for i in range(11)]
    cuts = [c[k * 4400:(k + 1) * 4400] for c in speech for k in range(3)][:32]
    clips = np.concatenate([noise_clips(4400, batch=32, seed=11), np.stack(cuts)]).astype(np.int16)
    assert clips.shape == (64, 4400)
    return np.ascontiguousarray(clips)


@pytest.mark.parametrize("entry", ["i16", "augment"])
def test_chunks_per_wavefront(native, ctx, dev, pool64, entry):
    """A wavefront of the resident kernels owns 1 chunk of a clip in small batches; with 7 chunks per clip, batches of 1200, 2400
    and 3600 clips give it 3, 5 and 7 (runs of 3+3+1, 5+2 and 7), where the chunk loop, the flag mask and its flush carry more than
    one chunk.  The batch repeats 64 distinct clips: every row must carry the bits of the 64-clip call, which goes against the
    oracle, and the call lists what its rows list in the small calls -- B // 64 times the 64-clip call's count plus that of
    the B % 64 clips left over."""
    spec = make_spec()
    configure(ctx, spec)
    pcm = torch.from_numpy(pool64).to(dev)

    def run(rows):
        idx = torch.arange(rows, dtype=torch.int32, device=dev) % 64
        out = torch.full((rows, 1, spec.num_frames, spec.numcep), float("nan"), dtype=torch.float32, device=dev)
        if entry == "i16":
            ctx.mfcc_i16(pcm[idx.long()].contiguous(), out)
        else:
            assert ctx.mfcc_augment_i16(pcm, idx, out) == native.KWS_OK
        ctx.sync()
        return out, ctx.frontend_stats()[2]

    small, listed64 = run(64)
    want = np.stack([o_mfcc.mfcc(o_mfcc.pcm16_to_float(c), spec) for c in pool64])
    err = worst(small.cpu().numpy()[:, 0], want)
    ratio = np.stack([peak_ratio(c, spec) for c in pool64])
    thr = native.FE_REFINE_SPAN_DEFAULT
    print(f"[geometry] C  {entry}: 64 clips max err {err:.3e}, {listed64} of {ratio.size} frames refined")
    assert err <= gate(spec, TOL)
    assert (ratio > thr + FLAG_BAND).sum() <= listed64 <= (ratio > thr - FLAG_BAND).sum()
    assert (ratio > thr + FLAG_BAND).sum(axis=1).max() >= 3, "no clip has flags in several pairs: the flush would carry one entry"
    rng = np.random.default_rng(5)
    for B in (1200, 2400, 3600):
        big, listed = run(B)
        _, listed_rest = run(B % 64)
        assert listed == (B // 64) * listed64 + listed_rest, (B, listed, listed64, listed_rest)
        same = (big.view(torch.int32) == small.view(torch.int32)[torch.arange(B, device=dev) % 64]).flatten(1).all(dim=1).cpu().numpy()
        rows = np.concatenate([[0, 63, 64, B - 1], rng.integers(0, B, 20)])
        assert same[rows].all() and same.all(), f"B {B}: rows {np.nonzero(~same)[0][:8].tolist()} differ from the 64-clip call"


# ------------------------------------------------------------------------------------------------ D. streaming frame kernel
@pytest.mark.parametrize("frame_len,frame_step,nfilt,numcep", [
    (400, 400, 26, 10),  # one hop per frame
    (400, 100, 26, 10),  # four
    (512, 128, 26, 10),
    (448, 192, 26, 10),
    (400, 160, 13, 13),  # deep segments
    (400, 160, 40, 13),  # two-log branch
    (400, 160, 32, 32),  # numcep at its limit (it may not exceed nfilt: 26 / 32 is refused, see below)
])
def test_streaming_frame_kernel_geometries(native, ctx, dev, frame_len, frame_step, nfilt, numcep):
    """Features-only pushes (the frame kernel alone) of three streams -- the last packed pair has no partner, one stream is 40
    times quieter -- into a ring of 12 frames over 30 hops, so it wraps twice.  Ring row f mod 12 holds frame f of the continuous
    signal, the newest being hops - K, K = ceil(frame_len / frame_step); rows never written are zero."""
    S, hops, T = 3, 30, 12
    K = -(-frame_len // frame_step)
    spec = make_spec(n_samples=frame_len + (T - 1) * frame_step, frame_len=frame_len, frame_step=frame_step, nfilt=nfilt, numcep=numcep)
    configure(ctx, spec)
    assert spec.num_frames == T
    pcm = np.random.default_rng(91).integers(-20000, 20000, size=(S, hops * frame_step)).astype(np.int16)
    pcm[1] //= 40
    whole = make_spec(n_samples=hops * frame_step, frame_len=frame_len, frame_step=frame_step, nfilt=nfilt, numcep=numcep)
    allf = np.stack([o_mfcc.mfcc(o_mfcc.pcm16_to_float(x), whole) for x in pcm])  # frame f depends on samples < f * step + frame_len only
    ctx.stream_open(S)
    dpcm = torch.from_numpy(pcm).to(dev)
    ring = torch.empty((S, T, numcep), dtype=torch.float32, device=dev)
    worst_err = 0.0
    for t in range(hops):
        ctx.stream_push_i16(dpcm[:, t * frame_step:(t + 1) * frame_step].contiguous())
        if t not in (K - 1, K, 11, 12, 13, 29):
            continue
        _, pushed = ctx.stream_state()
        assert pushed == t + 1
        ctx.stream_copy_features(ring)
        ctx.sync()
        got = ring.cpu().numpy()
        newest = t + 1 - K
        want = np.zeros((S, T, numcep))
        for f in range(max(0, newest - T + 1), newest + 1):
            want[:, f % T] = allf[:, f]
        err = float(np.abs(got - want).max())
        worst_err = max(worst_err, err)
        assert err <= gate(spec, TOL), f"hop {t}: {err:.3e}"
    print(f"[geometry] D  {frame_len}/{frame_step} {nfilt}/{numcep}: K {K}, max err {worst_err:.3e}")
    ctx.stream_close()


def test_streaming_refuses_hops_beyond_512_samples(native, ctx):
    from kws.common.errors import AudioProcessingError

    with pytest.raises(AudioProcessingError, match=f"code {native.KWS_EUNSUPPORTED}"):
        ctx.set_frontend(n_samples=400 + 11 * 160, nfilt=26, numcep=32)  # more cepstra than filters: no such front end
    configure(ctx, make_spec(n_samples=400 + 11 * 513, frame_step=513))
    assert ctx.frontend_math() == native.FE_F32
    with pytest.raises(AudioProcessingError, match=f"code {native.KWS_EUNSUPPORTED}"):
        ctx.stream_open(3)


# ------------------------------------------------------------------------------------------------ E. scan at another hop
def test_scan_at_a_non_default_hop(native, ctx, dev, e2e_golden):
    """kws_scan_i16 needs 99 x 10 windows, not 400 / 160: frames of 448 samples 192 apart.  Its frames against the oracle on the
    whole recording, and bit for bit against kws_mfcc_i16 on a context whose clips are as long as the recording; window 0's logits
    are kws_forward_f32 on rows 0 .. 98."""
    R, hop_frames = 2, 3
    n_samples = 448 + 98 * 192
    n_total = n_samples + 7 * 192
    spec = make_spec(n_samples=n_samples, frame_len=448, frame_step=192)
    whole = make_spec(n_samples=n_total, frame_len=448, frame_step=192)
    configure(ctx, spec)
    assert spec.num_frames == 99 and ctx.frontend_math() == native.FE_F32
    ctx.load_dscnn(e2e_golden["he.blob"], 12)
    F, W = native.host_scan_shape(n_total, 448, 192, 99, hop_frames)
    assert (F, W) == (whole.num_frames, 3) == (106, 3)
    rec = noise_clips(n_total, batch=R, seed=23)
    pcm = torch.from_numpy(np.array(rec)).to(dev)
    logits = torch.full((R, W, 12), float("nan"), device=dev)
    labels = torch.full((R, W), -1, dtype=torch.int32, device=dev)
    feat = torch.full((R, F, 10), float("nan"), device=dev)
    ctx.scan_i16(pcm, hop_frames, logits, labels, feat)
    ctx.sync()
    want, _ = oracle_of(whole, batch=R, seed=23)
    err = worst(feat.cpu().numpy(), want)
    print(f"[geometry] E  scan 448/192: frames max err {err:.3e}")
    assert err <= gate(whole, TOL)
    other = native.Context(0)
    try:
        other.use_torch_stream()
        configure(other, whole)
        clip_feat, _, _ = run_entry(other, dev, "i16", rec)
    finally:
        other.close()
    assert same_bits(feat.cpu().numpy(), clip_feat)
    want_logits = torch.full((R, 12), float("nan"), device=dev)
    ctx.forward_f32(feat[:, :99].contiguous().view(R, 1, 99, 10), want_logits)
    ctx.sync()
    assert torch.isfinite(logits).all() and torch.equal(logits[:, 0], want_logits)
