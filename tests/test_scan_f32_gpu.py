"""float32 recordings on the GPU: kws_frames_f32, kws_scan_f32, kws_cut_f32 and KeywordSpotter.scan_f32 / segment_f32 and the file
methods' decode="any".

Every comparison is on the words (np.array_equal on uint32 views, torch.equal) unless a tolerance is named; no frame and no clip
is exempt.  The strongest check of the new source path is the GRID PROPERTY: x[i] = (float)pcm[i] / 32768 is exact, and the int16
entries scale their PCM by that same exact division, so the float entry must reproduce the int16 entry's frames, logits, labels
and kws_frontend_stats increments bit for bit -- at lengths on a multiple of 8 (the wavefront-resident float kernel) and off it
(the tile kernel), with the refinement on and off, in float32 and under KWS_FE_F64."""
import struct
import wave

import numpy as np
import pytest
import torch

import _scan_ref as sref
import _segment_ref as gref
from _f32_ref import cut_f32_ref, n_for_frames, unit
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
T_WIN, N_CEP, FRAME_LEN, FRAME_STEP = sref.T_WIN, sref.N_CEP, sref.FRAME_LEN, sref.FRAME_STEP
TOL = 1e-4  # the project's MFCC gate (tests/test_gpu_parity.py)
u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)


# the edge lengths of tests/test_ragged_gpu.py: one sample, around one frame, around a second, frame counts 19-22 around a
# wavefront's run of 20 frames; on and off a multiple of 8, so both routes run
EDGE_LENGTHS = [1, 399, 400, 401, 560, 16000, 16001, 16007, 16008, n_for_frames(19), n_for_frames(20, 3), n_for_frames(21),
                n_for_frames(22, 150), 48000]


@pytest.fixture(scope="module")
def clips(e2e_golden):
    return e2e_golden["clips"]


@pytest.fixture(scope="module")
def ctx(e2e_golden):
    c = _native.Context(0)
    c.use_torch_stream()
    c.load_dscnn(e2e_golden["he.blob"], C)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_clip_ctx():
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def _frames(c, x, f32):
    """(frames [R, F, 10] on the device, (frames counted, frames refined)) of kws_frames_f32 / kws_frames_i16, into a prefilled
    and over-allocated buffer."""
    R, n = x.shape
    F, _ = sref.scan_shape(n, 1)
    before = c.frontend_stats()
    feat = torch.full((R + 1, F, N_CEP), float("nan"), device=DEV)
    (c.frames_f32 if f32 else c.frames_i16)(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), feat[:R])
    torch.cuda.synchronize()
    after = c.frontend_stats()
    assert torch.isnan(feat[R]).all(), "frames were written beyond [R, F_total, numcep]"
    assert not torch.isnan(feat[:R]).any(), "a frame was not written"
    return feat[:R], (after[0] - before[0], after[1] - before[1])


# ---- 1. the grid property, frames ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [_native.FE_F32, _native.FE_F64], ids=["default", "f64"])
@pytest.mark.parametrize("refine", [True, False], ids=["refine", "norefine"])
@pytest.mark.parametrize("R", [1, 3])
def test_grid_property_frames(ctx, R, refine, math):
    rng = np.random.default_rng(100 + R)
    ctx.set_frontend_math(math)
    ctx.set_frontend_refine(_native.FE_REFINE_SPAN_DEFAULT if refine else 0.0)
    try:
        refined_total = 0
        for n in EDGE_LENGTHS:
            pcm = np.round(rng.normal(0.0, 2500.0, (R, n))).clip(-32768, 32767).astype(np.int16)
            if n >= 16000:  # a tone near the top of the band on one recording: frames the refinement redoes
                pcm[0] = np.round(20000 * np.sin(2 * np.pi * 7900.0 * np.arange(n) / 16000.0)).astype(np.int16)
            want, want_stats = _frames(ctx, pcm, f32=False)
            got, got_stats = _frames(ctx, unit(pcm), f32=True)
            bad = (got != want).any(dim=2).nonzero()
            assert bad.numel() == 0, f"n_total {n}: {bad.shape[0]} frames differ from kws_frames_i16, first {bad[:4].tolist()}"
            assert got_stats == want_stats, f"n_total {n}: kws_frontend_stats counts {got_stats}, the int16 entry {want_stats}"
            assert want_stats[0] == (R * sref.scan_shape(n, 1)[0] if math == _native.FE_F32 else 0)
            refined_total += want_stats[1]
        assert (refined_total > 0) == (refine and math == _native.FE_F32), "the refinement leg is vacuous"
    finally:
        ctx.set_frontend_math(_native.FE_F32)
        ctx.set_frontend_refine(_native.FE_REFINE_SPAN_DEFAULT)


# ---- 2. off-grid signals ---------------------------------------------------------------------------------------------------
SUBNORMAL = slice(5000, 5240)


def off_grid_signals(n):
    """float32 [5, n]: Gaussian noise at 0.1; a tone mixture near the top of the band (the refinement flags its frames); noise at
    1e-6 and at 4.0 (beyond +-1: nothing is clamped); noise with one NaN-free stretch of subnormal values.  The stretch is 240
    samples, shorter than frame_len - frame_step: every frame that touches it also holds at least 160 normal samples, so its
    powers stay inside float32 -- a frame of subnormals alone has powers below 1e-76, which no float32 front end can take the
    logarithm of, whatever the source path does."""
    rng = np.random.default_rng(n)
    t = np.arange(n) / 16000.0
    x = np.empty((5, n), np.float32)
    x[0] = rng.normal(0.0, 0.1, n)
    x[1] = 0.55 * np.sin(2 * np.pi * 7000.0 * t) + 0.3 * np.sin(2 * np.pi * 7900.0 * t + 0.3)
    x[2] = rng.normal(0.0, 1e-6, n)
    x[3] = rng.normal(0.0, 4.0, n)
    x[4] = rng.normal(0.0, 0.1, n)
    x[4, SUBNORMAL] = (rng.integers(-4000, 4001, SUBNORMAL.stop - SUBNORMAL.start) * np.float64(1e-42)).astype(np.float32)
    sub = x[4, SUBNORMAL]
    assert np.isfinite(x).all() and (np.abs(sub[sub != 0]) < np.finfo(np.float32).tiny).all() and np.count_nonzero(sub) > 200
    assert np.abs(x[3]).max() > 1.0
    return x


@pytest.mark.parametrize("math", [_native.FE_F32, _native.FE_F64], ids=["default", "f64"])
@pytest.mark.parametrize("n_total", [16081, 21973, 21976, 48000])
def test_off_grid_frames_are_kws_mfcc_f32_of_one_long_clip(ctx, long_clip_ctx, n_total, math):
    x = off_grid_signals(n_total)
    R, F = x.shape[0], sref.scan_shape(n_total, 1)[0]
    ctx.set_frontend_math(math)
    long_clip_ctx.set_frontend(n_samples=n_total)
    long_clip_ctx.set_frontend_math(math)
    try:
        before_other = long_clip_ctx.frontend_stats()
        got, stats = _frames(ctx, x, f32=True)
        want = torch.full((R, 1, F, N_CEP), float("nan"), device=DEV)
        long_clip_ctx.mfcc_f32(torch.from_numpy(x).to(DEV), want)
        torch.cuda.synchronize()
        after_other = long_clip_ctx.frontend_stats()
        bad = (got != want[:, 0]).any(dim=2).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} frames differ from kws_mfcc_f32 on a {n_total}-sample clip, first {bad[:4].tolist()}"
        assert stats == (after_other[0] - before_other[0], after_other[1] - before_other[1]), "kws_frontend_stats counts differently"
        if math == _native.FE_F32:
            assert stats[0] == R * F and stats[1] > 0, "the tone mixture must flag frames"
        assert ctx.frontend_shape() == (T_WIN, N_CEP), "the context's own clip length must not change"
        if n_total == 16081:
            from oracle import psf_mfcc as o_mfcc

            spec = o_mfcc.FrontendSpec(n_samples=n_total)
            host = got.cpu().numpy().astype(np.float64)
            for r in range(R):
                err = np.abs(host[r] - o_mfcc.mfcc(x[r], spec)).max(axis=1)
                print(f"[scan-f32-oracle] signal {r} math {math}: max |mfcc - psf| = {err.max():.3e} (gate {TOL:.0e})")
                assert err.max() <= TOL, f"signal {r}: frame {int(err.argmax())} is {err.max():.3e} from psf.mfcc"
    finally:
        ctx.set_frontend_math(_native.FE_F32)


# ---- 3. a pure tone --------------------------------------------------------------------------------------------------------
def test_a_float_tone_flags_every_frame_and_the_worklist_holds_them(ctx, long_clip_ctx):
    """tests/test_scan_gpu.py's tone test on float32 samples: the worklist must hold R * F_total frames."""
    from oracle import psf_mfcc as o_mfcc

    n, R = 48000, 2
    t = np.arange(n) / 16000.0
    x = np.stack([(0.61 * np.sin(2 * np.pi * f * t)).astype(np.float32) for f in (7000.0, 7900.0)])
    must = 0
    for sig in x:
        band, _ = o_mfcc.fbank(sig, o_mfcc.FrontendSpec(n_samples=n))
        ps = o_mfcc.powspec(o_mfcc.framesig(o_mfcc.preemphasis(sig, 0.97), 400, 160), 512)
        must += int((np.log(ps.max(axis=1)) - np.log(band).min(axis=1) > _native.FE_REFINE_SPAN_DEFAULT + 1.0).sum())
    frames = R * sref.scan_shape(n, 1)[0]
    assert must == frames == 598, "the fixture: every frame of both tones is far over the flag's threshold"
    long_clip_ctx.set_frontend(n_samples=n)
    long_clip_ctx.set_frontend_math(_native.FE_F32)
    got, stats = _frames(ctx, x, f32=True)
    want = torch.full((R, 1, frames // R, N_CEP), float("nan"), device=DEV)
    long_clip_ctx.mfcc_f32(torch.from_numpy(x).to(DEV), want)
    torch.cuda.synchronize()
    assert torch.equal(got, want[:, 0])
    assert stats[0] == frames and must <= stats[1] <= frames, f"{stats[1]} frames were redone in float64, the oracle flags {must}"


# ---- 4. scan ---------------------------------------------------------------------------------------------------------------
def _scan(c, x, hop, f32, keep_frames=True):
    R, n = x.shape
    F, W = sref.scan_shape(n, hop)
    d = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    logits = torch.full((R + 1, W, C), float("nan"), device=DEV)
    labels = torch.full((R + 1, W), -1, dtype=torch.int32, device=DEV)
    feat = torch.full((R + 1, F, N_CEP), float("nan"), device=DEV) if keep_frames else None
    (c.scan_f32 if f32 else c.scan_i16)(d, hop, logits[:R], labels[:R], feat[:R] if keep_frames else None)
    torch.cuda.synchronize()
    assert torch.isfinite(logits[:R]).all() and torch.isnan(logits[R]).all(), "logits: a window missing, or written beyond [R, W, C]"
    assert ((labels[:R] >= 0) & (labels[:R] < C)).all() and (labels[R] == -1).all()
    if keep_frames:
        assert torch.isfinite(feat[:R]).all() and torch.isnan(feat[R]).all()
    return logits[:R], labels[:R], (feat[:R] if keep_frames else None)


def test_a_one_second_float_recording_is_kws_infer_f32(ctx, clips):
    rng = np.random.default_rng(3)
    x = unit(clips[[3, 8, 20, 33, 41]]) * rng.uniform(0.3, 1.7, (5, 1)).astype(np.float32)  # off the int16 grid
    logits, labels, _ = _scan(ctx, x, 1, f32=True)
    assert logits.shape == (5, 1, C)
    want_logits = torch.full((5, C), float("nan"), device=DEV)
    want_labels = torch.full((5,), -1, dtype=torch.int32, device=DEV)
    ctx.infer_f32(torch.from_numpy(x).to(DEV), want_logits, want_labels)
    torch.cuda.synchronize()
    assert torch.equal(logits[:, 0], want_logits) and torch.equal(labels[:, 0], want_labels)
    logits2, labels2, _ = _scan(ctx, x, 1, f32=True, keep_frames=False)  # the frames in the context's workspace: same results
    assert torch.equal(logits2, logits) and torch.equal(labels2, labels)


@pytest.mark.parametrize("math", [_native.PW_SPLIT_BF16, _native.PW_PAIR_F16], ids=["bf16_triple", "f16_pair"])
@pytest.mark.parametrize("R,n_total,hop", [(1, 16081, 1), (2, 48000, 7), (1, 64000, 150)])
def test_float_windows_are_kws_forward_f32_and_the_grid_property_holds(ctx, clips, R, n_total, hop, math):
    ctx.set_pointwise_math(math)
    try:
        pcm = sref.mixed_recordings(R, n_total, clips, seed=hop)
        logits, labels, feat = _scan(ctx, unit(pcm), hop, f32=True)
        frames_alone, _ = _frames(ctx, unit(pcm), f32=True)
        assert torch.equal(feat, frames_alone), "the scan's frames are not those of kws_frames_f32"
        x = feat.unfold(1, T_WIN, hop).permute(0, 1, 3, 2).reshape(-1, 1, T_WIN, N_CEP).contiguous()
        assert x.shape[0] == R * sref.scan_shape(n_total, hop)[1]
        want_logits = torch.full((x.shape[0], C), float("nan"), device=DEV)
        want_labels = torch.full((x.shape[0],), -1, dtype=torch.int32, device=DEV)
        ctx.forward_f32(x, want_logits, want_labels)
        torch.cuda.synchronize()
        assert torch.equal(logits.reshape(-1, C), want_logits) and torch.equal(labels.reshape(-1), want_labels)
        i_logits, i_labels, i_feat = _scan(ctx, pcm, hop, f32=False)
        assert torch.equal(feat, i_feat) and torch.equal(logits, i_logits) and torch.equal(labels, i_labels), \
            "kws_scan_f32(pcm / 32768) differs from kws_scan_i16(pcm)"
    finally:
        ctx.set_pointwise_math(_native.PW_PAIR_F16)


def _scan_rc(c, wav, R, n, hop, logits, label=None, feat=None):
    p = lambda t: t.data_ptr() if t is not None else None
    return c._lib.kws_scan_f32(c._h, p(wav), R, n, hop, p(logits), p(label), p(feat))


def test_scan_f32_scope_and_argument_errors(ctx, e2e_golden):
    """The checks of tests/test_scan_gpu.py::test_scan_scope_and_argument_errors, through kws_scan_f32."""
    wav = torch.zeros((1, 32000), dtype=torch.float32, device=DEV)
    logits = torch.full((1, 101, C), float("nan"), device=DEV)
    ctx.set_pointwise_math(_native.PW_F32)
    try:
        assert _scan_rc(ctx, wav, 1, 32000, 1, logits) == _native.KWS_EUNSUPPORTED
    finally:
        ctx.set_pointwise_math(_native.PW_PAIR_F16)
    other = _native.Context(0)
    try:
        other.use_torch_stream()
        assert _scan_rc(other, wav, 1, 32000, 1, logits) == _native.KWS_ESTATE  # no model
        other.load_dscnn(e2e_golden["he.blob"], C)
        other.set_frontend(n_samples=24000)  # 149 x 10 windows: not the fused kernel's map
        assert _scan_rc(other, wav, 1, 32000, 1, logits) == _native.KWS_EUNSUPPORTED
        other.set_frontend(numcep=13)
        assert _scan_rc(other, wav, 1, 32000, 1, logits) == _native.KWS_EUNSUPPORTED
    finally:
        other.close()
    assert _scan_rc(ctx, None, 1, 32000, 1, logits) == _native.KWS_EINVAL
    assert "kws_scan_f32: d_wav / d_logits is NULL" in ctx._lib.kws_last_error(ctx._h).decode()
    assert _scan_rc(ctx, wav, 1, 32000, 1, None) == _native.KWS_EINVAL
    assert _scan_rc(ctx, wav, 0, 32000, 1, logits) == _native.KWS_EINVAL
    assert _scan_rc(ctx, wav, 1, 32000, 0, logits) == _native.KWS_EINVAL
    assert _scan_rc(ctx, wav, 1, 15840, 1, logits) == _native.KWS_EINVAL  # 98 frames: shorter than a window
    feat = torch.full((1, 199, N_CEP), float("nan"), device=DEV)
    assert ctx._lib.kws_frames_f32(ctx._h, None, 1, 32000, feat.data_ptr()) == _native.KWS_EINVAL
    assert ctx._lib.kws_frames_f32(ctx._h, wav.data_ptr(), 1, 32000, None) == _native.KWS_EINVAL
    assert ctx._lib.kws_frames_f32(ctx._h, wav.data_ptr(), 0, 32000, feat.data_ptr()) == _native.KWS_EINVAL
    assert ctx._lib.kws_frames_f32(ctx._h, wav.data_ptr(), 1, 0, feat.data_ptr()) == _native.KWS_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(logits).all() and torch.isnan(feat).all(), "a refused call wrote results"


# ---- 5. cut ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cut_case():
    """R = 3 recordings of 4001 samples (rows not 16-byte aligned), off the int16 grid, and the spans of the test."""
    R, n = 3, 4001
    rng = np.random.default_rng(23)
    x = rng.normal(0.0, 0.08, (R, n)).astype(np.float32)
    x[0, 3000] = 0.97             # the first recording's peak, beyond n_out = 7 and beyond nothing of n_out = 16000
    x[0, 20] = -0.93              # the largest magnitude among its first samples
    x[1, 2000:2300] = 0.0         # an all-zero span
    x[1, 2100] = -0.0
    x[2, 3100] = np.nan           # a span holding one NaN
    spans = [(0, 0, 4001),        # longer than n_out = 7, its peak beyond n_out
             (0, 1, 1001),
             (0, 2, 16002),       # end > n_total
             (1, 2000, 2300),     # all zeros
             (1, 1234, 1234),     # empty
             (1, 3000, 2000),     # end before start: empty
             (2, 3001, 4001),     # holds the NaN, ends at the last sample of the last recording
             (2, -50, 120),       # start < 0
             (2, 5000, 6000),     # both beyond n_total: empty
             (-1, 0, 1000), (R, 0, 1000)]  # recording index -1 and R
    return x, spans


@pytest.mark.parametrize("normalize_to", [0.0, 0.5, 1e-3])
@pytest.mark.parametrize("n_out", [16000, 7])
def test_cut_f32_matches_the_numpy_cut(ctx, cut_case, n_out, normalize_to):
    x, spans = cut_case
    U = len(spans)
    want_clips, want_peaks = cut_f32_ref(x, spans, normalize_to, n_out)
    assert want_peaks.tolist().count(-1.0) == 2 and want_peaks.tolist().count(0.0) == 4 and want_peaks[0] == np.float32(0.97)
    assert np.isnan(want_clips[6]).sum() == (1 if n_out == 16000 else 0) and want_peaks[6] > 0, "a NaN must not raise the peak"
    if n_out == 7:
        assert np.abs(x[0, :7]).max() < 0.9, "the peak lies beyond n_out"
    d = torch.from_numpy(x).to(DEV)  # sized exactly: a read past the last sample is a read out of the allocation
    span = torch.tensor(spans, dtype=torch.int32, device=DEV)
    clips = torch.full((U + 1, n_out), -77.0, device=DEV)
    peak = torch.full((U + 1,), -77.0, device=DEV)
    ctx.cut_f32(d, span, clips[:U], normalize_to, peak[:U])
    clips, peak = clips.cpu().numpy(), peak.cpu().numpy()
    assert (clips[U] == -77.0).all() and peak[U] == -77.0, "written beyond [U]"
    assert np.array_equal(peak[:U], want_peaks, equal_nan=True)
    bad = [u for u in range(U) if not np.array_equal(clips[u], want_clips[u], equal_nan=True)]
    assert not bad, f"spans {bad} differ from the NumPy cut"
    if normalize_to == 0.0:  # a bitwise copy: the NaN's payload and the sign of -0.0 included
        assert np.array_equal(u32(clips[:U]), u32(want_clips))
    again = torch.full((U, n_out), -77.0, device=DEV)  # without d_peak: the same clips
    ctx.cut_f32(d, span, again, normalize_to)
    assert np.array_equal(again.cpu().numpy(), want_clips, equal_nan=True)


def test_cut_f32_argument_errors(ctx):
    x = torch.zeros((1, 64), device=DEV)
    span = torch.tensor([[0, 0, 64]], dtype=torch.int32, device=DEV)
    clips = torch.full((1, 8), float("nan"), device=DEV)

    def rc(wav=x, R=1, n=64, sp=span, U=1, norm=0.5, out=clips, n_out=8):
        p = lambda t: t.data_ptr() if t is not None else None
        return ctx._lib.kws_cut_f32(ctx._h, p(wav), R, n, p(sp), U, norm, p(out), n_out, None)

    for kw in (dict(wav=None), dict(sp=None), dict(out=None), dict(U=0), dict(R=0), dict(n=0), dict(n_out=0), dict(norm=-0.5),
               dict(norm=float("inf")), dict(norm=float("nan"))):
        assert rc(**kw) == _native.KWS_EINVAL, kw
    torch.cuda.synchronize()
    assert torch.isnan(clips).all(), "a refused call wrote a clip"
    assert rc() == _native.KWS_OK


# ---- 7. KeywordSpotter ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spotter(e2e_golden):
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=C)
    model.load_state_dict(sref.state_from_blob(e2e_golden["he.blob"]))
    return KeywordSpotter(model)


@pytest.fixture(scope="module")
def recipe():
    recs = gref.recipe_recordings()
    c0 = gref.oracle_frames(recs)[..., 0]
    kinds = [gref.frame_kinds(b, c0.shape[1]) for _, b in gref.RECIPES]
    return recs, gref.recipe_threshold(c0, kinds)


def _same_scan(a, b):
    assert np.array_equal(a.labels, b.labels) and np.array_equal(u32(a.logits), u32(b.logits))
    assert np.array_equal(a.window_start_s, b.window_start_s) and a.events == b.events


def _same_utterances(a, b, peaks=True):
    assert [len(g) for g in a] == [len(g) for g in b]
    for ua, ub in zip([u for g in a for u in g], [u for g in b for u in g]):
        assert (ua.recording, ua.start_s, ua.end_s, ua.open_s, ua.close_s, ua.reason, ua.label, ua.word) == \
            (ub.recording, ub.start_s, ub.end_s, ub.open_s, ub.close_s, ub.reason, ub.label, ub.word)
        assert np.array_equal(u32(ua.logits), u32(ub.logits))
        if peaks:
            assert ua.peak == ub.peak


def test_spotter_scan_f32_and_segment_f32_on_the_grid(spotter, recipe):
    recs, threshold = recipe
    x = unit(recs)
    # the top smoothed posterior of 12 classes is at least 1 / 12 > 0.05 and no class is excluded: every window is a candidate
    kw = dict(hop_frames=3, smooth_window=4, threshold=0.05, refractory=7, first_keyword=0)
    want = spotter.scan(recs, **kw)
    assert want.events is not None and sum(len(e) for e in want.events) > 0, "the fixture: events fire"
    _same_scan(spotter.scan_f32(x, **kw), want)
    _same_scan(spotter.scan_f32(torch.from_numpy(x).to(DEV), **kw), want)  # a device tensor
    _same_scan(spotter.scan_f32(x[0], **kw), spotter.scan(recs[0], **kw))   # [n]
    seg_i = spotter.segment(recs, threshold, on_window=3, off_window=5, normalize=0)
    seg_f = spotter.segment_f32(x, threshold, on_window=3, off_window=5, normalize=0)
    assert sum(len(g) for g in seg_i) >= 3
    _same_utterances(seg_f, seg_i, peaks=False)
    for uf, ui in zip([u for g in seg_f for u in g], [u for g in seg_i for u in g]):
        assert isinstance(uf.peak, float) and uf.peak == ui.peak / 32768.0, "the peak is in full-scale units"


def test_spotter_segment_f32_normalises_like_the_numpy_cut(ctx, spotter, recipe):
    recs, threshold = recipe
    x = unit(recs) * np.float32(0.37)  # off the grid
    got = spotter.segment_f32(x, threshold - 2.0, on_window=3, off_window=5, normalize=16384)
    flat = [u for g in got for u in g]
    assert len(flat) >= 3
    spans = [(u.recording, int(round(u.start_s * 16000)), int(round(u.end_s * 16000))) for u in flat]
    clips, peaks = cut_f32_ref(x, spans, 0.5, 16000)
    logits = torch.full((len(flat), C), float("nan"), device=DEV)
    labels = torch.full((len(flat),), -1, dtype=torch.int32, device=DEV)
    ctx.infer_f32(torch.from_numpy(clips).to(DEV), logits, labels)
    logits, labels = logits.cpu().numpy(), labels.cpu().numpy()
    for i, u in enumerate(flat):
        assert np.array_equal(u32(u.logits), u32(logits[i])) and u.label == labels[i] and u.peak == float(peaks[i])


def test_spotter_batches_equal_the_single_recording_methods(spotter, recipe):
    recs, threshold = recipe
    x = unit(recs) * np.float32(0.81)
    members = [x[0], x[1, :40001], x[0, 3000:12000], x[1, 100:35333]]  # the third is shorter than a window
    kw = dict(hop_frames=2, smooth_window=3, threshold=0.05, refractory=10, first_keyword=0)  # every window is a candidate
    got = spotter.scan_batch_f32(members, **kw)
    assert len(got) == 4 and got[2].labels.shape == (1, 0) and len(got[0].events[0]) > 0
    for r in (0, 1, 3):
        _same_scan(got[r], spotter.scan_f32(members[r], **kw))
    skw = dict(on_window=3, off_window=5, normalize=16384)
    seg = spotter.segment_batch_f32(members, threshold - 1.0, **skw)
    assert sum(len(g) for g in seg) >= 3
    for r, m in enumerate(members):
        alone = spotter.segment_f32(m, threshold - 1.0, **skw)[0]
        for u in alone:
            u.recording = r
        _same_utterances([seg[r]], [alone])


def _write_wav24(path, x, rate):
    v = np.round(np.asarray(x, np.float64) * 8388608.0).clip(-8388608, 8388607).astype("<i4")
    with wave.open(path, "wb") as w:
        w.setnchannels(1), w.setsampwidth(3), w.setframerate(rate)
        w.writeframes(v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes())


def _write_wav_float(path, x, rate):
    data = np.asarray(x, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
                + b"data" + struct.pack("<I", len(data)) + data)


def test_spotter_files_decode_any(ctx, spotter, recipe, tmp_path):
    from kws.common.errors import AudioProcessingError
    from kws.libs.audio_processor import read_wav

    recs, threshold = recipe
    x = unit(recs[0]) * np.float32(0.6)
    p24, pf48, p16 = str(tmp_path / "a24.wav"), str(tmp_path / "f48.wav"), str(tmp_path / "i16.wav")
    _write_wav24(p24, x, 16000)
    rng = np.random.default_rng(9)
    y48 = (0.2 * np.sin(2 * np.pi * 440.0 * np.arange(96000) / 48000.0) + rng.normal(0, 0.02, 96000)).astype(np.float32)
    _write_wav_float(pf48, y48, 48000)
    with wave.open(p16, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(recs[1].astype("<i2").tobytes())
    # 24-bit at the configured rate: the float path on read_wav's samples
    dec, rate = read_wav(p24)
    assert dec.dtype == np.float32 and rate == 16000 and not np.array_equal(dec, np.round(dec * 32768) / 32768), "24 bits are not on the int16 grid"
    _same_scan(spotter.scan_file(p24, decode="any", hop_frames=5), spotter.scan_f32(dec, hop_frames=5))
    _same_utterances([spotter.segment_file(p24, decode="any", threshold=threshold - 4.0, on_window=3, off_window=5)],
                     spotter.segment_f32(dec, threshold - 4.0, on_window=3, off_window=5))
    # float32 at 48 kHz: resampled on the device in float32
    dec48, rate48 = read_wav(pf48)
    assert dec48.dtype == np.float32 and rate48 == 48000 and np.array_equal(dec48, y48)
    n_out = _native.host_resample_len(96000, 48000, 16000)
    y16 = torch.empty((1, n_out), dtype=torch.float32, device=DEV)
    ctx.resample_f32(torch.from_numpy(y48[None]).to(DEV), 48000, 16000, y16)
    torch.cuda.synchronize()
    _same_scan(spotter.scan_file(pf48, decode="any", resample=True, hop_frames=5), spotter.scan_f32(y16, hop_frames=5))
    with pytest.raises(AudioProcessingError, match="sample rate 48000"):
        spotter.scan_file(pf48, decode="any")
    # the plural methods: one pass per sample type, results in input order
    many = spotter.scan_files([p24, p16, pf48], decode="any", resample=True, hop_frames=5)
    _same_scan(many[0], spotter.scan_f32(dec, hop_frames=5))
    _same_scan(many[1], spotter.scan(recs[1], hop_frames=5))
    _same_scan(many[2], spotter.scan_f32(y16, hop_frames=5))
    segs = spotter.segment_files([p16, p24], decode="any", threshold=threshold - 4.0, on_window=3, off_window=5)
    assert [u.recording for u in segs[1]] == [1] * len(segs[1]) and len(segs[1]) > 0
    _same_utterances([segs[0]], spotter.segment(recs[1], threshold - 4.0, on_window=3, off_window=5))
    # the default decode still raises as before
    with pytest.raises(AudioProcessingError):
        spotter.scan_file(p24)
    with pytest.raises(AudioProcessingError, match="there is no float32 scan"):
        spotter.scan_file(pf48, resample=True)
    with pytest.raises(AudioProcessingError, match="int16 only"):
        spotter.segment_file(pf48, resample=True)
