"""Utterances from recordings on the GPU (kws_frames_i16, kws_segment_f32, kws_cut_i16, KeywordSpotter.segment).

Every output buffer is prefilled with a sentinel and over-allocated by one row: every expected element must be written and
nothing beyond.  The frames are held bit for bit against kws_scan_i16 and kws_mfcc_i16, the walk and the cut exactly against their
NumPy restatements (tests/_segment_ref.py), and the whole against the CPU oracle at the project's standing gate (logits 1e-4).

Two refusals the header names cannot be reached through the C ABI and are therefore not exercised: kws_create configures a front
end (so KWS_ESTATE for "no front end" never occurs on a live context) and kws_set_frontend always appends the log energy (so
KWS_EUNSUPPORTED for "no log energy in cepstrum 0" never occurs either)."""
import itertools
import wave

import numpy as np
import pytest
import torch

import _segment_ref as ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
GATE = 1e-4
SENTINEL = -77


@pytest.fixture(scope="module")
def ctx(e2e_golden):
    c = _native.Context(0)
    c.use_torch_stream()
    c.load_dscnn(e2e_golden["he.blob"], C)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare_ctx():
    """A context with a front end and no model."""
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def _frames(c, pcm, numcep=ref.N_CEP):
    R, n = pcm.shape
    F = ref.scan_shape(n, 1)[0]
    x = torch.from_numpy(np.ascontiguousarray(pcm)).to(DEV)
    feat = torch.full((R + 1, F, numcep), float("nan"), device=DEV)
    c.frames_i16(x, feat[:R])
    torch.cuda.synchronize()
    assert torch.isfinite(feat[:R]).all(), "a frame was not written"
    assert torch.isnan(feat[R]).all(), "frames were written beyond [R, F_total, numcep]"
    return feat[:R]


# ---- 1. frames -------------------------------------------------------------------------------------------------------
def test_frames_are_the_scan_s_frames(ctx, bare_ctx, e2e_golden):
    from _scan_ref import mixed_recordings

    pcm = mixed_recordings(2, 64000, e2e_golden["clips"], seed=5)
    F, W = ref.scan_shape(64000, 7)
    x = torch.from_numpy(pcm).to(DEV)
    logits = torch.empty((2, W, C), device=DEV)
    want = torch.full((2, F, ref.N_CEP), float("nan"), device=DEV)
    ctx.scan_i16(x, 7, logits, None, want)
    got = _frames(ctx, pcm)
    assert torch.equal(got, want), f"{(got != want).any(dim=2).sum().item()} frames differ from kws_scan_i16's"
    assert torch.equal(_frames(bare_ctx, pcm), want), "a context with no model must give the same frames"


@pytest.mark.parametrize("math", [_native.FE_F32, _native.FE_F64], ids=["default", "f64"])
@pytest.mark.parametrize("n_total", [300, 401, 64000])
def test_frames_are_kws_mfcc_i16_of_one_long_clip(bare_ctx, e2e_golden, n_total, math):
    from _scan_ref import mixed_recordings

    R = 2
    pcm = mixed_recordings(R, n_total, e2e_golden["clips"], seed=n_total)
    F = ref.scan_shape(n_total, 1)[0]
    assert F == {300: 1, 401: 2, 64000: 399}[n_total]
    other = _native.Context(0)
    try:
        other.use_torch_stream()
        other.set_frontend(n_samples=n_total)
        other.set_frontend_math(math)
        bare_ctx.set_frontend_math(math)
        before, before_other = bare_ctx.frontend_stats(), other.frontend_stats()
        got = _frames(bare_ctx, pcm)
        want = torch.full((R, 1, F, ref.N_CEP), float("nan"), device=DEV)
        other.mfcc_i16(torch.from_numpy(pcm).to(DEV), want)
        torch.cuda.synchronize()
        assert torch.equal(got, want[:, 0]), f"{(got != want[:, 0]).any(dim=2).sum().item()} frames differ from kws_mfcc_i16"
        after, after_other = bare_ctx.frontend_stats(), other.frontend_stats()
        assert after[0] - before[0] == after_other[0] - before_other[0] == (R * F if math == _native.FE_F32 else 0)
        assert after[1] - before[1] == after_other[1] - before_other[1]  # the same frames were redone in float64
        # frames the last call listed: the same list under float32; the float64 front end lists none and leaves the figure alone
        assert after[2] == after_other[2] if math == _native.FE_F32 else (after[2], after_other[2]) == (before[2], before_other[2])
        assert bare_ctx.frontend_shape() == (99, ref.N_CEP), "the context's own clip length must not change"
    finally:
        bare_ctx.set_frontend_math(_native.FE_F32)
        other.close()


# ---- 2. the walk -----------------------------------------------------------------------------------------------------
def _segment(c, feat, n_total, threshold, pair, pre_roll, max_frames, max_utts):
    """Run kws_segment_f32 into prefilled, over-allocated buffers; (count [R], utt [R, max_utts, 5]) as host arrays."""
    R = feat.shape[0]
    count = torch.full((R + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    utt = torch.full((R + 1, max_utts, 5), SENTINEL, dtype=torch.int32, device=DEV)
    c.segment_f32(feat, n_total, threshold, count[:R], utt[:R] if max_utts else None, max_utts, pair[0], pair[1], pre_roll, max_frames)
    count, utt = count.cpu().numpy(), utt.cpu().numpy()
    assert count[R] == SENTINEL and (utt[R] == SENTINEL).all(), "written beyond [R]"
    return count[:R], utt[:R]


def _check_walk(count, utt, want, max_utts, what):
    np.testing.assert_array_equal(count, [len(w) for w in want], err_msg=what)  # exact, also beyond max_utts
    for r, w in enumerate(want):
        n = min(len(w), max_utts)
        np.testing.assert_array_equal(utt[r, :n], np.array(w[:n], np.int64).reshape(n, 5), err_msg=what)
        assert (utt[r, n:] == SENTINEL).all(), f"{what}: a slot at or beyond the count was written"


@pytest.fixture(scope="module")
def walk_expectation():
    """{(F, pair): (flags [3, F], {(pre_roll, max_frames): per recording the reference's utterances})}, computed once; the
    coverage the cases must have is asserted here on the reference's own answer."""
    out, got = {}, set()
    for F, pair in itertools.product(ref.WALK_FRAMES, ref.WINDOW_PAIRS):
        flags = ref.walk_flags(F, ref.walk_seeds(F, pair), pair)
        want = {}
        for pre_roll, max_frames in itertools.product(ref.WALK_PRE_ROLLS, ref.WALK_MAX_FRAMES):
            want[(pre_roll, max_frames)] = [ref.walk_ref(v, pair[0], pair[1], pre_roll, max_frames, ref.walk_n_total(F)) for v in flags]
            for utts, max_utts in itertools.product(want[(pre_roll, max_frames)], ref.WALK_MAX_UTTS):
                got |= ref.coverage_of(utts, F, max_utts, pre_roll)
        out[(F, pair)] = (flags, want)
    assert got >= ref.COVERAGE, f"the walk cases no longer cover {ref.COVERAGE - got}"
    return out


@pytest.fixture(scope="module")
def numcep_ctx():
    made = {}

    def get(numcep):
        if numcep not in made:
            c = _native.Context(0)
            c.use_torch_stream()
            c.set_frontend(numcep=numcep)
            made[numcep] = c
        return made[numcep]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("F", ref.WALK_FRAMES)
def test_walk_matches_the_reference(numcep_ctx, walk_expectation, F):
    n_total = ref.walk_n_total(F)
    for pair, numcep in itertools.product(ref.WINDOW_PAIRS, [1, 10, 13]):
        c = numcep_ctx(numcep)
        flags, want = walk_expectation[(F, pair)]
        feat = torch.from_numpy(ref.frames_from_flags(flags, numcep, seed=F + numcep)).to(DEV)
        for (pre_roll, max_frames), max_utts in itertools.product(want, ref.WALK_MAX_UTTS):
            count, utt = _segment(c, feat, n_total, 0.0, pair, pre_roll, max_frames, max_utts)
            _check_walk(count, utt, want[(pre_roll, max_frames)], max_utts,
                        f"F {F} numcep {numcep} windows {pair} pre_roll {pre_roll} max_frames {max_frames} max_utts {max_utts}")


def test_walk_threshold_is_strict_nan_is_unvoiced_and_runs_repeat(ctx):
    F, pair, threshold = 129, (3, 5), 0.25
    flags = ref.walk_flags(F, (11, 12, 13), pair)
    feat = ref.frames_from_flags(flags, ref.N_CEP, seed=1, threshold=threshold)
    voiced = np.flatnonzero(flags[0])
    feat[0, voiced[::3], 0] = threshold      # exactly the threshold: unvoiced
    feat[0, voiced[1::3], 0] = np.nan        # unvoiced
    feat[1, np.flatnonzero(flags[1] == 0)[::2], 0] = np.nan
    v = np.stack([ref.voiced_flags(f[:, 0], threshold) for f in feat])
    assert (v[0] != flags[0]).sum() >= 10 and (v[1] == flags[1]).all()
    want = [ref.walk_ref(r, pair[0], pair[1], 2, 0, ref.walk_n_total(F)) for r in v]
    assert want != [ref.walk_ref(r, pair[0], pair[1], 2, 0, ref.walk_n_total(F)) for r in flags], "the edge values must matter"
    d = torch.from_numpy(feat).to(DEV)
    a = _segment(ctx, d, ref.walk_n_total(F), threshold, pair, 2, 0, 64)
    _check_walk(a[0], a[1], want, 64, "threshold / NaN")
    b = _segment(ctx, d, ref.walk_n_total(F), threshold, pair, 2, 0, 64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two runs must give the same bits"


# ---- 3. the cut ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cut_case():
    """R = 3 recordings of 4001 samples (rows not 16-byte aligned) and the spans of the test."""
    R, n = 3, 4001
    rng = np.random.default_rng(21)
    pcm = np.clip(np.round(rng.normal(0, 2500, (R, n))), -32767, 32767).astype(np.int16)
    pcm[0, 3000] = 32767        # the first recording's peak, beyond n_out = 1000 of a span from 0
    pcm[1, 700] = -32768        # |-32768| = 32768
    pcm[1, 2000:2300] = 0       # an all-zero span
    pcm[2, 3500:3600] = rng.integers(-1, 2, 100)
    pcm[2, 3550] = 1            # a span whose peak is 1
    spans = [(0, 0, 4001),      # even start, longer than both n_out, peak beyond n_out = 1000
             (0, 1, 1001),      # odd start, len == 1000
             (0, 2, 16002),     # end beyond n_total
             (1, 7, 900),       # odd start, len < 1000, holds -32768
             (1, 2000, 2300),   # all zeros
             (1, 1234, 1234),   # len == 0
             (1, 3000, 2000),   # end before start: empty
             (2, 3001, 4001),   # ends at the last sample of the last recording
             (2, 3500, 3600),   # peak 1
             (2, -50, 120),     # start below 0
             (2, 5000, 6000),   # both beyond n_total: empty
             (-1, 0, 1000), (R, 0, 1000),  # recording index out of range
             (0, 2, 1002)]      # even start, len == 1000
    return pcm, spans


@pytest.mark.parametrize("normalize_to", [0, 16384, 32767])
@pytest.mark.parametrize("n_out", [1000, 16000])
def test_cut_matches_the_numpy_cut(bare_ctx, cut_case, n_out, normalize_to):
    pcm, spans = cut_case
    U = len(spans)
    want_clips, want_peaks = ref.cut_ref(pcm, spans, normalize_to, n_out)
    # the cases themselves
    lens = [max(0, min(max(e, 0), 4001) - min(max(s, 0), 4001)) for _, s, e in spans]
    assert {0, 1000} <= set(lens) and min(l for l in lens if l) < 1000 and max(lens) > 1000
    assert want_peaks.tolist().count(-1) == 2 and 32768 in want_peaks and 1 in want_peaks and 0 in want_peaks
    if n_out == 1000:
        assert want_peaks[0] == 32767 and np.abs(pcm[0, :1000].astype(np.int64)).max() < 32767, "the peak lies beyond n_out"
    if normalize_to == 32767:
        assert np.abs(want_clips[8].astype(np.int64)).max() == 32767, "a peak of 1 is scaled to full scale"
    x = torch.from_numpy(pcm).to(DEV)  # sized exactly: a read past the last sample is a read out of the allocation
    span = torch.tensor(spans, dtype=torch.int32, device=DEV)
    clips = torch.full((U + 1, n_out), SENTINEL, dtype=torch.int16, device=DEV)
    peak = torch.full((U + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    bare_ctx.cut_i16(x, span, clips[:U], normalize_to, peak[:U])
    clips, peak = clips.cpu().numpy(), peak.cpu().numpy()
    assert (clips[U] == SENTINEL).all() and peak[U] == SENTINEL, "written beyond [U]"
    np.testing.assert_array_equal(peak[:U], want_peaks)
    bad = np.flatnonzero((clips[:U] != want_clips).any(axis=1))
    assert bad.size == 0, f"spans {bad.tolist()} differ from the NumPy cut"
    # without d_peak: the same clips
    again = torch.full((U, n_out), SENTINEL, dtype=torch.int16, device=DEV)
    bare_ctx.cut_i16(x, span, again, normalize_to)
    np.testing.assert_array_equal(again.cpu().numpy(), want_clips)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spotter(e2e_golden):
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=C)
    model.load_state_dict(ref.state_from_blob(e2e_golden["he.blob"]))
    return KeywordSpotter(model)


@pytest.fixture(scope="module")
def recipe():
    recs = ref.recipe_recordings()
    c0 = ref.oracle_frames(recs)[..., 0]
    kinds = [ref.frame_kinds(b, c0.shape[1]) for _, b in ref.RECIPES]
    return recs, ref.recipe_threshold(c0, kinds)


@pytest.mark.parametrize("pair", ref.E2E_PAIRS, ids=lambda p: f"{p[0]}_{p[1]}")
def test_keyword_spotter_segment(ctx, spotter, recipe, e2e_golden, pair):
    recs, threshold = recipe
    got = spotter.segment(recs, threshold, on_window=pair[0], off_window=pair[1])
    assert len(got) == 2
    # spans: the reference walk over the device's own frames
    c0 = _frames(ctx, recs)[..., 0].cpu().numpy()
    want = [ref.walk_ref(ref.voiced_flags(c, threshold), pair[0], pair[1], 60, 1000, ref.RECIPE_N) for c in c0]
    assert all(want) and [len(g) for g in got] == [len(w) for w in want]
    flat = [(r, u) for r in range(2) for u in got[r]]
    rows = [(r, w) for r in range(2) for w in want[r]]
    for (r, u), (_, (start, end, opened, closed, reason)) in zip(flat, rows):
        assert (u.recording, u.start_s, u.end_s, u.open_s, u.close_s, u.reason) == \
            (r, start / 16000.0, end / 16000.0, opened * 160 / 16000.0, closed * 160 / 16000.0, ref.REASONS[reason])
    # logits and labels: kws_infer_i16 on the NumPy-cut clips, bit for bit
    clips, peaks = ref.cut_ref(recs, [(r, w[0], w[1]) for r, w in rows], 16384, 16000)
    logits = torch.full((len(rows), C), float("nan"), device=DEV)
    labels = torch.full((len(rows),), -1, dtype=torch.int32, device=DEV)
    ctx.infer_i16(torch.from_numpy(clips).to(DEV), logits, labels)
    logits, labels = logits.cpu().numpy(), labels.cpu().numpy()
    for i, (_, u) in enumerate(flat):
        assert np.array_equal(u.logits, logits[i]) and u.label == labels[i] and u.word == spotter.words[labels[i]] and u.peak == peaks[i]
    # the CPU chain: NumPy cut -> oracle MFCC -> oracle DS-CNN
    oracle = ref.oracle_clip_logits(clips, e2e_golden["he.blob"])
    err = np.abs(logits.astype(np.float64) - oracle).max()
    print(f"[segment-oracle] windows {pair}: {len(rows)} utterances, logits max err {err:.3e} (gate {GATE:.0e})")
    assert err <= GATE
    np.testing.assert_array_equal(labels, oracle.argmax(axis=1))
    # keep_unfinished=False drops what the end of the recording closed, and nothing else
    finished = spotter.segment(recs, threshold, on_window=pair[0], off_window=pair[1], keep_unfinished=False)
    assert [[(u.open_s, u.label) for u in g] for g in finished] == \
        [[(u.open_s, u.label) for u in g if u.reason != "end_of_recording"] for g in got]


def test_segment_file_device_input_rate_and_nothing_found(spotter, recipe, tmp_path):
    from kws.common.errors import ModelError

    recs, threshold = recipe
    want = spotter.segment(recs[0], threshold, on_window=3, off_window=5)[0]
    assert len(want) == 2
    path = str(tmp_path / "rec.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(recs[0].astype("<i2").tobytes())
    from_file = spotter.segment_file(path, threshold=threshold, on_window=3, off_window=5)
    same = lambda a, b: len(a) == len(b) and all(
        (x.start_s, x.end_s, x.reason, x.label, x.peak) == (y.start_s, y.end_s, y.reason, y.label, y.peak) and np.array_equal(x.logits, y.logits)
        for x, y in zip(a, b))
    assert same(from_file, want)
    assert same(spotter.segment(torch.from_numpy(recs[0]).to(DEV), threshold, on_window=3, off_window=5)[0], want)  # a device tensor
    # silence: no utterance, nothing further launched
    assert spotter.segment(np.zeros((2, 8000), np.int16), threshold) == [[], []]
    # 48 kHz: every sample three times is a crude 48 kHz rendering; times stay in seconds of the recording
    up = spotter.segment(np.repeat(recs[0], 3), threshold, on_window=3, off_window=5, sample_rate=48000)[0]
    assert len(up) == 2
    for a, b in zip(up, want):
        assert abs(a.open_s - b.open_s) <= 0.03 and abs(a.close_s - b.close_s) <= 0.03 and a.end_s <= 4.0 + 1e-9
    with pytest.raises(ModelError):
        spotter.segment(recs[0].astype(np.float32), threshold)
    with pytest.raises(ModelError):
        spotter.segment(recs[0], threshold, on_window=6, off_window=5)


# ---- 5. error codes --------------------------------------------------------------------------------------------------
def test_argument_errors(ctx, bare_ctx):
    p = lambda t: t.data_ptr() if t is not None else None
    R, F, n = 2, 50, 8240
    pcm = torch.zeros((R, n), dtype=torch.int16, device=DEV)
    feat = torch.full((R, F, ref.N_CEP), float("nan"), device=DEV)
    count = torch.full((R,), SENTINEL, dtype=torch.int32, device=DEV)
    utt = torch.full((R, 4, 5), SENTINEL, dtype=torch.int32, device=DEV)
    lib, h = bare_ctx._lib, bare_ctx._h

    def frames(pcm_=pcm, R_=R, n_=n, out=feat):
        return lib.kws_frames_i16(h, p(pcm_), R_, n_, p(out))

    for bad in (dict(pcm_=None), dict(out=None), dict(R_=0), dict(n_=0)):
        assert frames(**bad) == _native.KWS_EINVAL, bad
    assert frames(n_=(1 << 30) + 1) == _native.KWS_EUNSUPPORTED
    assert frames(R_=1 << 13, n_=1 << 30) == _native.KWS_EUNSUPPORTED  # 2^13 * 6 710 885 frames > 2^28
    torch.cuda.synchronize()
    assert torch.isnan(feat).all(), "a refused call wrote frames"

    zeros = torch.zeros((R, F, ref.N_CEP), device=DEV)

    def segment(feat_=zeros, R_=R, F_=F, n_=n, on=3, off=5, pre=0, mf=0, utt_=utt, mu=4, cnt=count):
        return lib.kws_segment_f32(h, p(feat_), R_, F_, n_, 0.5, on, off, pre, mf, p(utt_), mu, p(cnt))

    for bad in (dict(on=0), dict(on=6), dict(off=1025, on=1025), dict(off=1025), dict(pre=-1), dict(mf=1), dict(mf=-3), dict(mu=-1),
                dict(R_=0), dict(F_=0), dict(n_=0), dict(feat_=None), dict(cnt=None), dict(utt_=None)):
        assert segment(**bad) == _native.KWS_EINVAL, bad
    assert segment(R_=1 << 14, F_=(1 << 14) + 1) == _native.KWS_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (count == SENTINEL).all() and (utt == SENTINEL).all(), "a refused call wrote results"
    assert segment(utt_=None, mu=0) == _native.KWS_OK and segment(mf=2, off=1024) == _native.KWS_OK
    torch.cuda.synchronize()
    assert (count == 0).all()

    span = torch.tensor([[0, 0, 100]], dtype=torch.int32, device=DEV)
    clips = torch.full((1, 64), SENTINEL, dtype=torch.int16, device=DEV)

    def cut(pcm_=pcm, R_=R, n_=n, span_=span, U=1, norm=16384, clips_=clips, n_out=64):
        return lib.kws_cut_i16(h, p(pcm_), R_, n_, p(span_), U, norm, p(clips_), n_out, None)

    for bad in (dict(norm=-1), dict(norm=32768), dict(U=0), dict(R_=0), dict(n_=0), dict(n_out=0), dict(pcm_=None), dict(span_=None),
                dict(clips_=None)):
        assert cut(**bad) == _native.KWS_EINVAL, bad
    torch.cuda.synchronize()
    assert (clips == SENTINEL).all(), "a refused call wrote a clip"
    assert cut() == _native.KWS_OK
    torch.cuda.synchronize()
    assert (clips == 0).all()
