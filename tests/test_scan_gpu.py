"""Scanning long recordings on the GPU (kws_scan_i16, kws_scan_detect_f32, KeywordSpotter.scan).

Every output buffer is prefilled with NaN / -1 and over-allocated by one row: every expected element must be written and the extra
row must not be.  Frames are held bit for bit against kws_mfcc_i16 on a context whose clips are as long as the recording, windows
bit for bit against kws_forward_f32 on the same 99 rows gathered into a contiguous batch, and the whole against the CPU oracle at
the project's standing gates (frames 1e-4, logits 1e-4)."""
import itertools
import wave

import numpy as np
import pytest
import torch

import _scan_ref as ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
GATE = 1e-4


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


def _scan(ctx, pcm, hop, keep_frames=True):
    """Run kws_scan_i16 into prefilled, over-allocated buffers; returns device tensors (logits [R, W, C], labels [R, W], frames
    [R, F, 10] or None) after checking that all of them and nothing beyond was written."""
    R, n = pcm.shape
    F, W = ref.scan_shape(n, hop)
    x = torch.from_numpy(np.ascontiguousarray(pcm)).to(DEV)
    logits = torch.full((R + 1, W, C), float("nan"), device=DEV)
    labels = torch.full((R + 1, W), -1, dtype=torch.int32, device=DEV)
    feat = torch.full((R + 1, F, ref.N_CEP), float("nan"), device=DEV) if keep_frames else None
    ctx.scan_i16(x, hop, logits[:R], labels[:R], feat[:R] if keep_frames else None)
    torch.cuda.synchronize()
    assert torch.isfinite(logits[:R]).all(), "a window's logits were not written"
    assert torch.isnan(logits[R]).all(), "logits were written beyond [R, W, C]"
    assert ((labels[:R] >= 0) & (labels[:R] < C)).all() and (labels[R] == -1).all()
    if keep_frames:
        assert torch.isfinite(feat[:R]).all(), "a frame was not written"
        assert torch.isnan(feat[R]).all(), "frames were written beyond [R, F_total, numcep]"
    return logits[:R], labels[:R], (feat[:R] if keep_frames else None)


def _windows(feat, hop):
    """[R, F, 10] -> contiguous [R * W, 1, 99, 10]: the gather route."""
    w = feat.unfold(1, ref.T_WIN, hop).permute(0, 1, 3, 2)  # [R, W, 99, 10]
    return w.reshape(-1, 1, ref.T_WIN, ref.N_CEP).contiguous()


# ---- 1. one second is a clip -----------------------------------------------------------------------------------------
def test_a_one_second_recording_is_kws_infer_i16(ctx, clips):
    pcm = clips[[3, 8, 20, 33, 41]]
    logits, labels, _ = _scan(ctx, pcm, 1)
    assert logits.shape == (5, 1, C)
    want_logits = torch.full((5, C), float("nan"), device=DEV)
    want_labels = torch.full((5,), -1, dtype=torch.int32, device=DEV)
    ctx.infer_i16(torch.from_numpy(pcm).to(DEV), want_logits, want_labels)
    torch.cuda.synchronize()
    assert torch.equal(logits[:, 0], want_logits)
    assert torch.equal(labels[:, 0], want_labels)
    # without d_feat_out the frames live in the context: same results
    logits2, labels2, _ = _scan(ctx, pcm, 1, keep_frames=False)
    assert torch.equal(logits2, logits) and torch.equal(labels2, labels)


# ---- 2. frames are one long clip -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_clip_ctx():
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def _frames_like_one_clip(ctx, other, pcm, math):
    R, n = pcm.shape
    F, _ = ref.scan_shape(n, 1)
    ctx.set_frontend_math(math)
    other.set_frontend(n_samples=n)
    other.set_frontend_math(math)
    try:
        before, before_other = ctx.frontend_stats(), other.frontend_stats()
        _, _, feat = _scan(ctx, pcm, 1)
        want = torch.full((R, 1, F, ref.N_CEP), float("nan"), device=DEV)
        other.mfcc_i16(torch.from_numpy(pcm).to(DEV), want)
        torch.cuda.synchronize()
        assert torch.equal(feat, want[:, 0]), f"{(feat != want[:, 0]).any(dim=2).sum().item()} frames differ from kws_mfcc_i16"
        after, after_other = ctx.frontend_stats(), other.frontend_stats()
        # frames through the float32 front end: R * F_total, as kws_mfcc_i16 counts them (the float64 front end counts none)
        assert after[0] - before[0] == after_other[0] - before_other[0] == (R * F if math == _native.FE_F32 else 0)
        assert after[1] - before[1] == after_other[1] - before_other[1]  # the same frames were redone in float64
        assert after[2] == after_other[2]
        assert ctx.frontend_shape() == (ref.T_WIN, ref.N_CEP), "the context's own clip length must not change"
        return after[1] - before[1]
    finally:
        ctx.set_frontend_math(_native.FE_F32)


@pytest.mark.parametrize("math", [_native.FE_F32, _native.FE_F64], ids=["default", "f64"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("n_total", [16081, 21973, 48000])
def test_frames_are_kws_mfcc_i16_of_one_long_clip(ctx, long_clip_ctx, clips, n_total, R, math):
    _frames_like_one_clip(ctx, long_clip_ctx, ref.mixed_recordings(R, n_total, clips, seed=n_total + R), math)


def test_a_tone_flags_every_frame_and_the_worklist_holds_them(ctx, long_clip_ctx):
    """The refinement worklist must scale with R * F_total, not with R one-second clips (50 pairs each).  Tones near the top of
    the band flag every frame: pre-emphasis and the rectangular window leave the lowest mel band far below the peak bin.  The
    float64 oracle puts log(largest bin power / weakest mel band) at 12.7 (7 000 Hz) and 17.9 (7 900 Hz) on every frame, against
    the flag's threshold of 10.2; a frame more than 1 above it by the oracle must be listed by the float32 measurement too."""
    from oracle import psf_mfcc as o_mfcc

    t = np.arange(48000) / 16000.0
    pcm = np.stack([np.round(20000 * np.sin(2 * np.pi * f * t)).astype(np.int16) for f in (7000.0, 7900.0)])
    must = 0
    for rec in pcm:
        sig = o_mfcc.pcm16_to_float(rec)
        band, _ = o_mfcc.fbank(sig, o_mfcc.FrontendSpec(n_samples=48000))
        ps = o_mfcc.powspec(o_mfcc.framesig(o_mfcc.preemphasis(sig, 0.97), 400, 160), 512)
        must += int((np.log(ps.max(axis=1)) - np.log(band).min(axis=1) > _native.FE_REFINE_SPAN_DEFAULT + 1.0).sum())
    frames = 2 * ref.scan_shape(48000, 1)[0]
    assert must == frames == 598, "the fixture: every frame of both tones is far over the flag's threshold"
    refined = _frames_like_one_clip(ctx, long_clip_ctx, pcm, _native.FE_F32)
    assert must <= refined <= frames, f"{refined} frames of two tones were redone in float64, the oracle flags {must} of {frames}"


# ---- 3. windows are clips, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [_native.PW_SPLIT_BF16, _native.PW_PAIR_F16], ids=["bf16_triple", "f16_pair"])
@pytest.mark.parametrize("R,n_total,hop", [(1, 16081, 1), (1, 21973, 3), (2, 48000, 7), (3, 80000, 1), (1, 48000, 99), (1, 64000, 150)])
def test_windows_are_kws_forward_f32_on_the_gathered_rows(ctx, clips, R, n_total, hop, math):
    ctx.set_pointwise_math(math)
    try:
        pcm = ref.mixed_recordings(R, n_total, clips, seed=hop)
        logits, labels, feat = _scan(ctx, pcm, hop)
        x = _windows(feat, hop)
        assert x.shape[0] == R * ref.scan_shape(n_total, hop)[1]
        want_logits = torch.full((x.shape[0], C), float("nan"), device=DEV)
        want_labels = torch.full((x.shape[0],), -1, dtype=torch.int32, device=DEV)
        ctx.forward_f32(x, want_logits, want_labels)
        torch.cuda.synchronize()
        got = logits.reshape(-1, C)
        bad = (got != want_logits).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, f"{bad.numel()} windows differ from the same rows as a contiguous clip, first {bad[:5].tolist()}"
        assert torch.equal(labels.reshape(-1), want_labels)
    finally:
        ctx.set_pointwise_math(_native.PW_PAIR_F16)


def _scan_rc(c, pcm, R, n, hop, logits, label=None, feat=None):
    p = lambda t: t.data_ptr() if t is not None else None
    return c._lib.kws_scan_i16(c._h, p(pcm), R, n, hop, p(logits), p(label), p(feat))


def test_scan_scope_and_argument_errors(ctx, e2e_golden):
    pcm = torch.zeros((1, 32000), dtype=torch.int16, device=DEV)
    logits = torch.full((1, 101, C), float("nan"), device=DEV)
    ctx.set_pointwise_math(_native.PW_F32)
    try:
        assert _scan_rc(ctx, pcm, 1, 32000, 1, logits) == _native.KWS_EUNSUPPORTED
    finally:
        ctx.set_pointwise_math(_native.PW_PAIR_F16)
    other = _native.Context(0)
    try:
        other.use_torch_stream()
        assert _scan_rc(other, pcm, 1, 32000, 1, logits) == _native.KWS_ESTATE  # no model
        other.load_dscnn(e2e_golden["he.blob"], C)
        other.set_frontend(n_samples=24000)  # 149 x 10 windows: not the fused kernel's map
        assert _scan_rc(other, pcm, 1, 32000, 1, logits) == _native.KWS_EUNSUPPORTED
        other.set_frontend(numcep=13)
        assert _scan_rc(other, pcm, 1, 32000, 1, logits) == _native.KWS_EUNSUPPORTED
    finally:
        other.close()
    assert _scan_rc(ctx, None, 1, 32000, 1, logits) == _native.KWS_EINVAL
    assert _scan_rc(ctx, pcm, 1, 32000, 1, None) == _native.KWS_EINVAL
    assert _scan_rc(ctx, pcm, 0, 32000, 1, logits) == _native.KWS_EINVAL
    assert _scan_rc(ctx, pcm, 1, 32000, 0, logits) == _native.KWS_EINVAL
    assert _scan_rc(ctx, pcm, 1, 15840, 1, logits) == _native.KWS_EINVAL  # 98 frames: shorter than a window
    torch.cuda.synchronize()
    assert torch.isnan(logits).all(), "a refused call wrote logits"


# ---- 4. against the oracle -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_expectation(e2e_golden):
    recs = ref.oracle_recordings(e2e_golden["clips"])
    frames, logits = ref.oracle_scan(recs, e2e_golden["he.blob"], 5)
    return recs, frames, logits


def test_scan_against_the_oracle(ctx, oracle_expectation):
    recs, want_frames, want_logits = oracle_expectation
    assert recs.shape == (2, 48053) and want_frames.shape == (2, 299, 10) and want_logits.shape == (2, 41, C)
    # the expectation itself: clear top-2 margins (10 x the gate at the very least) and windows of several classes
    top = np.sort(want_logits, axis=2)
    margin = (top[..., -1] - top[..., -2]).min(axis=1)
    assert abs(margin[0] - 7.9e-3) < 1e-4 and abs(margin[1] - 2.8e-2) < 1e-3 and margin.min() > 10 * GATE, margin
    want_labels = want_logits.argmax(axis=2)
    assert len(np.unique(want_labels[0])) == 5, np.unique(want_labels[0])
    logits, labels, feat = _scan(ctx, recs, 5)
    err_f = np.abs(feat.cpu().numpy().astype(np.float64) - want_frames).max()
    err_l = np.abs(logits.cpu().numpy().astype(np.float64) - want_logits).max()
    print(f"[scan-oracle] frames max err {err_f:.3e}, logits max err {err_l:.3e} (gates {GATE:.0e})")
    assert err_f <= GATE, f"a frame is {err_f:.3e} from psf's float64 MFCC of the recording as one clip"
    assert err_l <= GATE, f"a window's logits are {err_l:.3e} from the reference forward"
    np.testing.assert_array_equal(labels.cpu().numpy(), want_labels)


# ---- 5. decisions ----------------------------------------------------------------------------------------------------
def _detect(ctx, logits, S, first_keyword, threshold, refractory, max_events, want_smoothed=True):
    R, W, Cn = logits.shape
    smoothed = torch.full((R + 1, W, Cn), float("nan"), device=DEV) if want_smoothed else None
    count = torch.full((R + 1,), -7, dtype=torch.int32, device=DEV)
    ev_w = torch.full((R + 1, max_events), -1, dtype=torch.int32, device=DEV)
    ev_k = torch.full((R + 1, max_events), -1, dtype=torch.int32, device=DEV)
    ev_s = torch.full((R + 1, max_events), float("nan"), device=DEV)
    ctx.scan_detect_f32(logits, S, first_keyword, threshold, refractory, count[:R], ev_w[:R], ev_k[:R], ev_s[:R], max_events,
                        smoothed[:R] if want_smoothed else None)
    torch.cuda.synchronize()
    assert count[R] == -7 and (ev_w[R] == -1).all() and (ev_k[R] == -1).all() and torch.isnan(ev_s[R]).all()
    if want_smoothed:
        assert torch.isnan(smoothed[R]).all()
    return (count[:R].cpu().numpy(), ev_w[:R].cpu().numpy(), ev_k[:R].cpu().numpy(), ev_s[:R].cpu().numpy(),
            smoothed[:R].cpu().numpy() if want_smoothed else None)


@pytest.mark.parametrize("S", [1, 7, 256])
@pytest.mark.parametrize("Cn", [2, 12, 64])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 200])
def test_decisions_match_the_float64_restatement(ctx, W, Cn, S):
    R, threshold, tol = 3, 0.5, ref.tol_smooth(S)
    z = ref.detect_logits(W, Cn, ref.DETECT_SEEDS[(W, Cn)])
    s = ref.smooth_ref(z, S)
    m2, mt = ref.margins(s, threshold)
    assert m2 > 2 * tol and mt > 2 * tol, f"the restatement's own decisions are within 2 tol of a boundary: {m2:.2e}, {mt:.2e}"
    zd = torch.from_numpy(z).to(DEV)
    worst = 0.0
    for refractory, first_keyword, max_events in itertools.product([1, 5, 1000], [0, 2], [0, 1, 3, 1024]):
        want = ref.events_ref(s, first_keyword, threshold, refractory)
        count, ev_w, ev_k, ev_s, smoothed = _detect(ctx, zd, S, first_keyword, threshold, refractory, max_events)
        what = f"refractory {refractory}, first_keyword {first_keyword}, max_events {max_events}"
        np.testing.assert_array_equal(count, [len(e) for e in want], err_msg=what)  # exact, also beyond max_events
        err = np.abs(smoothed.astype(np.float64) - s).max()
        worst = max(worst, err)
        assert err <= tol, f"{what}: smoothed posteriors {err:.2e} from the restatement (tol {tol:.2e})"
        for r in range(R):
            n = min(len(want[r]), max_events)
            np.testing.assert_array_equal(ev_w[r, :n], [e[0] for e in want[r][:n]], err_msg=what)
            np.testing.assert_array_equal(ev_k[r, :n], [e[1] for e in want[r][:n]], err_msg=what)
            if n:
                assert np.abs(ev_s[r, :n].astype(np.float64) - np.array([e[2] for e in want[r][:n]])).max() <= tol, what
            assert (ev_w[r, n:] == -1).all() and (ev_k[r, n:] == -1).all() and np.isnan(ev_s[r, n:]).all(), f"{what}: a slot beyond the count was written"
    print(f"[scan-detect] W {W} C {Cn} S {S}: smoothed worst err / tol {worst / tol:.4f}")


def test_decisions_ties_determinism_and_null_smoothed(ctx):
    # two equal logits: the lower index wins, in the smoothed argmax as in the labels
    z = torch.zeros((1, 5, 6), device=DEV)
    z[0, :, 4] = 3.0
    z[0, :, 2] = 3.0
    count, ev_w, ev_k, ev_s, _ = _detect(ctx, z, 3, 2, 0.4, 1, 8)
    assert count[0] == 5 and (ev_k[0, :5] == 2).all() and (ev_w[0, :5] == np.arange(5)).all()
    # two calls give the same bits; a NULL d_smoothed changes nothing else
    zr = torch.from_numpy(ref.detect_logits(200, 12, [5, 6, 7])).to(DEV)
    a = _detect(ctx, zr, 7, 0, 0.5, 5, 64)
    b = _detect(ctx, zr, 7, 0, 0.5, 5, 64)
    c = _detect(ctx, zr, 7, 0, 0.5, 5, 64, want_smoothed=False)
    for x, y, v in zip(a, b, c[:4] + (a[4],)):
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, v, equal_nan=True)


def test_decisions_argument_errors(ctx):
    R, W = 2, 10
    z = torch.zeros((R, W, 65), device=DEV)
    count = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    ev_i = torch.full((R, 4), -1, dtype=torch.int32, device=DEV)
    ev_s = torch.full((R, 4), float("nan"), device=DEV)

    def rc(logits=z, Cn=12, S=1, fk=0, refractory=1, max_events=4, cnt=count, evw=ev_i, evk=ev_i, evs=ev_s):
        p = lambda t: t.data_ptr() if t is not None else None
        return ctx._lib.kws_scan_detect_f32(ctx._h, p(logits), R, W, Cn, S, fk, 0.5, refractory, None, p(evw), p(evk), p(evs), max_events, p(cnt))

    assert rc() == _native.KWS_OK
    assert rc(max_events=0, evw=None, evk=None, evs=None) == _native.KWS_OK
    for bad in (dict(logits=None), dict(cnt=None), dict(evw=None), dict(evk=None), dict(evs=None), dict(Cn=65), dict(Cn=0), dict(S=0),
                dict(S=257), dict(refractory=0), dict(max_events=-1)):
        assert rc(**bad) == _native.KWS_EINVAL, bad


# ---- 6. the Python surface -------------------------------------------------------------------------------------------
def test_keyword_spotter_scan(ctx, e2e_golden, oracle_expectation, tmp_path):
    from kws.common.errors import ModelError
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=C)
    model.load_state_dict(ref.state_from_blob(e2e_golden["he.blob"]))
    sp = KeywordSpotter(model)
    rec = oracle_expectation[0][0]
    res = sp.scan(rec, hop_frames=5, smooth_window=3, threshold=0.15, refractory=4, first_keyword=2, max_events=16)
    logits, labels, _ = _scan(ctx, rec[None], 5)
    assert res.logits.shape == (1, 41, C) and res.labels.shape == (1, 41) and res.window_start_s.shape == (41,)
    np.testing.assert_array_equal(res.logits, logits.cpu().numpy())
    np.testing.assert_array_equal(res.labels, labels.cpu().numpy())
    assert res.window_start_s[1] - res.window_start_s[0] == 5 * 0.01
    count, ev_w, ev_k, ev_s, _ = _detect(ctx, logits.contiguous(), 3, 2, 0.15, 4, 16)
    n = int(count[0])
    assert 0 < n <= 16 and len(res.events) == 1 and len(res.events[0]) == n
    for i, (time_s, index, word, score) in enumerate(res.events[0]):
        end = min(ev_w[0, i] * 5 * 160 + 98 * 160 + 400, 48053) / 16000.0  # the window's end
        assert (time_s, index, word, score) == (end, ev_k[0, i], sp.words[ev_k[0, i]], ev_s[0, i])
    assert sp.scan(rec, hop_frames=5).events is None
    # a device tensor, two recordings
    both = sp.scan(torch.from_numpy(oracle_expectation[0]).to(DEV), hop_frames=5)
    np.testing.assert_array_equal(both.logits[0], res.logits[0])
    with pytest.raises(ModelError, match="shorter than one window"):
        sp.scan(np.zeros(8000, np.int16))
    path = str(tmp_path / "rec.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(rec.astype("<i2").tobytes())
    from_file = sp.scan_file(path, hop_frames=5, smooth_window=3, threshold=0.15, refractory=4, max_events=16)
    np.testing.assert_array_equal(from_file.logits, res.logits)
    np.testing.assert_array_equal(from_file.labels, res.labels)
    assert from_file.events == res.events
