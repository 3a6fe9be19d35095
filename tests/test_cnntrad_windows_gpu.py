"""cnn-trad-fpool3 over windows read in place (kws_forward_cnn_trad_windows_f32: kws_cnntrad_conv_windows_kernel + the dense kernel
in chunks), the recording entries built on it (kws_scan_cnn_trad_*, kws_scan_ragged_cnn_trad_*, kws_infer_cnn_trad_f32) and the
spotter that takes the model.

The gate: the conv kernel reads its 99 x 10 map in one place and everything after that is per clip, so logits and labels of the
windows entry are torch.equal -- no tolerance -- to kws_forward_cnn_trad_f32 on the same windows gathered into contiguous
[B, 1, 99, 10], for every window, under both arithmetics."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from kws import _native  # noqa: E402
from oracle import cnn_trad as o_ct  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PAIR, TRIPLE = _native.KWS_CT_F16_PAIR, _native.KWS_CT_BF16_TRIPLE
MATHS = [pytest.param(PAIR, id="f16_pair"), pytest.param(TRIPLE, id="bf16_triple")]
T, NF = 99, 10


def _state(C=12, seed=1):
    """As tests/test_cnntrad_forward_gpu.py::_state("random"): fan-in scaled weights, non-zero biases."""
    return o_ct.random_state(seed, num_classes=C)


_loaded = {}


@pytest.fixture(scope="module")
def ctx():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    c = _native.Context(0)
    _loaded.clear()
    yield c
    c.close()


def _load(ctx, C=12):
    if _loaded.get("C") != C:
        ctx.load_cnn_trad(o_ct.flatten_state(_state(C)), C)
        _loaded["C"] = C


def _frames(R, F, seed):
    """Synthetic frame arrays [R, F, 10]: noise whose level and sign pattern change every few rows, so windows differ in label."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, F, NF, generator=g) * 3.0
    level = torch.exp(torch.randn(R, (F + 12) // 13, 1, generator=g) * 1.5).repeat_interleave(13, dim=1)[:, :F]
    tilt = torch.randn(R, (F + 30) // 31, NF, generator=g).repeat_interleave(31, dim=1)[:, :F] * 4.0
    return (x * level + tilt * level).contiguous()


def _gather(frames, hop):
    """Every window as a contiguous clip: [R * W, 1, 99, 10], window order of the entry."""
    R, F, _ = frames.shape
    W = (F - T) // hop + 1
    idx = (torch.arange(W, device=frames.device) * hop)[:, None] + torch.arange(T, device=frames.device)[None, :]
    return frames[:, idx].reshape(R * W, 1, T, NF).contiguous(), W


def _windows(ctx, math, frames_d, hop, C, want_label=True):
    R, F, _ = frames_d.shape
    W = (F - T) // hop + 1
    logits = torch.full((R, W, C), float("nan"), device=DEV)
    label = torch.full((R, W), -1, dtype=torch.int32, device=DEV) if want_label else None
    torch.cuda.synchronize()
    ctx.set_cnn_trad_math(math)
    try:
        ctx.forward_cnn_trad_windows_f32(frames_d, hop, logits, label)
        ctx.sync()
    finally:
        ctx.set_cnn_trad_math(PAIR)
    return logits, label


def _contiguous(ctx, math, clips_d, C):
    B = clips_d.shape[0]
    logits = torch.full((B, C), float("nan"), device=DEV)
    label = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.set_cnn_trad_math(math)
    try:
        ctx.forward_cnn_trad_f32(clips_d, logits, label)
        ctx.sync()
    finally:
        ctx.set_cnn_trad_math(PAIR)
    return logits, label


def _gate(ctx, math, frames, hop, C=12, many_labels=True):
    """Logits and labels of the windows entry equal the contiguous forward on the gathered windows, all of them."""
    frames_d = frames.to(DEV).contiguous()
    clips_d, W = _gather(frames_d, hop)
    got_l, got_k = _windows(ctx, math, frames_d, hop, C)
    want_l, want_k = _contiguous(ctx, math, clips_d, C)
    assert torch.isfinite(want_l).all()
    assert torch.equal(got_l.reshape(-1, C), want_l), "window logits differ from their contiguous twins"
    assert torch.equal(got_k.reshape(-1), want_k), "window labels differ from their contiguous twins"
    return got_l, got_k, W


_pool_labels = set()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("R,F,hop,W", [(1, 99, 1, 1), (1, 100, 1, 2), (1, 104, 3, 2)])
def test_a_window_count_edges(ctx, math, R, F, hop, W):
    _load(ctx)
    _, label, got_w = _gate(ctx, math, _frames(R, F, seed=F), hop)
    assert got_w == W
    _pool_labels.update(label.reshape(-1).tolist())


@pytest.mark.parametrize("math", MATHS)
def test_b_recording_window_split(ctx, math):
    """R = 3, F = 130, hop 7: W = 5 each; window i is window i % 5 of recording i / 5."""
    _load(ctx)
    _, label, W = _gate(ctx, math, _frames(3, 130, seed=3), 7)
    assert W == 5
    _pool_labels.update(label.reshape(-1).tolist())
    # the label comparison of the gate is not vacuous: the windows of (a) and (b) take more than one label
    lone = set(_gate(ctx, math, _frames(3, 130, seed=4), 1)[1].reshape(-1).tolist())
    assert len(lone | _pool_labels) > 1, "every window of the pool got one label"


@pytest.mark.parametrize("math", MATHS)
def test_c_scale_is_per_window(ctx, math):
    """R = 1, F = 140, hop 1 (42 windows): row 120 carries a 2^10 spike, rows 0..98 are zero.  Window 0 is the zero window, windows
    1..21 hold neither the spike nor only zeros, windows 22..41 hold the spike -- a scale per recording or per chunk breaks them."""
    _load(ctx)
    frames = _frames(1, 140, seed=5)
    frames[0, :99] = 0.0
    frames[0, 120] *= 1024.0
    logits, label, W = _gate(ctx, math, frames, 1)
    assert W == 42
    assert len(set(label.reshape(-1).tolist())) > 1 or not torch.equal(logits[0, 0], logits[0, 41])


def test_d_chunk_edge(ctx):
    """R = 2 with W = chunk / 2 + 1 windows each at hop 1: the chunk boundary falls inside recording 1.  All chunk + 2 windows."""
    _load(ctx)
    n = _native.host_cnn_trad_window_chunk()
    W = n // 2 + 1
    _, label, got_w = _gate(ctx, PAIR, _frames(2, W + 98, seed=6), 1)
    assert got_w == W and label.numel() == n + 2
    assert len(set(label.reshape(-1).tolist())) > 1


@pytest.mark.parametrize("C,math", [(12, PAIR), (1, PAIR), (35, TRIPLE)])
def test_e_null_label_and_class_counts(ctx, C, math):
    _load(ctx, C)
    try:
        frames = _frames(3, 130, seed=7)
        with_l, _, _ = _gate(ctx, math, frames, 7, C=C)
        without_l, none = _windows(ctx, math, frames.to(DEV), 7, C, want_label=False)
        assert none is None and torch.equal(with_l, without_l)
    finally:
        _load(ctx, 12)


def test_f_float64_parity(ctx, capsys):
    """8 windows of shape (b) against the float64 oracle on the gathered windows: err <= max(4 e_f32, 2e-6 scale), the rule of
    tests/test_cnntrad_forward_gpu.py."""
    _load(ctx)
    state = _state()
    frames = _frames(3, 130, seed=3)
    clips, _ = _gather(frames, 7)
    clips = clips[:8]
    ref64 = o_ct.forward({k: v.double() for k, v in state.items()}, clips.double())
    ref32 = o_ct.forward(state, clips).double()
    e32 = (ref32 - ref64).abs().amax(1)
    tol = torch.maximum(4.0 * e32, 2e-6 * ref64.abs().amax(1).clamp_min(1.0))
    for math in (PAIR, TRIPLE):
        got, _ = _windows(ctx, math, frames.to(DEV), 7, 12)
        ratio = ((got.reshape(-1, 12)[:8].cpu().double() - ref64).abs().amax(1) / tol).max()
        with capsys.disabled():
            print(f"windows vs float64, math={math}: worst err/tol = {float(ratio):.3f}")
        assert float(ratio) <= 1.0


# ---- recordings ---------------------------------------------------------------------------------------------------
def _recordings(R, n, seed):
    from speechlike import speechlike_clip

    rng = np.random.default_rng(seed)
    pcm = rng.integers(-3000, 3000, size=(R, n), dtype=np.int16)
    for r in range(R):
        clip = speechlike_clip(400 + r, -20.0)
        m = min(n, clip.shape[0])
        pcm[r, :m] = np.clip(pcm[r, :m].astype(np.int32) + clip[:m], -32768, 32767).astype(np.int16)
    return torch.from_numpy(pcm)


def _scan(ctx, pcm_d, hop, f32=False, keep=True):
    R, n = pcm_d.shape
    F, W = _native.host_scan_shape(n, 400, 160, T, hop)
    logits = torch.full((R, W, 12), float("nan"), device=DEV)
    label = torch.full((R, W), -1, dtype=torch.int32, device=DEV)
    feat = torch.full((R, F, NF), float("nan"), device=DEV) if keep else None
    torch.cuda.synchronize()
    (ctx.scan_cnn_trad_f32 if f32 else ctx.scan_cnn_trad_i16)(pcm_d, hop, logits, label, feat)
    ctx.sync()
    return logits, label, feat


@pytest.mark.parametrize("hop", [1, 10])
def test_g_scan_is_frames_then_windows(ctx, hop):
    _load(ctx)
    pcm = _recordings(2, 20800, seed=11).to(DEV)  # 1.3 s
    logits, label, feat = _scan(ctx, pcm, hop)
    F, W = _native.host_scan_shape(20800, 400, 160, T, hop)
    want_feat = torch.empty((2, F, NF), device=DEV)
    torch.cuda.synchronize()
    ctx.frames_i16(pcm, want_feat)
    ctx.sync()
    assert torch.equal(feat, want_feat)
    want_l, want_k = _windows(ctx, PAIR, want_feat, hop, 12)
    assert torch.equal(logits, want_l) and torch.equal(label, want_k)
    no_feat_l, no_feat_k, _ = _scan(ctx, pcm, hop, keep=False)
    assert torch.equal(no_feat_l, logits) and torch.equal(no_feat_k, label)
    wav = (pcm.float() / 32768.0).contiguous()
    f_l, f_k, f_feat = _scan(ctx, wav, hop, f32=True)
    assert torch.equal(f_l, logits) and torch.equal(f_k, label) and torch.equal(f_feat, feat)


def test_g_infer_f32_is_infer_i16(ctx):
    _load(ctx)
    pcm = _recordings(5, 16000, seed=12).to(DEV)
    out = []
    for fn, src in ((ctx.infer_cnn_trad_i16, pcm), (ctx.infer_cnn_trad_f32, (pcm.float() / 32768.0).contiguous())):
        logits = torch.full((5, 12), float("nan"), device=DEV)
        label = torch.full((5,), -1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        fn(src, logits, label)
        ctx.sync()
        out.append((logits, label))
    assert torch.isfinite(out[0][0]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_h_ragged(ctx):
    _load(ctx)
    lens = [16000, 8000, 21920]
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        at += (n + 7) // 8 * 8
    recs = [_recordings(1, n, seed=20 + i)[0] for i, n in enumerate(lens)]
    buf = torch.zeros(at, dtype=torch.int16)
    for s, r in zip(starts, recs):
        buf[s:s + r.numel()] = r
    buf = buf.to(DEV)
    _, _, windows, win_off, W_pack = _native.host_ragged_plan(lens, 400, 160, T, 1)
    assert windows[1] == 0 and windows[0] == 1 and windows[2] > 1
    for f32 in (False, True):
        src = (buf.float() / 32768.0).contiguous() if f32 else buf
        logits = torch.full((W_pack, 12), float("nan"), device=DEV)
        label = torch.full((W_pack,), -1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        (ctx.scan_ragged_cnn_trad_f32 if f32 else ctx.scan_ragged_cnn_trad_i16)(src, starts, lens, 1, logits, label)
        ctx.sync()
        for r in (0, 2):
            alone_l, alone_k, _ = _scan(ctx, recs[r][None].to(DEV), 1)
            rows = slice(win_off[r], win_off[r] + windows[r])
            assert torch.equal(logits[rows], alone_l[0]) and torch.equal(label[rows], alone_k[0])
    # every recording shorter than a window: KWS_OK and nothing classified
    short = torch.zeros(16000, dtype=torch.int16, device=DEV)
    n_rows = max(1, int(_native.host_ragged_plan([8000, 4000], 400, 160, T, 1)[4]))
    logits = torch.full((n_rows, 12), float("nan"), device=DEV)
    torch.cuda.synchronize()
    ctx.scan_ragged_cnn_trad_i16(short, [0, 8000], [8000, 4000], 1, logits)
    ctx.sync()
    assert torch.isnan(logits).all()


# ---- errors -------------------------------------------------------------------------------------------------------
def _win_rc(c, frames, R, F, hop, logits, label=None):
    p = lambda t: t.data_ptr() if t is not None else None
    return c._lib.kws_forward_cnn_trad_windows_f32(c._h, p(frames), R, F, hop, p(logits), p(label))


def _scan_rc(c, name, pcm, R, n, hop, logits):
    p = lambda t: t.data_ptr() if t is not None else None
    return getattr(c._lib, name)(c._h, p(pcm), R, n, hop, p(logits), None, None)


def test_j_errors(ctx):
    _load(ctx)
    E = _native
    frames = torch.zeros((1, 130, NF), device=DEV)
    logits = torch.full((1, 32, 12), float("nan"), device=DEV)
    assert _win_rc(ctx, None, 1, 130, 1, logits) == E.KWS_EINVAL
    assert _win_rc(ctx, frames, 1, 130, 1, None) == E.KWS_EINVAL
    assert _win_rc(ctx, frames, 0, 130, 1, logits) == E.KWS_EINVAL
    assert _win_rc(ctx, frames, 1, 130, 0, logits) == E.KWS_EINVAL
    assert _win_rc(ctx, frames, 1, 98, 1, logits) == E.KWS_EINVAL
    assert b"kws_forward_cnn_trad_windows_f32" in ctx._lib.kws_last_error(ctx._h)
    assert _win_rc(ctx, frames, (1 << 28) // 130 + 1, 130, 1, logits) == E.KWS_EUNSUPPORTED  # more than 2^28 frames
    # (W <= F, so 2^30 windows cannot be reached below 2^28 frames: the frame limit is the one a caller can meet)
    pcm = torch.zeros((1, 32000), dtype=torch.int16, device=DEV)
    wav = torch.zeros((1, 32000), device=DEV)
    for name, src in (("kws_scan_cnn_trad_i16", pcm), ("kws_scan_cnn_trad_f32", wav)):
        assert _scan_rc(ctx, name, None, 1, 32000, 1, logits) == E.KWS_EINVAL
        assert _scan_rc(ctx, name, src, 1, 32000, 1, None) == E.KWS_EINVAL
        assert _scan_rc(ctx, name, src, 0, 32000, 1, logits) == E.KWS_EINVAL
        assert _scan_rc(ctx, name, src, 1, 32000, 0, logits) == E.KWS_EINVAL
        assert _scan_rc(ctx, name, src, 1, 15840, 1, logits) == E.KWS_EINVAL  # 98 frames
    other = _native.Context(0)
    try:
        assert _win_rc(other, frames, 1, 130, 1, logits) == E.KWS_ESTATE  # no model at all
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "e2e_golden.npz"))
        other.load_dscnn(g["he.blob"], 12)  # a DS-CNN is not a cnn-trad model
        assert _win_rc(other, frames, 1, 130, 1, logits) == E.KWS_ESTATE
        starts, lens = [0], [32000]
        for name, src in (("kws_scan_cnn_trad_i16", pcm), ("kws_scan_cnn_trad_f32", wav)):
            assert _scan_rc(other, name, src, 1, 32000, 1, logits) == E.KWS_ESTATE
        with pytest.raises(_native.ModelError):
            other.scan_ragged_cnn_trad_i16(pcm, starts, lens, 1, logits)
        with pytest.raises(_native.ModelError):
            other.infer_cnn_trad_f32(wav[:, :16000].contiguous(), logits[0, :1])
        other.load_cnn_trad(o_ct.flatten_state(_state()), 12)
        for kw in ({"n_samples": 24000}, {"numcep": 13}):  # 149 x 10, 99 x 13: not the kernels' map
            other.set_frontend(**kw)
            for name, src in (("kws_scan_cnn_trad_i16", pcm), ("kws_scan_cnn_trad_f32", wav)):
                assert _scan_rc(other, name, src, 1, 32000, 1, logits) == E.KWS_EUNSUPPORTED
            with pytest.raises(_native.ModelError):
                other.scan_ragged_cnn_trad_i16(pcm, starts, lens, 1, logits)
            other.set_frontend()
    finally:
        other.close()
    torch.cuda.synchronize()
    assert torch.isnan(logits).all(), "a refused call wrote logits"


# ---- the spotter --------------------------------------------------------------------------------------------------
def _ct_model(C=12):
    from kws.libs.models import CnnTradFpool3

    model = CnnTradFpool3(C)
    model.load_state_dict(_state(C))
    return model


def test_i_keyword_spotter_scan_and_scan_batch(ctx):
    """scan(): the logits of kws_scan_cnn_trad_i16 and the events of kws_scan_detect_f32 over them; scan_batch of two unequal
    recordings is the per-recording scan."""
    from kws.inference import KeywordSpotter, scan_window_times

    _load(ctx)
    spotter = KeywordSpotter(_ct_model())
    pcm = _recordings(1, 40000, seed=31)
    want_l, want_k, _ = _scan(ctx, pcm.to(DEV), 10)
    W = want_l.shape[1]
    rules = dict(smooth_window=3, first_keyword=0, refractory=4)
    probe = spotter.scan(pcm.numpy(), hop_frames=10)
    assert np.array_equal(probe.logits, want_l.cpu().numpy()) and np.array_equal(probe.labels, want_k.cpu().numpy())
    # a threshold some smoothed windows pass and some do not: the median of the windows' top smoothed posterior (an input of
    # the decision layer; the expectation below is the layer's own entry over the same logits)
    z = probe.logits.astype(np.float64)
    post = np.exp(z - z.max(-1, keepdims=True))
    threshold = float(np.median((post / post.sum(-1, keepdims=True)).max(-1)))
    res = spotter.scan(pcm.numpy(), hop_frames=10, threshold=threshold, **rules)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    ev_w, ev_k = (torch.zeros((1, W), dtype=torch.int32, device=DEV) for _ in range(2))
    ev_s = torch.zeros((1, W), device=DEV)
    torch.cuda.synchronize()
    ctx.scan_detect_f32(want_l, rules["smooth_window"], rules["first_keyword"], threshold, rules["refractory"], count, ev_w, ev_k, ev_s, W)
    ctx.sync()
    n = int(count[0])
    _, end_s = scan_window_times(W, 10, n_total=40000)
    want_events = [(float(end_s[int(ev_w[0, i])]), int(ev_k[0, i]), spotter.words[int(ev_k[0, i])], float(ev_s[0, i])) for i in range(n)]
    assert n >= 1 and res.events == [want_events]
    f32 = spotter.scan_f32(pcm.numpy().astype(np.float32) / np.float32(32768.0), hop_frames=10)
    assert np.array_equal(f32.logits, probe.logits)
    recs = [_recordings(1, 40000, seed=31)[0].numpy(), _recordings(1, 21920, seed=32)[0].numpy(), np.zeros(8000, np.int16)]
    batch = spotter.scan_batch(recs, hop_frames=3, threshold=threshold, **rules)
    for r in range(2):
        alone = spotter.scan(recs[r], hop_frames=3, threshold=threshold, **rules)
        assert np.array_equal(batch[r].logits, alone.logits) and np.array_equal(batch[r].labels, alone.labels)
        assert batch[r].events == alone.events
    assert batch[2].labels.shape == (1, 0)
    labels, logits = spotter.infer_pcm16(recs[0][:16000])
    (bl, bg), = list(spotter.infer_batches([recs[0][None, :16000]]))
    assert np.array_equal(logits, bg) and np.array_equal(labels, bl)
    assert np.array_equal(spotter.infer_f32(recs[0][None, :16000].astype(np.float32) / np.float32(32768.0))[1], logits)


def test_i_segment_spans_are_the_dscnn_spotters(ctx):
    """The endpointer is model-independent: the same spans as a DS-CNN spotter on the same gated audio, and the logits of
    model.infer_pcm16 on the cut clips."""
    import _segment_ref as sref
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConv

    recs = sref.recipe_recordings()
    c0 = sref.oracle_frames(recs)[..., 0]
    threshold = sref.recipe_threshold(c0, [sref.frame_kinds(b, c0.shape[1]) for _, b in sref.RECIPES])
    model = _ct_model()
    got = KeywordSpotter(model).segment(recs, threshold, on_window=3, off_window=5)
    torch.manual_seed(0)
    want = KeywordSpotter(DepthwiseSeparableConv(12)).segment(recs, threshold, on_window=3, off_window=5)
    span = lambda u: (u.recording, u.start_s, u.end_s, u.open_s, u.close_s, u.reason, u.peak)
    assert [[span(u) for u in g] for g in got] == [[span(u) for u in g] for g in want]
    flat = [u for g in got for u in g]
    assert len(flat) >= 4
    clips, _ = sref.cut_ref(recs, [(u.recording, round(u.start_s * 16000), round(u.end_s * 16000)) for u in flat], 16384, 16000)
    logits, labels = model.infer_pcm16(torch.from_numpy(clips).to(DEV))
    torch.cuda.synchronize()
    for i, u in enumerate(flat):
        assert np.array_equal(u.logits, logits[i].cpu().numpy()) and u.label == int(labels[i])


def test_i_bn_spotter_scans_with_its_fold():
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConvBN

    torch.manual_seed(3)
    bn = DepthwiseSeparableConvBN(12)
    with torch.no_grad():
        for m in [bn.bn_conv1, *bn.bn_dw, *bn.bn_pw]:
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.uniform_(0.8, 1.2)
            m.bias.normal_(0.0, 0.1)
    pcm = _recordings(1, 24000, seed=33).numpy()
    a = KeywordSpotter(bn).scan(pcm, hop_frames=5)
    b = KeywordSpotter(bn.fold()).scan(pcm, hop_frames=5)
    assert np.isfinite(a.logits).all() and np.array_equal(a.logits, b.logits) and np.array_equal(a.labels, b.labels)
