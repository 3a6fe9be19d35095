"""cnn-trad-fpool3 behind the stream ring (kws_stream_push_cnn_trad_i16: kws_stream_frame_kernel, kws_cnntrad_conv_ring_kernel, the
dense kernel) and the StreamingSpotter that takes the model.  The gate is the windows' one: a window read from the ring in place
gives the bits of kws_forward_cnn_trad_f32 on the same rows rotated into a contiguous clip."""
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
T, NF, HOP, LAG = 99, 10, 160, 3  # LAG = frames_lag: ceil(400 / 160)


def _blob(C=12, seed=1):
    return o_ct.flatten_state(o_ct.random_state(seed, num_classes=C))


def _hops(S, n, seed):
    """Seeded int16 hops [n, S, 160]: noise whose level changes from stream to stream and every 25 hops."""
    rng = np.random.default_rng(seed)
    level = np.exp(rng.normal(0.0, 1.0, size=(n // 25 + 1, S, 1))).repeat(25, axis=0)[:n]
    return torch.from_numpy(np.clip(rng.normal(0.0, 2000.0, size=(n, S, HOP)) * level, -32768, 32767).astype(np.int16))


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("S", [1, 17])
def test_k_push_is_the_forward_on_the_rotated_ring(S, math):
    """99 + K + 4 pushes, so the head wraps; after every push logits and labels equal kws_forward_cnn_trad_f32 on the ring read
    back and rotated so that the window's first row is ring row (hops + 1 - K) mod 99 -- the early pushes, whose window still
    holds zero rows, included."""
    ctx = _native.Context(0)
    try:
        ctx.load_cnn_trad(_blob(), 12)
        ctx.set_cnn_trad_math(math)
        ctx.stream_open(S)
        n = T + LAG + 4
        hops = _hops(S, n, seed=S).to(DEV)
        logits = torch.full((S, 12), float("nan"), device=DEV)
        label = torch.full((S,), -1, dtype=torch.int32, device=DEV)
        ring = torch.empty((S, T, NF), device=DEV)
        want_l = torch.empty((S, 12), device=DEV)
        want_k = torch.empty((S,), dtype=torch.int32, device=DEV)
        seen = set()
        torch.cuda.synchronize()
        for h in range(1, n + 1):
            ctx.stream_push_cnn_trad_i16(hops[h - 1], logits, label)
            ctx.stream_copy_features(ring)
            ctx.sync()
            head = (h + 1 - LAG) % T
            clip = torch.roll(ring, shifts=-head, dims=1).reshape(S, 1, T, NF).contiguous()
            torch.cuda.synchronize()
            ctx.forward_cnn_trad_f32(clip, want_l, want_k)
            ctx.sync()
            assert torch.equal(logits, want_l), f"push {h}: logits differ from the forward on the rotated ring"
            assert torch.equal(label, want_k), f"push {h}: labels differ"
            seen.update(label.tolist())
        assert ctx.stream_state()[1] == n
        assert torch.isfinite(logits).all()
        if S > 1:
            assert len(seen) > 1, "every push of every stream got one label"
    finally:
        ctx.close()


def test_k_push_argument_errors():
    ctx = _native.Context(0)
    try:
        hop = torch.zeros((2, HOP), dtype=torch.int16, device=DEV)
        logits = torch.full((2, 12), float("nan"), device=DEV)
        rc = lambda h, l: ctx._lib.kws_stream_push_cnn_trad_i16(ctx._h, h.data_ptr() if h is not None else None,
                                                               l.data_ptr() if l is not None else None, None)
        assert rc(hop, logits) == _native.KWS_ESTATE  # no stream set
        ctx.stream_open(2)
        assert rc(hop, logits) == _native.KWS_ESTATE  # no cnn-trad model
        ctx.load_cnn_trad(_blob(), 12)
        assert rc(None, logits) == _native.KWS_EINVAL
        assert rc(hop, None) == _native.KWS_EINVAL
        ctx.sync()
        assert ctx.stream_state()[1] == 0 and torch.isnan(logits).all()
    finally:
        ctx.close()


# ---- the spotter ------------------------------------------------------------------------------------------------------
def _ct_model(C=12):
    from kws.libs.models import CnnTradFpool3

    model = CnnTradFpool3(C)
    model.load_state_dict(o_ct.random_state(1, num_classes=C))
    return model


def test_l_live_events_follow_the_host_reference():
    """S = 3, smooth_window 4, no decision on partial windows: the popped events are those of tests/_live_detect_ref.py (float64)
    fed with the pushes' own logits; the scores agree within the float32 mean's bound (_scan_ref.tol_smooth)."""
    import _live_detect_ref as ld
    import _scan_ref as sref
    from kws.inference import DetectConfig, StreamingSpotter

    S, W, n = 3, 4, 101 + 44
    model = _ct_model()
    hops = _hops(S, n, seed=5).numpy()
    plain = StreamingSpotter(S, model)
    try:
        assert not plain._host, "cnn-trad-fpool3 has no zero-copy delivery"
        logits = np.stack([plain.push(hops[t])[1] for t in range(n)])  # [n, S, C]
    finally:
        plain.close()
    first_hop = ld.first_hop(T, 400, HOP)
    assert first_hop == 101
    # the rules: every class may fire, and the threshold sits in the widest gap of the reference's smoothed top scores
    sm = sref.smooth_ref(np.ascontiguousarray(logits[first_hop - 1:].transpose(1, 0, 2)), W)
    top = np.sort(sm.max(-1).reshape(-1))
    gap = int(np.argmax(np.diff(top[len(top) // 4:3 * len(top) // 4]))) + len(top) // 4
    threshold = float(0.5 * (top[gap] + top[gap + 1]))
    m2, mt = sref.margins(sm, threshold)
    tol = sref.tol_smooth(W)
    print(f"[cnn-trad live events] threshold {threshold:.6f}: top-2 margin {m2:.2e}, threshold margin {mt:.2e}, tol {tol:.2e}")
    assert m2 > 2 * tol and mt > 2 * tol, "the reference's own decisions lie within 2 tol of a boundary: pick other hops"
    want_ref = ld.LiveDetectRef(S, 12, W, 0, threshold, 5, first_hop=first_hop)
    want = [rec for t in range(n) for rec in want_ref.step(logits[t], hop=t + 1)]
    assert len(want) >= 4 and len({r[0] for r in want}) >= 2
    live = StreamingSpotter(S, model, detect=DetectConfig(threshold, smooth_window=W, refractory=5, first_keyword=0))
    try:
        got = []
        for t in range(n):
            lb, lg = live.push(hops[t])
            assert np.array_equal(lg.view(np.uint32), logits[t].view(np.uint32)), f"push {t + 1}: arming changed the logits"
            got += live.pop_events()
        assert [(e.stream, e.decision, e.hop, e.index) for e in got] == [(int(s), int(d), int(h), int(k)) for s, d, h, k, _ in want]
        for e, (_, _, h, _, score) in zip(got, want):
            assert abs(e.score - score) <= tol and e.time_s == ld.event_time(int(h), 400, HOP)
    finally:
        live.close()


def test_l_detection_set_of_another_class_count_is_refused_by_name():
    """The armed step compares the set's class count with the model that made the logits, and names the push entry; the DS-CNN
    entry behaves and speaks as it did."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "e2e_golden.npz"))
    for kind in ("cnn_trad", "dscnn"):
        ctx = _native.Context(0)
        try:
            if kind == "cnn_trad":
                ctx.load_cnn_trad(_blob(), 12)
                push = lambda h, lg: ctx._lib.kws_stream_push_cnn_trad_i16(ctx._h, h.data_ptr(), lg.data_ptr(), None)
                name = b"kws_stream_push_cnn_trad_i16"
            else:
                ctx.load_dscnn(g["he.blob"], 12)
                push = lambda h, lg: ctx._lib.kws_stream_push_i16(ctx._h, h.data_ptr(), lg.data_ptr(), None, 0)
                name = b"kws_stream_push_i16"
            ctx.stream_open(2)
            ctx.stream_detect_open(7, 2, 0, 0.5, 3, 0, 16)  # 7 classes; the model has 12
            hop = torch.zeros((2, HOP), dtype=torch.int16, device=DEV)
            logits = torch.zeros((2, 12), device=DEV)
            torch.cuda.synchronize()
            assert push(hop, logits) == _native.KWS_EINVAL
            msg = ctx._lib.kws_last_error(ctx._h)
            assert msg.startswith(name + b": kws_stream_detect_open was given another class count"), msg
            ctx.sync()
            assert ctx.stream_state()[1] == 1, "the hop was taken"
            ctx.stream_detect_close()
            ctx.stream_detect_open(12, 2, 0, 0.5, 3, 0, 16)
            assert push(hop, logits) == _native.KWS_OK
            ctx.sync()
            assert ctx.stream_detect_poll()[1] == 1
        finally:
            ctx.close()


def test_m_live_utterances_are_the_dscnn_spotters():
    """One gated stream: the endpointer and the cut are model-independent, so pop_utterances returns the spans a DS-CNN spotter
    returns for the same pushes, classified by this model's fused entry (model.infer_pcm16 of the cut clips)."""
    import _live_ref as lr
    from _segment_ref import cut_ref
    from kws.inference import StreamingSpotter, UtteranceConfig
    from kws.libs.models import DepthwiseSeparableConv

    on, off, pre_roll, n = 3, 5, 4, 66
    pattern = lr.delayed(lr.cycles(on, off, n), [0])
    pattern[0, n - 6:] = True  # ends inside an utterance: flush() closes it
    pcm = lr.pcm_of(pattern, 11)
    cfg = UtteranceConfig(threshold=lr.THR, on_window=on, off_window=off, pre_roll=pre_roll)
    model = _ct_model()
    torch.manual_seed(0)
    spotters = [StreamingSpotter(1, model, utterances=cfg), StreamingSpotter(1, DepthwiseSeparableConv(12), utterances=cfg)]
    try:
        runs = [[], []]
        for t in range(n):
            for sp, out in zip(spotters, runs):
                sp.push(pcm[:, t * HOP:(t + 1) * HOP])
                out += [(t, u) for u in sp.pop_utterances()]
        for sp, out in zip(spotters, runs):
            out += [(n, u) for u in sp.flush()]
    finally:
        for sp in spotters:
            sp.close()
    span = lambda u: (u.recording, u.start_s, u.end_s, u.open_s, u.close_s, u.reason, u.peak)
    assert [(t, span(u)) for t, u in runs[0]] == [(t, span(u)) for t, u in runs[1]]
    mine = [u for _, u in runs[0]]
    assert len(mine) >= 3 and mine[-1].reason == "end_of_recording"
    clips, peaks = cut_ref(pcm, [(0, round(u.start_s * 16000), round(u.end_s * 16000)) for u in mine], 16384, 16000)
    assert [u.peak for u in mine] == [int(p) for p in peaks]
    logits, labels = model.infer_pcm16(torch.from_numpy(clips).to(DEV))
    torch.cuda.synchronize()
    for i, u in enumerate(mine):
        assert np.array_equal(u.logits, logits[i].cpu().numpy()) and u.label == int(labels[i])


def test_n_input_rate_48k_hears_the_delayed_batch_resampling():
    """S = 2, 110 pushes of 480 samples at 48 kHz: the logits of a 16 kHz spotter pushed with kws_resample_i16 of the whole
    signal, delayed by delay_samples and cut into hops (the relation of tests/test_stream_resample_gpu.py)."""
    from kws.inference import StreamingSpotter

    S, n = 2, 110
    up, down, delay, _ = _native.host_stream_resample_plan(48000, 16000)
    x = np.random.default_rng(48).integers(-12000, 12001, size=(S, n * 480)).astype(np.int16)
    x[1, 20000:30000] = 0
    ctx = _native.Context(0)
    try:
        z = -(-delay // up)
        padded = np.concatenate([np.zeros((S, down * z), np.int16), x], axis=1)
        lo = up * z - delay
        out = torch.zeros((S, lo + n * HOP), dtype=torch.int16, device=DEV)
        src = torch.from_numpy(padded).to(DEV)
        torch.cuda.synchronize()
        ctx.resample_i16(src, 48000, 16000, out)
        ctx.sync()
        heard = out.cpu().numpy()[:, lo:]
    finally:
        ctx.close()
    model = _ct_model()
    at48, plain = StreamingSpotter(S, model, input_rate=48000), StreamingSpotter(S, model)
    try:
        assert (at48.hop_in, at48.delay_samples, at48._host) == (480, delay, False)
        for t in range(n):
            want_lb, want_lg = plain.push(heard[:, t * HOP:(t + 1) * HOP])
            lb, lg = at48.push(x[:, t * 480:(t + 1) * 480])
            assert np.array_equal(lb, want_lb) and np.array_equal(lg.view(np.uint32), want_lg.view(np.uint32)), f"push {t + 1}"
        assert np.isfinite(want_lg).all() and np.abs(want_lg).max() > 0
    finally:
        at48.close()
        plain.close()


def test_streaming_spotter_refusals_and_model_swap():
    from kws.common.errors import ModelError
    from kws.inference import StreamingSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = _ct_model()
    with pytest.raises(ModelError, match="use_graph"):
        StreamingSpotter(1, model, use_graph=True)
    sp = StreamingSpotter(2, model, smooth_window=3, vad_log_energy=-10.0)
    try:
        hop = _hops(2, 1, seed=9).numpy()[0]
        lb, post = sp.push(hop)
        assert np.allclose(post.sum(-1), 1.0, atol=1e-5) and sp.vad_state is not None
        with pytest.raises(ModelError, match="another model family"):
            sp.load_model(DepthwiseSeparableConv(12))
        sp.load_model(_ct_model())  # within the family: the streams keep running
        sp.push(hop)
    finally:
        sp.close()
