"""Batches of recordings of unequal length, the part that needs no GPU: the host plan (kws_host_ragged_plan) against a NumPy
restatement written here and against kws_host_scan_shape per recording, its refusals, and the argument checks of
KeywordSpotter.scan_batch / segment_batch / scan_files / segment_files that run before any device call."""
import ctypes as C
import wave

import numpy as np
import pytest

native = pytest.importorskip("kws._native")

T_WIN, FRAME_LEN, FRAME_STEP = 99, 400, 160
HOPS = [1, 3, 7, 99, 100]
EDGE_LENGTHS = [1, 400, 401, 16000, 16001]


def plan_ref(lengths, hop, frame_len=FRAME_LEN, frame_step=FRAME_STEP, window=T_WIN):
    """The layout of include/kws_hip.h, restated: rows rounded up to the hop per recording, windows by the scan's formula."""
    frames = [1 if n <= frame_len else 1 + -(-(n - frame_len) // frame_step) for n in lengths]
    frame_off = [0]
    for F in frames:
        frame_off.append(frame_off[-1] + -(-F // hop) * hop)
    windows = [0 if F < window else (F - window) // hop + 1 for F in frames]
    win_off = [o // hop for o in frame_off[:-1]]
    F_pack = frame_off[-1]
    return frames, frame_off, windows, win_off, (0 if F_pack < window else (F_pack - window) // hop + 1)


def _check_invariants(lengths, hop):
    frames, frame_off, windows, win_off, W_pack = native.host_ragged_plan(lengths, FRAME_LEN, FRAME_STEP, T_WIN, hop)
    want = plan_ref(lengths, hop)
    for got, exp in zip((frames, frame_off, windows, win_off), want[:4]):
        assert got.dtype == np.int32 and got.tolist() == exp
    assert W_pack == want[4]
    for r, n in enumerate(lengths):
        assert (int(frames[r]), int(windows[r])) == native.host_scan_shape(n, FRAME_LEN, FRAME_STEP, T_WIN, hop)
        assert frame_off[r] % hop == 0 and win_off[r] * hop == frame_off[r]
        assert frame_off[r] + frames[r] <= frame_off[r + 1] < frame_off[r] + frames[r] + hop  # rounded up, by less than a hop
        for w in ([0, int(windows[r]) - 1] if windows[r] else []):
            assert win_off[r] + w < W_pack, "a recording's window lies beyond the packed windows"
            first_row = (win_off[r] + w) * hop
            assert frame_off[r] <= first_row and first_row + T_WIN <= frame_off[r] + frames[r], "a window leaves its recording's rows"
    # the windows of no recording: at most ceil((T - 1) / hop) + 1 per recording
    assert W_pack - int(windows.sum()) <= len(lengths) * (-(-(T_WIN - 1) // hop) + 1)


@pytest.mark.parametrize("hop", HOPS)
def test_plan_matches_the_restatement_and_the_scan_shape(hop):
    _check_invariants(EDGE_LENGTHS, hop)
    _check_invariants(EDGE_LENGTHS[::-1], hop)
    for n in EDGE_LENGTHS:
        _check_invariants([n], hop)
    rng = np.random.default_rng(hop)
    for _ in range(50):
        R = int(rng.integers(1, 12))
        lengths = [int(v) for v in np.exp(rng.uniform(0.0, np.log(200000.0), R)).astype(np.int64) + 1]
        _check_invariants(lengths, hop)


def test_plan_takes_other_geometries_and_null_outputs():
    lengths = [5000, 30, 80000]
    got = native.host_ragged_plan(lengths, 410, 176, 50, 4)
    want = plan_ref(lengths, 4, 410, 176, 50)
    assert [g.tolist() for g in got[:4]] == list(want[:4]) and got[4] == want[4]
    ln = (C.c_int32 * 3)(*lengths)
    w_pack = C.c_int(-1)
    assert native.lib().kws_host_ragged_plan(ln, 3, 410, 176, 50, 4, None, None, None, None, C.byref(w_pack)) == native.KWS_OK
    assert w_pack.value == want[4]
    assert native.lib().kws_host_ragged_plan(ln, 3, 410, 176, 50, 4, None, None, None, None, None) == native.KWS_OK


def test_plan_refusals():
    lib = native.lib()
    ln = (C.c_int32 * 3)(16000, 400, 1)
    call = lambda p, R, hop=1, fl=FRAME_LEN: lib.kws_host_ragged_plan(p, R, fl, FRAME_STEP, T_WIN, hop, None, None, None, None, None)
    assert call(ln, 3) == native.KWS_OK
    assert call(ln, 0) == native.KWS_EINVAL and call(ln, -1) == native.KWS_EINVAL      # R < 1
    assert call(ln, 3, hop=0) == native.KWS_EINVAL and call(ln, 3, hop=-2) == native.KWS_EINVAL  # hop < 1
    assert call((C.c_int32 * 3)(16000, 0, 1), 3) == native.KWS_EINVAL                  # a zero length
    assert call((C.c_int32 * 3)(16000, -5, 1), 3) == native.KWS_EINVAL
    assert call(None, 3) == native.KWS_EINVAL and call(ln, 3, fl=0) == native.KWS_EINVAL
    # limits: more than 2^20 recordings, more than 2^28 packed rows
    many = np.ones((1 << 20) + 1, np.int32)
    assert call(many.ctypes.data_as(C.POINTER(C.c_int32)), len(many)) == native.KWS_EUNSUPPORTED
    assert call(many.ctypes.data_as(C.POINTER(C.c_int32)), 1 << 20) == native.KWS_OK
    long_ones = np.full(64, 1 << 30, np.int32)  # 64 x 6.7 million frames
    assert call(long_ones.ctypes.data_as(C.POINTER(C.c_int32)), 64) == native.KWS_EUNSUPPORTED
    with pytest.raises(native.KWSError):
        native.host_ragged_plan([16000, 0])


# ---- the Python argument checks that need no device -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spotter():
    from kws.inference import KeywordSpotter

    return KeywordSpotter()


def _wav(path, x, rate=16000, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(x, "<i2").tobytes())
    return str(path)


def test_batch_argument_checks(spotter):
    from kws.common.errors import ModelError

    ok = np.zeros(16000, np.int16)
    for call in (spotter.scan_batch, lambda recs, **kw: spotter.segment_batch(recs, threshold=0.0, **kw)):
        with pytest.raises(ModelError, match="no recordings"):
            call([])
        with pytest.raises(ModelError, match="recording 1 is empty"):
            call([ok, np.zeros(0, np.int16), ok])
        with pytest.raises(ModelError, match="recording 2.*int16"):
            call([ok, ok, ok.astype(np.float32)])
        with pytest.raises(ModelError, match="recording 0 must be one int16"):
            call([np.zeros((2, 100), np.int16)])
        with pytest.raises(ModelError, match="2 sample rates for 1 recordings"):
            call([ok], sample_rate=[16000, 8000])
        with pytest.raises(ModelError, match="sample rates must be positive"):
            call([ok], sample_rate=0)
    with pytest.raises(ModelError, match="hop_frames"):
        spotter.scan_batch([ok], hop_frames=0)
    with pytest.raises(ModelError, match="smooth_window"):
        spotter.scan_batch([ok], threshold=0.5, smooth_window=257)
    with pytest.raises(ModelError, match="refractory"):
        spotter.scan_batch([ok], threshold=0.5, refractory=0)
    with pytest.raises(ModelError, match="on_window"):
        spotter.segment_batch([ok], threshold=0.0, on_window=5, off_window=4)
    with pytest.raises(ModelError, match="normalize"):
        spotter.segment_batch([ok], threshold=0.0, normalize=40000)
    with pytest.raises(ModelError, match="max_seconds"):
        spotter.segment_batch([ok], threshold=0.0, max_seconds=0.01)


def test_file_decode_rules_are_the_single_file_ones(spotter, tmp_path):
    from kws.common.errors import AudioProcessingError

    good = _wav(tmp_path / "good.wav", np.zeros(800, np.int16))
    stereo = _wav(tmp_path / "stereo.wav", np.zeros(1600, np.int16), channels=2)
    other = _wav(tmp_path / "other.wav", np.zeros(800, np.int16), rate=8000)
    for many, one, kw in ((spotter.scan_files, spotter.scan_file, {}), (spotter.segment_files, spotter.segment_file, {"threshold": 0.0})):
        for bad in (stereo, other):  # refused while decoding, before any device call, with the single-file method's own words
            with pytest.raises(AudioProcessingError) as single:
                one(bad, **kw)
            with pytest.raises(AudioProcessingError) as batch:
                many([good, bad], **kw)
            assert str(batch.value) == str(single.value)
