"""Scanning long recordings, the parts that need no GPU: the shape helper of the C ABI against the oracle's frame count and the
window formula, the window-time helper, and the argument checks ``KeywordSpotter.scan`` makes before it touches a device."""
import os
import wave

import numpy as np
import pytest

import _scan_ref as ref
from kws import _native
from kws.common.errors import AudioProcessingError, KWSError, ModelError
from kws.inference import KeywordSpotter, ScanResult, scan_window_times
from oracle import psf_mfcc as o_mfcc

pytestmark = pytest.mark.skipif(not os.path.exists(_native.LIB_PATH), reason="libkws_hip.so not built")

LENGTHS = [399, 400, 401, 16000, 16080, 16081, 21973, 48053]
HOPS = [1, 2, 3, 99, 150]


@pytest.mark.parametrize("n", LENGTHS)
def test_host_scan_shape_matches_the_oracle_frame_count_and_the_window_formula(n):
    frames_oracle = o_mfcc.FrontendSpec(n_samples=n).num_frames
    for hop in HOPS:
        frames, windows = _native.host_scan_shape(n, 400, 160, 99, hop)
        assert frames == frames_oracle == ref.scan_shape(n, hop)[0], (n, hop)
        want = 0 if frames < 99 else (frames - 99) // hop + 1
        assert windows == want == ref.scan_shape(n, hop)[1], (n, hop)


def test_host_scan_shape_edges():
    assert _native.host_scan_shape(16000) == (99, 1)            # one second is one window
    assert _native.host_scan_shape(15999) == (99, 1)            # the last frame is zero-padded: still 99 frames
    assert _native.host_scan_shape(15840) == (98, 0)            # shorter than a window: no windows, not an error
    assert _native.host_scan_shape(399) == (1, 0)
    assert _native.host_scan_shape(16081, hop_frames=1) == (100, 2)
    assert _native.host_scan_shape(16081, hop_frames=2) == (100, 1)
    assert _native.host_scan_shape(48053, hop_frames=5) == (299, 41)
    assert _native.host_scan_shape(80000, hop_frames=1) == (499, 401)
    assert _native.host_scan_shape(9_600_000, hop_frames=1) == (59999, 59901)
    # another geometry: 30 ms frames every 20 ms, windows of 49 frames
    assert _native.host_scan_shape(16000, 480, 320, 49, 1) == (50, 2)
    # either output may be NULL
    lib, out = _native.lib(), _native.C.c_int(0)
    assert lib.kws_host_scan_shape(16081, 400, 160, 99, 1, None, _native.C.byref(out)) == 0 and out.value == 2
    assert lib.kws_host_scan_shape(16081, 400, 160, 99, 1, _native.C.byref(out), None) == 0 and out.value == 100


@pytest.mark.parametrize("args", [(0, 400, 160, 99, 1), (-5, 400, 160, 99, 1), (16000, 0, 160, 99, 1), (16000, 400, 0, 99, 1),
                                  (16000, 400, 160, 0, 1), (16000, 400, 160, 99, 0), (16000, 400, 160, 99, -1)])
def test_host_scan_shape_refuses_non_positive_sizes(args):
    assert _native.lib().kws_host_scan_shape(*args, None, None) == _native.KWS_EINVAL
    with pytest.raises(KWSError):
        _native.host_scan_shape(*args)


def test_window_times():
    start, end = scan_window_times(4, 3)
    np.testing.assert_array_equal(start, np.array([0, 480, 960, 1440]) / 16000.0)
    np.testing.assert_array_equal(end, (np.array([0, 480, 960, 1440]) + 98 * 160 + 400) / 16000.0)
    assert start[1] - start[0] == 3 * 0.01
    # the last window of a recording whose last frame is zero-padded ends with the recording
    frames, W = _native.host_scan_shape(21973, hop_frames=1)
    start, end = scan_window_times(W, 1, n_total=21973)
    assert W == 38 and end[-1] == 21973 / 16000.0 and end[-2] == (36 * 160 + 98 * 160 + 400) / 16000.0
    # one second: one window, the whole clip
    start, end = scan_window_times(1, 1, n_total=16000)
    assert (start[0], end[0]) == (0.0, 1.0)
    assert scan_window_times(0, 1)[0].shape == (0,)


def test_scan_argument_checks_need_no_device(tmp_path):
    sp = KeywordSpotter()
    ok = np.zeros(32000, np.int16)
    with pytest.raises(ModelError, match="int16"):
        sp.scan(ok.astype(np.float32))
    with pytest.raises(ModelError, match="int16"):
        sp.scan(ok.astype(np.int32))
    with pytest.raises(ModelError, match="shape"):
        sp.scan(np.zeros((2, 3, 16000), np.int16))
    with pytest.raises(ModelError, match="hop_frames"):
        sp.scan(ok, hop_frames=0)
    with pytest.raises(ModelError, match="smooth_window"):
        sp.scan(ok, threshold=0.5, smooth_window=0)
    with pytest.raises(ModelError, match="smooth_window"):
        sp.scan(ok, threshold=0.5, smooth_window=257)
    with pytest.raises(ModelError, match="refractory"):
        sp.scan(ok, threshold=0.5, refractory=0)
    with pytest.raises(ModelError, match="max_events"):
        sp.scan(ok, threshold=0.5, max_events=-1)
    with pytest.raises(ModelError, match="shorter than one window"):
        sp.scan(np.zeros(8000, np.int16))
    with pytest.raises(ModelError, match="shorter than one window"):
        sp.scan(np.zeros((2, 15840), np.int16))
    with pytest.raises(ModelError, match="shorter than one window"):
        sp.scan(np.zeros(0, np.int16))

    def write(name, rate, width, channels):
        path = str(tmp_path / name)
        with wave.open(path, "wb") as w:
            w.setnchannels(channels)
            w.setsampwidth(width)
            w.setframerate(rate)
            w.writeframes(b"\0" * (width * channels * 32000))
        return path

    with pytest.raises(AudioProcessingError, match="sample rate 8000"):
        sp.scan_file(write("rate.wav", 8000, 2, 1))
    with pytest.raises(AudioProcessingError, match="16-bit"):
        sp.scan_file(write("width.wav", 16000, 1, 1))
    with pytest.raises(AudioProcessingError, match="2 channels"):
        sp.scan_file(write("stereo.wav", 16000, 2, 2))
    assert ScanResult.__dataclass_fields__.keys() >= {"labels", "logits", "window_start_s", "events"}


def test_the_restatement_of_the_decisions_on_a_hand_made_track():
    """The float64 restatement the GPU test trusts, on a case small enough to check by hand."""
    z = np.full((1, 6, 3), -20.0, np.float32)
    for w, k in enumerate([2, 2, 0, 1, 1, 2]):
        z[0, w, k] = 20.0
    s1 = ref.smooth_ref(z, 1)
    assert [e[:2] for e in ref.events_ref(s1, 0, 0.5, 1)[0]] == [(0, 2), (1, 2), (2, 0), (3, 1), (4, 1), (5, 2)]
    assert [e[:2] for e in ref.events_ref(s1, 1, 0.5, 1)[0]] == [(0, 2), (1, 2), (3, 1), (4, 1), (5, 2)]
    assert [e[:2] for e in ref.events_ref(s1, 1, 0.5, 3)[0]] == [(0, 2), (3, 1)]
    assert [e[:2] for e in ref.events_ref(s1, 0, 0.5, 1000)[0]] == [(0, 2)]
    s3 = ref.smooth_ref(z, 3)  # windows {2}, {2,2}, {2,2,0}, {2,0,1}, {0,1,1}, {1,1,2}
    np.testing.assert_allclose(s3[0, :, 2], [1, 1, 2 / 3, 1 / 3, 0, 1 / 3], atol=1e-12)
    assert [e[:2] for e in ref.events_ref(s3, 0, 0.5, 1)[0]] == [(0, 2), (1, 2), (2, 2), (4, 1), (5, 1)]


def test_the_decision_fixture_is_clear_of_its_boundaries():
    """What the GPU test asserts first, checked here too: a drifted generator or seed table shows without a GPU."""
    for (W, Cn), seeds in ref.DETECT_SEEDS.items():
        z = ref.detect_logits(W, Cn, seeds)
        assert z.shape == (3, W, Cn) and z.dtype == np.float32
        for S in (1, 7, 256):
            m2, mt = ref.margins(ref.smooth_ref(z, S), 0.5)
            assert min(m2, mt) > 2 * ref.tol_smooth(S), (W, Cn, S, m2, mt)
    events = ref.events_ref(ref.smooth_ref(ref.detect_logits(200, 12, ref.DETECT_SEEDS[(200, 12)]), 7), 2, 0.5, 5)
    assert all(len(e) > 3 for e in events) and len({k for e in events for _, k, _ in e}) > 2
