"""CPU tests of the float32 recording path: the argument checks of the new methods need no device, the int16 methods keep
their refusals and defaults, and the NumPy restatement of kws_cut_f32 that the GPU tests trust is checked on a hand-made case."""
import inspect
import wave

import numpy as np
import pytest

from _f32_ref import cut_f32_ref, unit
from kws import _native
from kws.common.errors import AudioProcessingError, ModelError
from kws.inference import KeywordSpotter, Utterance


@pytest.fixture(scope="module")
def spotter():
    return KeywordSpotter()


def test_the_five_entries_are_bound():
    import ctypes as C

    for name in ("kws_scan_f32", "kws_frames_f32", "kws_frames_ragged_f32", "kws_scan_ragged_f32", "kws_cut_f32"):
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name)
        assert len(_native.SIGNATURES[name][1]) == len(_native.SIGNATURES[name.replace("_f32", "_i16")][1]), "a twin's arity"
    twin = _native.SIGNATURES["kws_cut_i16"][1]
    assert [a is C.c_float for a in _native.SIGNATURES["kws_cut_f32"][1]] == [i == 6 for i in range(len(twin))], "normalize_to is the one float"
    for name in ("scan_f32", "frames_f32", "frames_ragged_f32", "scan_ragged_f32", "cut_f32"):
        assert callable(getattr(_native.Context, name))
    assert _native.lib().kws_abi_version() == 1


def test_scan_f32_and_segment_f32_argument_checks_need_no_device(spotter):
    ok = np.zeros(32000, np.float32)
    for call in (spotter.scan_f32, lambda x, **kw: spotter.segment_f32(x, threshold=0.0, **kw)):
        with pytest.raises(ModelError, match="float32"):
            call(ok.astype(np.int16))
        with pytest.raises(ModelError, match="float32"):
            call(ok.astype(np.float64))
        with pytest.raises(ModelError, match="float32.*shape"):
            call(np.zeros((2, 3, 16000), np.float32))
    with pytest.raises(ModelError, match="scan_f32: hop_frames"):
        spotter.scan_f32(ok, hop_frames=0)
    with pytest.raises(ModelError, match="scan_f32: smooth_window"):
        spotter.scan_f32(ok, threshold=0.5, smooth_window=257)
    with pytest.raises(ModelError, match="refractory"):
        spotter.scan_f32(ok, threshold=0.5, refractory=0)
    with pytest.raises(ModelError, match="scan_f32: .*shorter than one window"):
        spotter.scan_f32(np.zeros(8000, np.float32))
    with pytest.raises(ModelError, match="segment_f32: need 1 <= on_window"):
        spotter.segment_f32(ok, threshold=0.0, on_window=5, off_window=4)
    with pytest.raises(ModelError, match="normalize in \\[0, 32767\\]"):
        spotter.segment_f32(ok, threshold=0.0, normalize=40000)  # normalize stays in int16 units
    with pytest.raises(ModelError, match="segment_f32: max_seconds"):
        spotter.segment_f32(ok, threshold=0.0, max_seconds=0.01)
    with pytest.raises(ModelError, match="segment_f32: the recording is empty"):
        spotter.segment_f32(np.zeros(0, np.float32), threshold=0.0)


def test_batch_f32_argument_checks_and_the_mixed_batch_messages(spotter):
    ok, ok16 = np.zeros(16000, np.float32), np.zeros(16000, np.int16)
    for call in (spotter.scan_batch_f32, lambda recs, **kw: spotter.segment_batch_f32(recs, threshold=0.0, **kw)):
        with pytest.raises(ModelError, match="no recordings"):
            call([])
        with pytest.raises(ModelError, match="recording 1 is empty"):
            call([ok, np.zeros(0, np.float32), ok])
        with pytest.raises(ModelError, match="recording 2.*float32"):
            call([ok, ok, ok16])
        with pytest.raises(ModelError, match="recording 0 must be one float32"):
            call([np.zeros((2, 100), np.float32)])
        with pytest.raises(ModelError, match="2 sample rates for 1 recordings"):
            call([ok], sample_rate=[16000, 8000])
    with pytest.raises(ModelError, match="scan_batch_f32: hop_frames"):
        spotter.scan_batch_f32([ok], hop_frames=0)
    with pytest.raises(ModelError, match="segment_batch_f32: need pre_roll"):
        spotter.segment_batch_f32([ok], threshold=0.0, normalize=-1)
    # a float32 member of an otherwise int16 batch keeps being refused, in the words it had
    for call in (spotter.scan_batch, lambda recs: spotter.segment_batch(recs, threshold=0.0)):
        with pytest.raises(ModelError, match="recording 2.*int16"):
            call([ok16, ok16, ok])
    with pytest.raises(ModelError, match="scan expects int16 PCM, got float32"):
        spotter.scan(ok)
    with pytest.raises(ModelError, match="segment expects int16 PCM, got float32"):
        spotter.segment(ok, threshold=0.0)


def test_defaults_are_unchanged_and_decode_is_checked(spotter, tmp_path):
    for name in ("scan_file", "segment_file", "scan_files", "segment_files"):
        params = inspect.signature(getattr(KeywordSpotter, name)).parameters
        assert params["decode"].default == "pcm16" and params["resample"].default is False
    for i16, f32 in (("scan", "scan_f32"), ("segment", "segment_f32"), ("scan_batch", "scan_batch_f32"), ("segment_batch", "segment_batch_f32")):
        a, b = inspect.signature(getattr(KeywordSpotter, i16)).parameters, inspect.signature(getattr(KeywordSpotter, f32)).parameters
        assert [(p.name, p.default) for p in list(a.values())[2:]] == [(p.name, p.default) for p in list(b.values())[2:]]
    assert "peak" in Utterance.__dataclass_fields__

    def write(name, rate, width, channels=1):
        path = str(tmp_path / name)
        with wave.open(path, "wb") as w:
            w.setnchannels(channels)
            w.setsampwidth(width)
            w.setframerate(rate)
            w.writeframes(b"\0" * (width * channels * 32000))
        return path

    wide, slow = write("wide.wav", 16000, 3), write("slow.wav", 8000, 3)
    with pytest.raises(AudioProcessingError, match="16-bit"):
        spotter.scan_file(wide)  # the default decode refuses as before
    with pytest.raises(AudioProcessingError, match="there is no float32 scan"):
        spotter.scan_file(slow, resample=True)
    with pytest.raises(AudioProcessingError, match="decode must be 'pcm16' or 'any'"):
        spotter.scan_file(wide, decode="float")
    with pytest.raises(AudioProcessingError, match="decode must be"):
        spotter.segment_files([wide], decode="f32", threshold=0.0)
    with pytest.raises(AudioProcessingError, match="sample rate 8000 != 16000"):
        spotter.scan_file(slow, decode="any")  # refused while decoding, before any device call
    with pytest.raises(AudioProcessingError, match="sample rate 8000 != 16000"):
        spotter.segment_files([slow], decode="any", threshold=0.0)


def test_the_file_methods_refuse_in_their_own_words(spotter, tmp_path):
    """The full message of every decode refusal of the four file methods, before any device call.  Under decode="pcm16" the
    plural methods speak with the singular method's name; under decode="any" with their own."""
    def write(name, rate, width, channels=1):
        path = str(tmp_path / name)
        with wave.open(path, "wb") as w:
            w.setnchannels(channels)
            w.setsampwidth(width)
            w.setframerate(rate)
            w.writeframes(b"\0" * (width * channels * 64))
        return path

    slow, slow24, stereo = write("slow.wav", 8000, 2), write("slow24.wav", 8000, 3), write("stereo.wav", 16000, 2, channels=2)
    methods = {"scan_file": (spotter.scan_file, "scan_file", " (there is no float32 scan)"),
               "segment_file": (lambda p, **kw: spotter.segment_file(p, threshold=0.0, **kw), "segment_file", ""),
               "scan_files": (lambda p, **kw: spotter.scan_files([p], **kw), "scan_file", " (there is no float32 scan)"),
               "segment_files": (lambda p, **kw: spotter.segment_files([p], threshold=0.0, **kw), "segment_file", "")}
    for name, (call, singular, tail) in methods.items():
        def message(path, **kw):
            with pytest.raises(AudioProcessingError) as e:
                call(path, **kw)
            assert e.value.args[0].startswith("Audio processing error: ")
            return e.value.args[0][len("Audio processing error: "):]

        assert message(slow) == f"{slow}: sample rate 8000 != 16000; resampling is not implemented"
        assert message(slow, decode="any") == f"{slow}: sample rate 8000 != 16000; pass resample=True to {name} to resample on the device"
        assert message(slow24, resample=True) == (f"{slow24}: sample rate 8000 != 16000 and the file is not 16-bit mono PCM; the device "
                                                  f"resampler of {singular} takes int16 only{tail}")
        assert message(slow24) == f"{slow24}: only 16-bit PCM WAV is supported (sample width 3)"
        assert message(stereo) == f"{stereo}: 2 channels; {singular} takes mono files"
        assert message(stereo, resample=True) == f"{stereo}: 2 channels; {singular} takes mono files"
        assert message(slow, decode="float") == f"{name}: decode must be 'pcm16' or 'any', got 'float'"
        assert message(slow, decode=None, resample=True) == f"{name}: decode must be 'pcm16' or 'any', got None"


def test_the_restatement_of_the_float_cut_on_a_hand_made_case():
    x = np.array([[0.25, -0.5, np.nan, 0.125, 0.0, 1.5, -2.0, 0.0625]], np.float32)
    spans = [(0, 0, 4), (0, 3, 5), (0, 4, 5), (0, 5, 99), (0, 2, 2), (1, 0, 4), (-1, 0, 4), (0, -3, 2)]
    clips, peaks = cut_f32_ref(x, spans, 0.5, 3)
    assert peaks.dtype == np.float32 and peaks.tolist() == [0.5, 0.125, 0.0, 2.0, 0.0, -1.0, -1.0, 0.5]  # the NaN raises nothing
    assert np.array_equal(clips[0], np.float32([0.25, -0.5, np.nan]), equal_nan=True)                  # times = 1
    assert clips[1].tolist() == [0.5, 0.0, 0.0]                                                        # 0.125 * 4, zeros past the span
    assert clips[2].tolist() == [0.0, 0.0, 0.0] and clips[4].tolist() == [0.0, 0.0, 0.0]               # peak 0, empty
    assert clips[3].tolist() == [0.375, -0.5, 0.015625]                                                # the peak 2.0 lies inside n_out here
    assert clips[5].tolist() == clips[6].tolist() == [0.0, 0.0, 0.0]                                   # recording out of range
    assert clips[7].tolist() == [0.25, -0.5, 0.0]                                                      # start clamped to 0
    copy, peaks0 = cut_f32_ref(x, spans, 0.0, 3)
    assert np.array_equal(copy[0].view(np.uint32), x[0, :3].view(np.uint32)) and peaks0.tolist() == peaks.tolist()
    # one rounding: the float64 product rounded once is not always the float32 product
    y = np.array([[np.float32(1.0) / np.float32(3.0), 0.7]], np.float32)
    clips, _ = cut_f32_ref(y, [(0, 0, 2)], 0.3, 2)
    t = np.float64(np.float32(0.3)) / np.float64(np.float32(0.7))
    assert clips[0, 0] == np.float32(np.float64(y[0, 0]) * t) and clips[0, 1] == np.float32(np.float64(y[0, 1]) * t)
    assert np.array_equal(unit(np.array([-32768, 1, 32767], np.int16)), np.float32([-1.0, 2.0 ** -15, 32767 / 32768]))
