"""CPU tests of the device resampler's host side: the taps kws_host_resample_design hands back (exactly the device table)
against scipy's own design, the lengths, the limits, the NumPy restatement test_resample_gpu.py judges the kernel by against
scipy.signal.resample_poly, read_wav beside load_audio, and the hazard lint over the new unit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from scipy.signal import resample_poly

import _resample_ref as ref
from conftest import REPO
from test_host_audio_cpu import write_wav

native = pytest.importorskip("kws._native")

# the six pairs of the definition's own check, then two with many zero crossings per tap (96 and 192 kHz -> 16 kHz)
DESIGN_PAIRS = [(48000, 16000), (44100, 16000), (8000, 16000), (44100, 32000), (32000, 48000), (44100, 64000), (96000, 16000),
                (192000, 16000)]
DESIGN_RATIOS = [(1, 3), (160, 441), (2, 1), (320, 441), (3, 2), (640, 441), (1, 6), (1, 12)]


@pytest.mark.parametrize("rates,want", list(zip(DESIGN_PAIRS, DESIGN_RATIOS)), ids=[f"{u}/{d}" for u, d in DESIGN_RATIOS])
def test_taps_are_scipys_firwin(rates, want):
    """1e-13 absolute: 2^8 x the difference between two float64 formulations of the same taps, 2^-20 of a float32 ulp at full
    scale; a shifted or mis-scaled tap is off by 1e-3 or more."""
    up, down, half, tile, taps = native.host_resample_design(*rates)
    assert (up, down) == want == ref.ratio(*rates)
    assert half == 10 * max(up, down) and taps.shape == (2 * half + 1,) and taps.dtype == np.float64
    assert tile >= 1
    err = np.abs(taps - ref.firwin_taps(up, down)).max()
    print(f"[resample-taps] {up}/{down}: max |taps - firwin| = {err:.2e}")
    assert err <= 1e-13
    assert abs(taps.sum() - up) <= 1e-12 * up and np.array_equal(taps, taps[::-1])


def test_design_count_protocol_and_errors():
    fn = native.lib().kws_host_resample_design
    need, up = C.c_size_t(7), C.c_int(0)
    assert fn(48000, 16000, C.byref(up), None, None, None, None, 0, C.byref(need)) == native.KWS_OK
    assert need.value == 61 and up.value == 1
    buf = np.full(62, np.nan)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert fn(48000, 16000, None, None, None, None, p, 60, C.byref(need)) == native.KWS_EINVAL  # cap below need
    assert need.value == 61 and np.isnan(buf).all()
    assert fn(48000, 16000, None, None, None, None, p, 61, None) == native.KWS_OK
    assert np.isfinite(buf[:61]).all() and np.isnan(buf[61])
    for bad in ((0, 16000), (16000, 0), (-1, 16000)):
        assert fn(*bad, None, None, None, None, None, 0, C.byref(need)) == native.KWS_EINVAL and need.value == 0
    # max(up, down) <= 1024 after reduction
    assert fn(1024, 1, None, None, None, None, None, 0, C.byref(need)) == native.KWS_OK and need.value == 20481
    assert fn(1025, 1, None, None, None, None, None, 0, C.byref(need)) == native.KWS_EUNSUPPORTED and need.value == 0
    assert fn(16000, 16001, None, None, None, None, None, 0, None) == native.KWS_EUNSUPPORTED
    assert fn(2050, 2, None, None, None, None, None, 0, None) == native.KWS_EUNSUPPORTED  # 1025 / 1
    assert fn(2048, 2, None, None, None, None, None, 0, None) == native.KWS_OK
    with pytest.raises(Exception, match="1024"):
        native.host_resample_design(16000, 16001)
    # equal rates: the copy; a design exists all the same
    up, down, half, tile, taps = native.host_resample_design(16000, 16000)
    assert (up, down, half) == (1, 1, 10) and tile >= 1 and taps.shape == (21,)


def test_lengths():
    for rates in DESIGN_PAIRS + [(16000, 16000)]:
        up, down = ref.ratio(*rates)
        for n in list(range(0, 40)) + [down, 2 * down, 7 * down, 7 * down + 1, 7 * down - 1, 16000, 28800000, 1 << 30 if up <= down else 1 << 20]:
            assert native.host_resample_len(n, *rates) == -((-n * up) // down), (rates, n)
    n = C.c_int(-5)
    fn = native.lib().kws_host_resample_len
    assert fn(10, 0, 16000, C.byref(n)) == native.KWS_EINVAL and fn(-1, 8000, 16000, C.byref(n)) == native.KWS_EINVAL
    assert fn(10, 8000, 16000, None) == native.KWS_EINVAL
    assert fn(10, 1025, 1, C.byref(n)) == native.KWS_EUNSUPPORTED
    assert fn(1 << 30, 8000, 16000, C.byref(n)) == native.KWS_EUNSUPPORTED and n.value == -5  # 2^31 does not fit an int


def test_kernel_id():
    assert native.KWS_K_RESAMPLE == 10 and native.kernel_name(native.KWS_K_RESAMPLE) == "kws_resample_kernel"
    assert native.kernel_name(native.KWS_K_RESAMPLE + 1) == ""


@pytest.mark.parametrize("rates", DESIGN_PAIRS[:6], ids=[f"{u}/{d}" for u, d in DESIGN_RATIOS[:6]])
def test_the_restatement_is_resample_poly(rates):
    up, down = ref.ratio(*rates)
    taps = ref.firwin_taps(up, down)
    rng = np.random.default_rng(up * 1000 + down)
    for n in (1, 2, 37, 1000, 2999):
        x = rng.uniform(-1, 1, n)
        want = resample_poly(x, up, down, window=("kaiser", 14.0))
        y, S = ref.resample_ref(x, up, down, taps)
        assert y.shape == (1, len(want)) == (1, ref.natural_len(n, up, down))
        assert np.abs(y[0] - want).max() <= 4e-15 * np.abs(x).max(), (rates, n)
        assert (S[0] >= np.abs(y[0])).all()
    for m0 in (0, 500, 999):  # one non-zero term per output: bit for bit
        x = np.zeros(1000)
        x[m0] = 1.0
        y, _ = ref.resample_ref(x, up, down, taps)
        assert np.array_equal(y[0], resample_poly(x, up, down, window=("kaiser", 14.0))), (rates, m0)


def test_the_restatement_handles_lengths_and_n_out():
    up, down = 1, 3
    taps = ref.firwin_taps(up, down)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (3, 300))
    lens = [300, 0, 151]
    y, _ = ref.resample_ref(x, up, down, taps, d_len=lens, n_out=120)
    for r, L in enumerate(lens):
        alone = resample_poly(x[r, :L], up, down, window=("kaiser", 14.0)) if L else np.zeros(0)
        n = ref.natural_len(L, up, down)
        assert len(alone) == n
        assert np.abs(y[r, :min(n, 120)] - alone[:120]).max(initial=0.0) <= 4e-15
        assert (y[r, n:] == 0).all()


def test_read_wav_beside_load_audio(tmp_path):
    from kws.libs.audio_processor import load_audio, read_wav, resample_host

    rng = np.random.default_rng(0)
    x8 = (np.sin(2 * np.pi * 440 * np.arange(8000) / 8000.0) * 12000).astype(np.int16)
    write_wav(tmp_path / "r8k.wav", x8.tobytes(), 1, 1, 8000, 16)
    pcm, rate = read_wav(tmp_path / "r8k.wav")
    assert rate == 8000 and pcm.dtype == np.int16 and np.array_equal(pcm, x8)
    # read_wav + the host resampler = load_audio(resample=True), bit for bit
    via = resample_host(pcm.astype(np.float32) / np.float32(32768.0), 8000, 16000).astype(np.float32)
    assert np.array_equal(via, load_audio(tmp_path / "r8k.wav", resample=True))
    # every other encoding: float32 mono, the array load_audio returns, at the file's own rate
    i16 = rng.integers(-32768, 32768, 1000, dtype=np.int16)
    write_wav(tmp_path / "a16.wav", i16.tobytes(), 1, 1, 16000, 16)
    assert np.array_equal(load_audio(tmp_path / "a16.wav"), i16.astype(np.float32) / np.float32(32768))
    u8 = rng.integers(0, 256, 999, dtype=np.uint8)
    i24 = rng.integers(-(1 << 23), 1 << 23, 500)
    i32 = rng.integers(-(1 << 31), 1 << 31, 400, dtype=np.int64).astype("<i4")
    f32 = rng.uniform(-1, 1, (300, 2)).astype("<f4")
    f64 = rng.uniform(-1, 1, 200).astype("<f8")
    st = rng.integers(-3000, 3000, (100, 2), dtype=np.int16)
    files = {"a8": (u8.tobytes(), 1, 1, 8, False, (u8.astype(np.float32) - 128) / 128),
             "a24": (b"".join(int(v & 0xFFFFFF).to_bytes(3, "little") for v in i24), 1, 1, 24, True, (i24 / 8388608.0).astype(np.float32)),
             "a32": (i32.tobytes(), 1, 1, 32, False, (i32.astype(np.float64) / 2147483648.0).astype(np.float32)),
             "f32s": (f32.tobytes(), 3, 2, 32, False, f32.mean(axis=1, dtype=np.float32)),
             "f64": (f64.tobytes(), 3, 1, 64, False, f64.astype(np.float32)),
             "st16": (st.tobytes(), 1, 2, 16, False, (st.astype(np.float32) / np.float32(32768)).mean(axis=1, dtype=np.float32))}
    for name, (payload, tag, ch, bits, ext, want) in files.items():
        for file_rate in (16000, 22050):
            path = tmp_path / f"{name}_{file_rate}.wav"
            write_wav(path, payload, tag, ch, file_rate, bits, extensible=ext)
            got, rate = read_wav(path)
            assert rate == file_rate and got.dtype == np.float32 and np.array_equal(got, want), name
        assert np.array_equal(load_audio(tmp_path / f"{name}_16000.wav"), want), name  # load_audio's own output is what it was
    from kws.common.errors import AudioProcessingError

    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    with pytest.raises(AudioProcessingError, match="not a RIFF/WAVE file"):
        read_wav(tmp_path / "junk.wav")
    write_wav(tmp_path / "adpcm.wav", b"\0" * 64, 2, 1, 44100, 4)
    with pytest.raises(AudioProcessingError, match="unsupported WAV encoding"):
        read_wav(tmp_path / "adpcm.wav")


def test_no_unprotected_hazard_in_the_resample_unit():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_hazard_lint as lint

    if not os.path.exists(lint.HIPCC):
        pytest.skip("hipcc not installed")
    findings, _, isa = lint.lint_file(os.path.join(REPO, "keyword-spotting_amd", "csrc", "kws_resample.hip"))
    flat = [(fn[:60], line, rule, msg) for fn, fs in findings.items() for line, rule, msg in fs]
    assert not flat, f"kws_resample.hip ({isa}): {flat[:5]}"
    body = open(isa).read()
    assert "v_fmac_f64" in body or "v_fma_f64" in body  # the walk saw the kernel: fused float64 multiply-adds
