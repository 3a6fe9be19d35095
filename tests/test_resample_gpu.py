"""The device resampler (kws_resample_i16 / kws_resample_f32) against the project's host definition, restated in NumPy float64 by
_resample_ref.py with the library's own taps (kws_host_resample_design: what the device table holds).

Gates.  The kernel sums in float64, so an output may differ from the exact sum by the forward bound of a float64 dot product of
at most 256 terms in any order, with or without FMA: 2 * 256 * 2^-53 = 2^-44 times S = sum |x| |h| (the one pair with more terms
per output, 1/24 with 481, gets 2 * 481 * 2^-53 by the same rule: _resample_ref.dot_bound).  _f32 adds one rounding to
float32 (2^-24 |y|, or 2^-149 below the normal range); _i16 adds one rounding to an integer (0.5).  A kernel that accumulated in
float32 would miss the 2^-44 S term on a third of the outputs and more.  Every output row is over-allocated by one row that must
stay untouched."""
import functools
import wave

import numpy as np
import pytest
import torch

import _resample_ref as ref
import _scan_ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PAIR_IDS = list(ref.PAIRS)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def design(pair):
    rate_in, rate_out = ref.PAIRS[pair]
    up, down, half, tile, taps = _native.host_resample_design(rate_in, rate_out)
    assert (up, down) == ref.ratio(rate_in, rate_out) and tile >= 1
    return rate_in, rate_out, up, down, half, tile, taps


def run(ctx, x, rate_in, rate_out, n_out, lens=None):
    """Resample host ``x`` [R, n_in] (int16 or float32) into a prefilled buffer of R + 1 rows; the last one must not be written."""
    x = np.ascontiguousarray(np.atleast_2d(x))
    R = x.shape[0]
    d_in = torch.from_numpy(x).to(DEV)
    d_len = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    if x.dtype == np.int16:
        out = torch.full((R + 1, n_out), -12345, dtype=torch.int16, device=DEV)
        ctx.resample_i16(d_in, rate_in, rate_out, out[:R], d_len)
    else:
        out = torch.full((R + 1, n_out), float("nan"), dtype=torch.float32, device=DEV)
        ctx.resample_f32(d_in, rate_in, rate_out, out[:R], d_len)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[R] == -12345).all() if x.dtype == np.int16 else np.isnan(got[R]).all(), "written beyond [R, n_out]"
    return got[:R]


def check_f32(got, y, S, what, dot=ref.F64_DOT):
    assert np.isfinite(got).all(), f"{what}: an output was not written"
    err = np.abs(got.astype(np.float64) - y)
    tol = 2.0 ** -24 * np.abs(y) + dot * S + 2.0 ** -149
    print(f"[resample] {what} f32: worst err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all(), f"{what}: {(err > tol).sum()} of {err.size} outputs beyond the float64-sum gate, worst {(err / tol).max():.2f} x"


def check_i16(got, y, S, what, dot=ref.F64_DOT):
    want = np.clip(y, -32768.0, 32767.0)
    err = np.abs(got.astype(np.float64) - want)
    tol = 0.5 + dot * S
    assert (err <= tol).all(), f"{what}: {(err > tol).sum()} of {err.size} outputs beyond 0.5 + 2^-44 S, worst {err.max():.3f}"
    # exact wherever the reference itself decides the rounding: the fraction is farther from 1/2 than the float64 bound
    decided = np.abs(np.abs(want - np.floor(want)) - 0.5) > dot * S
    left_out = 1.0 - decided.mean()
    print(f"[resample] {what} i16: worst err {err.max():.4f}, share left out of the exact check {left_out:.1e}")
    assert left_out <= 1e-3
    assert np.array_equal(got[decided], ref.to_int16(y)[decided]), f"{what}: {(got != ref.to_int16(y))[decided].sum()} outputs are not rne(clip(y))"


def lengths_for(pair):
    """n_in values whose natural lengths sit at 1, 2, the wavefront edge and both sides of the tile edges, plus one shorter than
    half / up where every output is an edge output."""
    _, _, up, down, half, T, _ = design(pair)
    targets = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    return sorted({ref.n_in_for(n, up, down) for n in targets} | {max(1, half // up // 3)})


# ---- 1. values at every length --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIR_IDS)
def test_values_at_wavefront_and_tile_edges(ctx, pair):
    rate_in, rate_out, up, down, half, T, taps = design(pair)
    rng = np.random.default_rng(sum(map(ord, pair)))
    naturals = set()
    for n_in in lengths_for(pair):
        n_nat = ref.natural_len(n_in, up, down)
        assert n_nat == _native.host_resample_len(n_in, rate_in, rate_out)
        naturals.add(n_nat)
        xf = rng.uniform(-1, 1, n_in).astype(np.float32)
        xi = rng.integers(-32768, 32768, n_in, dtype=np.int16)
        for n_out in {n_nat, n_nat + 3, max(1, n_nat - 1)}:
            y, S = ref.resample_ref(xf, up, down, taps, n_out=n_out)
            got = run(ctx, xf, rate_in, rate_out, n_out)
            check_f32(got, y, S, f"{pair} n_in {n_in} n_out {n_out}", ref.dot_bound(up, down))
            assert (got[:, n_nat:] == 0).all()
            y, S = ref.resample_ref(xi, up, down, taps, n_out=n_out)
            got = run(ctx, xi, rate_in, rate_out, n_out)
            check_i16(got, y, S, f"{pair} n_in {n_in} n_out {n_out}", ref.dot_bound(up, down))
            assert (got[:, n_nat:] == 0).all()
    if down >= up:  # every natural length can be hit
        assert naturals >= {1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1}, naturals
    else:           # natural lengths are multiples of up / down: the cut-short n_out above puts the odd ones on the edges
        assert max(naturals) >= 2 * T + 1 and min(naturals) <= 2 * up


# ---- 2. an impulse reads the taps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIR_IDS)
def test_an_impulse_returns_the_taps_bit_for_bit(ctx, pair):
    rate_in, rate_out, up, down, half, T, taps = design(pair)
    n_in = ref.n_in_for(T + T // 2, up, down)
    n_out = ref.natural_len(n_in, up, down)
    k = np.arange(n_out, dtype=np.int64)
    for m0 in (0, ref.n_in_for(T // 2, up, down), n_in - 1):  # first sample, one whose outputs sit mid-tile, last sample
        x = np.zeros(n_in, np.float32)
        x[m0] = 1.0
        t = half + k * down - m0 * up
        want = np.where((t >= 0) & (t <= 2 * half), taps[np.clip(t, 0, 2 * half)], 0.0).astype(np.float32)
        assert np.count_nonzero(want) >= half // down - 1  # the sample's whole response, or the half of it inside the output
        got = run(ctx, x, rate_in, rate_out, n_out)[0]
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{pair} m0 {m0}: {(got != want).sum()} outputs differ from float32(h)"


# ---- 3. saturation --------------------------------------------------------------------------------------------------
def test_int16_overshoot_is_clamped_not_wrapped(ctx):
    rate_in, rate_out, up, down, half, T, taps = design("1/3")
    n_in = 4800
    x = np.where((np.arange(n_in) // 240) % 2 == 0, 32767, -32768).astype(np.int16)  # period 480 samples at 48 kHz
    y, S = ref.resample_ref(x, up, down, taps)
    assert 37000 < y.max() < 38000 and -38000 < y.min() < -37000, (y.max(), y.min())  # the reference overshoots to +-37 619
    got = run(ctx, x, rate_in, rate_out, y.shape[1])
    check_i16(got, y, S, "square wave")
    assert got.max() == 32767 and got.min() == -32768
    over = y[0] > 32767.5
    assert over.sum() > 10 and (got[0][over] == 32767).all() and (got[0][y[0] < -32768.5] == -32768).all()


# ---- 4. ragged batches, zeros beyond the natural length ---------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIR_IDS)
def test_ragged_batch(ctx, pair):
    rate_in, rate_out, up, down, half, T, taps = design(pair)
    n_in = ref.n_in_for(T + 70, up, down)
    lens = [n_in, 0, n_in // 2 + 1]
    rng = np.random.default_rng(5)
    xf = rng.uniform(-1, 1, (3, n_in)).astype(np.float32)   # rows 1 and 2 hold garbage at and beyond their lengths
    xi = rng.integers(-32768, 32768, (3, n_in), dtype=np.int16)
    nat = [ref.natural_len(L, up, down) for L in lens]
    for n_out in (nat[2] - 5, nat[0] + 9):  # below the natural lengths of rows 0 and 2, above all
        for x, check in ((xf, check_f32), (xi, check_i16)):
            y, S = ref.resample_ref(x, up, down, taps, d_len=lens, n_out=n_out)
            got = run(ctx, x, rate_in, rate_out, n_out, lens)
            check(got, y, S, f"{pair} ragged n_out {n_out}", ref.dot_bound(up, down))
            assert (got[1] == 0).all(), "a recording of length 0 must come out as zeros whatever its row holds"
            for r in range(3):
                assert (got[r, nat[r]:] == 0).all(), f"row {r}: outputs beyond the natural length {nat[r]} must be zero"
    # lengths outside [0, n_in] are clamped
    got = run(ctx, xi, rate_in, rate_out, nat[0], [n_in + 1000, -3, n_in // 2 + 1])
    want = run(ctx, xi, rate_in, rate_out, nat[0], lens)
    assert np.array_equal(got, want)


# ---- 5. an output depends on its own span alone -------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIR_IDS)
def test_position_independence(ctx, pair):
    rate_in, rate_out, up, down, half, T, taps = design(pair)
    n_in = ref.n_in_for(2 * T + 1, up, down)
    lens = [n_in, n_in // 3, n_in // 2 + 1]
    rng = np.random.default_rng(9)
    for x in (rng.uniform(-1, 1, (3, n_in)).astype(np.float32), rng.integers(-32768, 32768, (3, n_in), dtype=np.int16)):
        n_out = ref.natural_len(n_in, up, down)
        batch = run(ctx, x, rate_in, rate_out, n_out, lens)
        for r, L in enumerate(lens):
            nat = ref.natural_len(L, up, down)
            alone = run(ctx, x[r, :max(L, 1)], rate_in, rate_out, n_out, [L])  # R = 1, no padding behind the recording
            assert np.array_equal(batch[r].view(np.uint8), alone[0].view(np.uint8)), f"{pair} row {r}: differs from the recording alone"
            padded = np.concatenate([x[r, :L], np.full(777, 77, x.dtype)])    # another n_in, garbage in the padding
            other = run(ctx, padded, rate_in, rate_out, n_out, [L])
            assert np.array_equal(batch[r].view(np.uint8), other[0].view(np.uint8)), f"{pair} row {r}: depends on the padding"
            short = max(1, nat - T // 2 - 1)                                   # n_out cut short: another tile count
            cut = run(ctx, x[r], rate_in, rate_out, short, [L])
            assert np.array_equal(batch[r, :short].view(np.uint8), cut[0].view(np.uint8)), f"{pair} row {r}: depends on n_out"
        assert np.array_equal(batch, run(ctx, x, rate_in, rate_out, n_out, lens)), "two runs differ"


# ---- 6. equal rates, errors ------------------------------------------------------------------------------------------
def test_equal_rates_copy(ctx):
    rng = np.random.default_rng(2)
    n_in = 2500
    lens = [n_in, 0, 1301]
    for x in (rng.uniform(-1, 1, (3, n_in)).astype(np.float32), rng.integers(-32768, 32768, (3, n_in), dtype=np.int16)):
        for n_out in (1200, n_in, n_in + 1030):
            got = run(ctx, x, 22050, 22050, n_out, lens)
            want = np.zeros((3, n_out), x.dtype)
            for r, L in enumerate(lens):
                want[r, :min(L, n_out)] = x[r, :min(L, n_out)]
            assert np.array_equal(got, want)
        assert np.array_equal(run(ctx, x, 16000, 16000, n_in), x)


def test_argument_errors(ctx):
    x = torch.zeros((2, 100), dtype=torch.int16, device=DEV)
    out = torch.full((2, 40), -12345, dtype=torch.int16, device=DEV)
    fn = ctx._lib.kws_resample_i16

    def rc(d_in=x, R=2, n_in=100, rate_in=48000, rate_out=16000, d_out=out, n_out=40):
        p = lambda t: t.data_ptr() if t is not None else None
        return fn(ctx._h, p(d_in), R, n_in, None, rate_in, rate_out, p(d_out), n_out)

    for bad in (dict(d_in=None), dict(d_out=None), dict(R=0), dict(n_in=0), dict(n_out=0), dict(rate_in=0), dict(rate_out=-1)):
        assert rc(**bad) == _native.KWS_EINVAL, bad
    assert rc(rate_in=16001, rate_out=16000) == _native.KWS_EUNSUPPORTED  # 16001 / 16000 does not reduce below 1024
    assert rc(rate_in=1025, rate_out=1) == _native.KWS_EUNSUPPORTED
    assert "1024" in ctx._lib.kws_last_error(ctx._h).decode()
    torch.cuda.synchronize()
    assert (out == -12345).all(), "a refused call wrote its output"
    assert rc() == _native.KWS_OK
    torch.cuda.synchronize()
    assert (out[:, :34] == 0).all() and (out[:, 34:] == 0).all()  # zeros in, zeros out, beyond the natural length (34) too
    # timed under its own kernel id
    ctx.prof_enable(True)
    ctx.prof_reset()
    assert rc() == _native.KWS_OK
    ms, n = ctx.prof_read(_native.KWS_K_RESAMPLE)
    ctx.prof_enable(False)
    assert n == 1 and ms > 0


# ---- 7. end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spotter(e2e_golden):
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=12)
    model.load_state_dict(_scan_ref.state_from_blob(e2e_golden["he.blob"]))
    return KeywordSpotter(model)


def confident_clips(e2e_golden):
    """Golden clips whose top-2 margin under the `he` weights exceeds 1e-2, most confident first."""
    top = np.sort(e2e_golden["he.logits"][8:], axis=1)
    margin = top[:, -1] - top[:, -2]
    order = [int(i) for i in np.argsort(-margin) if margin[i] > 1e-2]
    assert len(order) >= 6
    return e2e_golden["clips"], order


def upsample_i16(pcm, rate_out, rate_in=16000):
    from kws.libs.audio_processor import resample_host

    return ref.to_int16(resample_host(pcm.astype(np.float64) * 0.7, rate_in, rate_out))  # headroom: no clipping in the fixture


def write_wav16(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def test_scan_at_another_rate(ctx, spotter, e2e_golden, tmp_path):
    from kws.common.errors import AudioProcessingError

    clips, order = confident_clips(e2e_golden)
    rec48 = upsample_i16(np.concatenate([clips[i] for i in order[:3]]), 48000)
    assert rec48.shape == (144000,)
    res = spotter.scan(rec48, hop_frames=5, smooth_window=3, threshold=0.15, refractory=4, sample_rate=48000)
    rec16 = torch.full((1, 48000), -12345, dtype=torch.int16, device=DEV)
    ctx.resample_i16(torch.from_numpy(rec48[None]).to(DEV), 48000, 16000, rec16)
    torch.cuda.synchronize()
    want = spotter.scan(rec16, hop_frames=5, smooth_window=3, threshold=0.15, refractory=4)
    assert res.logits.shape == want.logits.shape == (1, 41, 12)
    assert np.array_equal(res.logits, want.logits) and np.array_equal(res.labels, want.labels)
    assert np.array_equal(res.window_start_s, want.window_start_s) and res.events == want.events  # seconds of the recording
    same_rate = spotter.scan(rec16, hop_frames=5, sample_rate=16000)  # the configured rate: nothing to resample
    assert np.array_equal(same_rate.logits, want.logits)
    path = tmp_path / "rec48.wav"
    write_wav16(path, rec48, 48000)
    from_file = spotter.scan_file(str(path), resample=True, hop_frames=5, smooth_window=3, threshold=0.15, refractory=4)
    assert np.array_equal(from_file.logits, res.logits) and from_file.events == res.events
    with pytest.raises(AudioProcessingError, match="sample rate 48000 != 16000; resampling is not implemented"):
        spotter.scan_file(str(path), hop_frames=5)
    # a float file at another rate: refused, with the reason
    import struct

    body = rec48[:48000].astype("<f4") / np.float32(32768)
    fmt = struct.pack("<HHIIHH", 3, 1, 48000, 48000 * 4, 4, 32)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", body.nbytes) + body.tobytes()
    (tmp_path / "f32.wav").write_bytes(b"RIFF" + struct.pack("<I", len(riff)) + riff)
    with pytest.raises(AudioProcessingError, match="not 16-bit mono"):
        spotter.scan_file(str(tmp_path / "f32.wav"), resample=True)


def test_infer_files_on_the_device(spotter, e2e_golden, tmp_path):
    """A mixed list -- 16 kHz int16, 48 kHz int16, 8 kHz float32, unequal lengths -- gets, per file, the label of infer_pcm16 /
    infer_f32 on the reference-resampled, fix_length-ed clip."""
    import struct

    from kws.libs.audio_processor import fix_length, resample_host

    clips, order = confident_clips(e2e_golden)
    a, b, c, d = (clips[i] for i in order[:4])
    files, want_clips = [], []
    # 16 kHz int16, short: padded
    write_wav16(tmp_path / "a16.wav", a[:12000], 16000)
    files.append(tmp_path / "a16.wav")
    want_clips.append(fix_length(a[:12000], 16000))
    # 48 kHz int16, longer than a clip once resampled: cut; and a second, shorter one in the same group
    for name, pcm in (("b48", upsample_i16(np.concatenate([b, c[:500]]), 48000)), ("d48", upsample_i16(d[:15000], 48000))):
        write_wav16(tmp_path / f"{name}.wav", pcm, 48000)
        files.append(tmp_path / f"{name}.wav")
        y, _ = ref.resample_ref(pcm, 1, 3, _native.host_resample_design(48000, 16000)[4])
        want_clips.append(fix_length(ref.to_int16(y[0]), 16000))
    # 8 kHz float32, 7000 samples: 14000 after resampling, padded
    x8 = resample_host(c.astype(np.float64) / 32768.0, 16000, 8000)[:7000].astype(np.float32)
    fmt = struct.pack("<HHIIHH", 3, 1, 8000, 8000 * 4, 4, 32)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", x8.nbytes) + x8.astype("<f4").tobytes()
    (tmp_path / "c8.wav").write_bytes(b"RIFF" + struct.pack("<I", len(riff)) + riff)
    files.append(tmp_path / "c8.wav")
    y, _ = ref.resample_ref(x8, 2, 1, _native.host_resample_design(8000, 16000)[4])
    want_clips.append(fix_length(y[0].astype(np.float32), 16000))

    want = []
    for clip in want_clips:
        labels, logits = spotter.infer_pcm16(clip[None]) if clip.dtype == np.int16 else spotter.infer_f32(clip[None])
        top = np.sort(logits[0])
        assert top[-1] - top[-2] > 1e-3, "the fixture: the expected clip's own decision must be clear"
        want.append(int(labels[0]))
    order_in = [3, 0, 2, 1]  # the callers' order is not the groups' order
    got = spotter.infer_files([str(files[i]) for i in order_in], resample="device")
    assert [g[0] for g in got] == [want[i] for i in order_in]
    assert all(word == spotter.words[idx] for idx, word in got)
    # the existing routes still answer for what they serve
    assert spotter.infer_files([str(files[0])])[0][0] == want[0]
    with pytest.raises(Exception, match="resample"):
        spotter.infer_files([str(files[0])], resample="host")
