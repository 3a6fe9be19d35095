"""Batches of float32 recordings of unequal length on the GPU (kws_frames_ragged_f32, kws_scan_ragged_f32).

Every comparison is np.array_equal on the words against the equal-length float entry run on each recording alone, and -- for
samples on the int16 grid -- against the int16 ragged entry.  The gaps of the packed buffer and the tail after the last
recording are NaN: one sample read past a recording's end as part of it turns its frames into NaN.  Output buffers are prefilled
with NaN / -1 and over-allocated by one row."""
import numpy as np
import pytest
import torch

import _scan_ref as sref
from _f32_ref import n_for_frames, unit
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
T_WIN, N_CEP, FRAME_LEN, FRAME_STEP = sref.T_WIN, sref.N_CEP, sref.FRAME_LEN, sref.FRAME_STEP
u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)

# the edge lengths of tests/test_scan_f32_gpu.py as ONE batch, and the batch of more than 4096 chunks (two chunks per wavefront)
EDGE_LENGTHS = [1, 399, 400, 401, 560, 16000, 16001, 16007, 16008, n_for_frames(19), n_for_frames(20, 3), n_for_frames(21),
                n_for_frames(22, 150), 48000]
TWO_CHUNK_LENGTHS = [n_for_frames(4 * 4097), n_for_frames(19), n_for_frames(20), n_for_frames(21, 5), n_for_frames(28), n_for_frames(33, 1), 16001]


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


def recordings(lengths, seed):
    """int16 recordings (so that the grid property can be asked): noise, and a tone near the top of the band on the second-long
    ones with an odd index (frames for the refinement)."""
    rng = np.random.default_rng(seed)
    recs = [np.round(rng.normal(0.0, 2500.0, n)).clip(-32768, 32767).astype(np.int16) for n in lengths]
    for i, n in enumerate(lengths):
        if 16000 <= n <= 48000 and i % 2:
            recs[i] = np.round(20000 * np.sin(2 * np.pi * 7900.0 * np.arange(n) / 16000.0)).astype(np.int16)
    return recs


def place(recs, layout, dtype):
    """Recordings -> (device buffer [n], start int64 [R], length int32 [R]).  float32: the buffer is NaN wherever no recording
    lies; int16: +-32767 sentinels.  'packed': each start the next multiple of 8 that leaves at least one gap sample; 'rect':
    rows of equal pitch, eight gap samples ahead of the first."""
    length = np.array([len(x) for x in recs], np.int32)
    up8 = lambda n: (n + 7) & ~7
    if layout == "packed":
        start, at = [], 8
        for n in length:
            start.append(at)
            at = up8(at + int(n) + 1)
        n_buf = at + 8
    else:
        pitch = up8(int(length.max()) + 1)
        start = [8 + r * pitch for r in range(len(recs))]
        n_buf = 8 + len(recs) * pitch
    if dtype == np.float32:
        buf = np.full(n_buf, np.nan, np.float32)
    else:
        buf = np.where(np.arange(n_buf) % 2 == 0, 32767, -32767).astype(np.int16)
    for s, x in zip(start, recs):
        buf[s:s + len(x)] = x
    for s, n in zip(start, length):
        gap = (buf[s - 1], buf[s + n])
        assert all(np.isnan(g) for g in gap) if dtype == np.float32 else all(abs(int(g)) == 32767 for g in gap)
    return torch.from_numpy(buf).to(DEV), np.array(start, np.int64), length


def frames_alone(ctx, x):
    F, _ = sref.scan_shape(len(x), 1)
    before = ctx.frontend_stats()
    feat = torch.full((2, F, N_CEP), float("nan"), device=DEV)
    ctx.frames_f32(torch.from_numpy(np.ascontiguousarray(x)).to(DEV)[None], feat[:1])
    torch.cuda.synchronize()
    after = ctx.frontend_stats()
    assert torch.isnan(feat[1]).all()
    return feat[0].cpu().numpy(), (after[0] - before[0], after[1] - before[1])


def frames_ragged(ctx, buf, start, length, row_multiple, f32=True):
    frames, frame_off, _, _, _ = _native.host_ragged_plan(length, FRAME_LEN, FRAME_STEP, T_WIN, row_multiple)
    F_pack = int(frame_off[-1])
    before = ctx.frontend_stats()
    feat = torch.full((F_pack + 1, N_CEP), float("nan"), device=DEV)
    (ctx.frames_ragged_f32 if f32 else ctx.frames_ragged_i16)(buf, start, length, row_multiple, feat[:F_pack])
    torch.cuda.synchronize()
    after = ctx.frontend_stats()
    assert torch.isnan(feat[F_pack]).all(), "frames were written beyond [F_pack, numcep]"
    return feat[:F_pack].cpu().numpy(), frames, frame_off, (after[0] - before[0], after[1] - before[1])


def check_frames(got, frames, frame_off, alone):
    for r, want in enumerate(alone):
        o, F = int(frame_off[r]), int(frames[r])
        assert want.shape[0] == F
        bad = (u32(got[o:o + F]) != u32(want)).any(axis=1)
        assert not bad.any(), f"recording {r} ({F} frames): frames {np.flatnonzero(bad)[:8]} differ from kws_frames_f32 alone"
        assert (u32(got[o + F:int(frame_off[r + 1])]) == 0).all(), f"recording {r}: the rounding rows are not zero"


@pytest.mark.parametrize("refine", [True, False], ids=["refine", "norefine"])
def test_float_frames_equal_each_recording_alone_and_the_int16_batch(ctx, refine):
    recs = recordings(EDGE_LENGTHS, 5)
    off_grid = [unit(x) * np.float32(0.77) for x in recs]
    ctx.set_frontend_refine(_native.FE_REFINE_SPAN_DEFAULT if refine else 0.0)
    try:
        for samples, grid in ((off_grid, False), ([unit(x) for x in recs], True)):
            singles = [frames_alone(ctx, x) for x in samples]
            alone = [s[0] for s in singles]
            assert not any(np.isnan(a).any() for a in alone)
            counted, refined = sum(s[1][0] for s in singles), sum(s[1][1] for s in singles)
            assert (refined > 0) == refine, "the refinement leg is vacuous"
            for layout, row_multiple in (("packed", 1), ("rect", 7)):
                buf, start, length = place(samples, layout, np.float32)
                got, frames, frame_off, delta = frames_ragged(ctx, buf, start, length, row_multiple)
                check_frames(got, frames, frame_off, alone)
                assert delta == (counted, refined), "kws_frontend_stats differs from the per-recording calls' sum"
                if grid:
                    ibuf, istart, ilength = place(recs, layout, np.int16)
                    want, _, _, idelta = frames_ragged(ctx, ibuf, istart, ilength, row_multiple, f32=False)
                    assert np.array_equal(u32(got), u32(want)), "kws_frames_ragged_f32(pcm / 32768) differs from kws_frames_ragged_i16(pcm)"
                    assert delta == idelta
    finally:
        ctx.set_frontend_refine(_native.FE_REFINE_SPAN_DEFAULT)


def test_float_frames_with_two_chunks_per_wavefront(ctx):
    recs = [unit(x) * np.float32(1.3) for x in recordings(TWO_CHUNK_LENGTHS, 6)]
    alone = [frames_alone(ctx, x)[0] for x in recs]
    buf, start, length = place(recs, "packed", np.float32)
    got, frames, frame_off, _ = frames_ragged(ctx, buf, start, length, 1)
    check_frames(got, frames, frame_off, alone)


@pytest.mark.parametrize("hop", [1, 7])
def test_float_scan_equals_each_recording_alone(ctx, clips, hop):
    lengths = [n_for_frames(T_WIN), 40000, 8000, 33333, n_for_frames(T_WIN + 1, 7), 399]
    recs = [unit(sref.mixed_recordings(1, n, clips, seed=20 + i)[0]) * np.float32(0.9) for i, n in enumerate(lengths)]
    buf, start, length = place(recs, "packed" if hop == 1 else "rect", np.float32)
    _, frame_off, windows, win_off, W_pack = _native.host_ragged_plan(length, FRAME_LEN, FRAME_STEP, T_WIN, hop)
    logits = torch.full((W_pack + 1, C), float("nan"), device=DEV)
    labels = torch.full((W_pack + 1,), -1, dtype=torch.int32, device=DEV)
    ctx.scan_ragged_f32(buf, start, length, hop, logits[:W_pack], labels[:W_pack])
    torch.cuda.synchronize()
    assert torch.isnan(logits[W_pack]).all() and int(labels[W_pack]) == -1, "written beyond the packed windows"
    logits, labels = logits.cpu().numpy(), labels.cpu().numpy()
    assert [int(w) for w in windows] == [sref.scan_shape(n, hop)[1] for n in lengths] and windows[2] == 0 and windows[0] == 1
    for r, rec in enumerate(recs):
        W, o = int(windows[r]), int(win_off[r])
        if W == 0:
            continue  # kws_scan_f32 refuses a recording shorter than a window
        want_logits = torch.full((1, W, C), float("nan"), device=DEV)
        want_labels = torch.full((1, W), -1, dtype=torch.int32, device=DEV)
        ctx.scan_f32(torch.from_numpy(rec).to(DEV)[None], hop, want_logits, want_labels)
        torch.cuda.synchronize()
        assert np.array_equal(u32(logits[o:o + W]), u32(want_logits[0].cpu().numpy())), f"recording {r}: logits differ from kws_scan_f32 alone"
        assert np.array_equal(labels[o:o + W], want_labels[0].cpu().numpy())


def test_the_rectangular_output_of_kws_resample_f32_is_accepted(ctx):
    rng = np.random.default_rng(8)
    n_in = [48000, 31111, 7000]
    src = np.zeros((3, max(n_in)), np.float32)
    for r, n in enumerate(n_in):
        src[r, :n] = rng.normal(0.0, 0.1, n)
    length = np.array([_native.host_resample_len(n, 48000, 16000) for n in n_in], np.int32)
    n_out = (int(length.max()) + 7) & ~7
    out = torch.full((3, n_out), float("nan"), device=DEV)
    ctx.resample_f32(torch.from_numpy(src).to(DEV), 48000, 16000, out, torch.tensor(n_in, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    start = np.arange(3, dtype=np.int64) * n_out
    got, frames, frame_off, _ = frames_ragged(ctx, out, start, length, 1)
    check_frames(got, frames, frame_off, [frames_alone(ctx, host[r, :length[r]])[0] for r in range(3)])


def test_ragged_f32_refusals_launch_nothing(ctx):
    buf = torch.zeros((40008,), dtype=torch.float32, device=DEV)
    feat = torch.full((400, N_CEP), float("nan"), device=DEV)
    logits = torch.full((200, C), float("nan"), device=DEV)
    lib, h = ctx._lib, ctx._h
    i64 = lambda v: np.array(v, np.int64).ctypes.data_as(_native._h_i64p)
    i32 = lambda v: np.array(v, np.int32).ctypes.data_as(_native._h_i32p)

    def frames(ptr=buf.data_ptr(), n=40008, start=(8,), length=(20000,), R=1, rm=1, out=feat.data_ptr(), c=ctx):
        return c._lib.kws_frames_ragged_f32(c._h, ptr, n, i64(start), i32(length), R, rm, out)

    def scan(ptr=buf.data_ptr(), start=(8,), hop=1, out=logits.data_ptr()):
        return lib.kws_scan_ragged_f32(h, ptr, 40008, i64(start), i32((20000,)), 1, hop, out, None, None)

    assert frames(ptr=buf.data_ptr() + 4) == _native.KWS_EINVAL  # off a 16-byte boundary
    assert "d_wav must be 16-byte aligned" in lib.kws_last_error(h).decode()
    assert frames(start=(4,)) == _native.KWS_EINVAL               # start % 8 != 0
    assert frames(start=(20016,)) == _native.KWS_EINVAL           # runs past n_wav
    assert frames(length=(0,)) == _native.KWS_EINVAL
    assert frames(ptr=None) == _native.KWS_EINVAL and frames(out=None) == _native.KWS_EINVAL and frames(rm=0) == _native.KWS_EINVAL
    assert scan(ptr=buf.data_ptr() + 4) == _native.KWS_EINVAL and scan(start=(4,)) == _native.KWS_EINVAL
    assert scan(hop=0) == _native.KWS_EINVAL and scan(out=None) == _native.KWS_EINVAL
    ctx.set_frontend_math(_native.FE_F64)
    try:
        assert frames() == _native.KWS_EUNSUPPORTED and scan() == _native.KWS_EUNSUPPORTED
    finally:
        ctx.set_frontend_math(_native.FE_F32)
    other = _native.Context(0)
    try:
        other.use_torch_stream()
        other.set_frontend(frame_len=480, nfft=512)  # outside (384, 448]: not the wavefront-resident kernel's geometry
        assert frames(c=other) == _native.KWS_EUNSUPPORTED
    finally:
        other.close()
    torch.cuda.synchronize()
    assert torch.isnan(feat).all() and torch.isnan(logits).all(), "a refused call wrote results"
    assert frames() == _native.KWS_OK
