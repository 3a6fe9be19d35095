"""The streaming resampler (kws_stream_resample_*, kws_stream_push_rate_i16 / kws_stream_push_host_rate_i16, StreamingSpotter(
input_rate=...)) on the device.

The gate is equality: whatever the chunking, the concatenated outputs of a stream are the bits kws_resample_i16 gives the whole
signal, front-padded by down * z zeros and read from up * z - d on (the d pre-ringing outputs included) -- an output's bits
depend on its own input span and the rate pair alone.  Beside that every output is within 0.5 + dot_bound * S of the NumPy
float64 definition (_resample_ref: S = sum |x| |h|, one rounding to an integer), which leaves nothing out.  Output buffers carry
a guard row and guard columns that must stay untouched."""
import functools

import numpy as np
import pytest
import torch

import _resample_ref as ref
import _resample_stream_ref as sref
import _scan_ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = -12345
# pair -> max_in: large enough that a push of max_in samples yields more than 1024 outputs per stream (several workgroups per
# stream) wherever history + max_in <= 6144 allows it (1/12: 416, 1/24: 235 outputs at the limit)
MAX_IN = {"1/3": 3500, "2/1": 1100, "160/441": 3000, "1/12": 5000, "1/24": 5641}
HOP_IN = {"1/3": 480, "2/1": 80, "160/441": 441, "1/12": 1920, "1/24": 3840}  # 160 output samples


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def design(pair):
    rate_in, rate_out = ref.PAIRS[pair]
    up, down, delay, history = _native.host_stream_resample_plan(rate_in, rate_out)
    taps = _native.host_resample_design(rate_in, rate_out)[4]
    return rate_in, rate_out, up, down, delay, history, taps


def batch_window(ctx, x, pair, n_total):
    """kws_resample_i16 of x [S, N] front-padded by down * z zeros, read at [up z - d, up z - d + n_total)."""
    rate_in, rate_out, up, down, delay, _, _ = design(pair)
    z = -(-delay // up)
    padded = np.concatenate([np.zeros((x.shape[0], down * z), np.int16), x], axis=1)
    lo = up * z - delay
    out = torch.full((x.shape[0], lo + n_total), GUARD, dtype=torch.int16, device=DEV)
    ctx.resample_i16(torch.from_numpy(padded).to(DEV), rate_in, rate_out, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, lo:]


def stream_run(ctx, x, rates, max_in, sizes, first_sample=0, reopen=True):
    """Push x [S, N] through the streaming resampler in chunks of ``sizes`` (cycled; the last chunk is what is left) ->
    int16 [S, floor(N up / down)].  Checks every push's n_out against the host count and the guards of every output buffer."""
    S, N = x.shape
    rate_in, rate_out = rates
    up, down = ref.ratio(rate_in, rate_out)
    if reopen:
        ctx.stream_resample_open(S, rate_in, rate_out, max_in, first_sample)
    plan, at, i = [], 0, 0
    while at < N:
        n = min(sizes[i % len(sizes)], N - at)
        plan.append((at, n))
        at, i = at + n, i + 1
    out_cap = max(n for _, n in plan) * up // down + 2
    # chunk-major copy of the input so that a push reads a contiguous [S, n] block without a copy kernel per push
    blocks = torch.from_numpy(np.concatenate([x[:, a:a + n].reshape(-1) for a, n in plan])).to(DEV)
    outs = torch.full((len(plan), S + 1, out_cap), GUARD, dtype=torch.int16, device=DEV)
    counts, off = [], 0
    for p, (a, n) in enumerate(plan):
        chunk = blocks[off:off + S * n].view(S, n)
        off += S * n
        got = ctx.stream_resample_i16(chunk, outs[p, :S])
        assert got == _native.host_stream_resample_count(rate_in, rate_out, first_sample + a, n) == sref.count(first_sample + a, n, up, down)
        counts.append(got)
    torch.cuda.synchronize()
    host = outs.cpu().numpy()
    assert (host[:, S] == GUARD).all(), "written beyond the S rows"
    pieces = []
    for p, c in enumerate(counts):
        assert (host[p, :S, c:] == GUARD).all(), f"push {p}: written beyond its {c} outputs"
        pieces.append(host[p, :S, :c])
    y = np.concatenate(pieces, axis=1)
    assert y.shape[1] == N * up // down
    return y


# ---- 1. chunking ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", list(MAX_IN))
def test_any_chunking_gives_the_batch_bits(ctx, pair):
    rate_in, rate_out, up, down, delay, history, taps = design(pair)
    max_in, hop_in = MAX_IN[pair], HOP_IN[pair]
    assert history + max_in <= 6144 and hop_in * up == 160 * down
    S, N = 3, 3 * max_in + 17
    rng = np.random.default_rng(sum(map(ord, pair)))
    x = rng.integers(-16384, 16384, (S, N)).astype(np.int16)  # half scale: nothing clips
    n_total = N * up // down
    want = batch_window(ctx, x, pair, n_total)
    y, sabs = sref.batch_window(x, up, down, taps, delay, -(-delay // up), n_total)
    assert np.abs(y[:, :delay]).max() > 0, "the pre-ringing before the onset is part of the comparison"
    tol = 0.5 + ref.dot_bound(up, down) * sabs
    tiles = set()
    for size in (1, 2, 63, 64, 65, hop_in, hop_in + 1, max_in):
        got = stream_run(ctx, x, (rate_in, rate_out), max_in, [size])
        tiles.add(-(-(size * up // down) // 1024))
        assert np.array_equal(got, want), f"{pair} chunks of {size}: {(got != want).sum()} of {got.size} outputs differ from kws_resample_i16"
        err = np.abs(got.astype(np.float64) - y)
        assert (err <= tol).all(), f"{pair} chunks of {size}: worst error {err.max():.4f} beyond 0.5 + dot_bound * S"
    print(f"[stream-resample] {pair}: workgroups per stream seen {sorted(tiles)}")
    if pair in ("1/3", "2/1", "160/441"):
        assert max(tiles) >= 2, "the largest push must span several workgroups per stream"
    # mixed sizes in one run, zero-output pushes included
    got = stream_run(ctx, x, (rate_in, rate_out), max_in, [1, hop_in, 65, 2, max_in, 63, hop_in + 1, 64])
    assert np.array_equal(got, want)


# ---- 2. streams are independent ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def independent_signals():
    return np.random.default_rng(77).integers(-16384, 16384, (257, 1700)).astype(np.int16)


@pytest.fixture(scope="module")
def alone(ctx):
    """Every signal through an S = 1 resampler of its own."""
    x = independent_signals()
    return np.concatenate([stream_run(ctx, x[s:s + 1], (48000, 16000), 600, [480, 7, 600]) for s in range(x.shape[0])])


@pytest.mark.parametrize("S", [1, 5, 64, 257])
def test_streams_are_independent(ctx, alone, S):
    x = independent_signals()[:S]
    got = stream_run(ctx, x, (48000, 16000), 600, [480, 7, 600])
    assert np.array_equal(got, alone[:S]), f"rows {sorted(set(np.nonzero((got != alone[:S]).any(axis=1))[0]))[:8]} differ from their S = 1 runs"
    assert len({row.tobytes() for row in got}) == S


# ---- 3. position ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["1/3", "160/441", "2/1"])
def test_a_start_beyond_2_to_the_40_gives_the_bits_of_a_start_at_zero(ctx, pair):
    rate_in, rate_out, up, down, delay, history, taps = design(pair)
    x = np.random.default_rng(3).integers(-16384, 16384, (2, 2500)).astype(np.int16)
    sizes = [HOP_IN[pair], 1, 65, HOP_IN[pair] + 1]
    zero = stream_run(ctx, x, (rate_in, rate_out), 1000, sizes)
    first = down * -(-2 ** 40 // down)
    assert first >= 2 ** 40 and first % down == 0
    far = stream_run(ctx, x, (rate_in, rate_out), 1000, sizes, first_sample=first)
    assert np.array_equal(far, zero)
    if down > 1:
        rc = ctx._lib.kws_stream_resample_open(ctx._h, 2, rate_in, rate_out, 1000, first + 1)
        assert rc == _native.KWS_EINVAL and "multiple of down" in ctx._lib.kws_last_error(ctx._h).decode()
        # the refused open left the state alone: the streams go on where they were
        more = np.random.default_rng(4).integers(-16384, 16384, (2, 700)).astype(np.int16)
        both = stream_run(ctx, np.concatenate([x, more], axis=1), (rate_in, rate_out), 1000, sizes)
        cont = stream_run(ctx, x, (rate_in, rate_out), 1000, sizes, first_sample=first)
        assert ctx._lib.kws_stream_resample_open(ctx._h, 2, rate_in, rate_out, 1000, 1) == _native.KWS_EINVAL
        n0 = x.shape[1]
        d_more = torch.from_numpy(more).to(DEV)
        out = torch.full((2, 700 * up // down + 2), GUARD, dtype=torch.int16, device=DEV)
        n = ctx.stream_resample_i16(d_more, out)
        torch.cuda.synchronize()
        assert n == (n0 + 700) * up // down - n0 * up // down
        assert np.array_equal(out.cpu().numpy()[:, :n], both[:, cont.shape[1]:])


# ---- 4. clamp -------------------------------------------------------------------------------------------------------------
def test_overshoot_is_clamped_like_the_batch_kernel(ctx):
    n_in = 4800
    x = np.where((np.arange(n_in) // 240) % 2 == 0, 32767, -32768).astype(np.int16)[None]  # the reference overshoots to +-37 619
    want = batch_window(ctx, x, "1/3", n_in // 3)
    got = stream_run(ctx, x, (48000, 16000), 500, [480, 481, 1])
    assert np.array_equal(got, want)
    assert got.max() == 32767 and got.min() == -32768 and (got == 32767).sum() > 10 and (got == -32768).sum() > 10


# ---- 5. lifecycle and errors ------------------------------------------------------------------------------------------------
def test_reopen_close_and_equal_rates(ctx):
    x = np.random.default_rng(8).integers(-16384, 16384, (2, 1000)).astype(np.int16)
    first = stream_run(ctx, x, (48000, 16000), 500, [480])
    cont = stream_run(ctx, x, (48000, 16000), 500, [480], reopen=False)  # the same samples behind a history that is not zero
    assert not np.array_equal(cont[:, :20], first[:, :20])
    again = stream_run(ctx, x, (48000, 16000), 500, [480])  # a reopen zeroes the history and the position
    assert np.array_equal(again, first)
    ctx.stream_resample_close()
    d_in = torch.zeros((2, 480), dtype=torch.int16, device=DEV)
    out = torch.full((2, 200), GUARD, dtype=torch.int16, device=DEV)
    n = _native.C.c_int(-7)
    fn = ctx._lib.kws_stream_resample_i16
    assert fn(ctx._h, d_in.data_ptr(), 480, out.data_ptr(), 200, _native.C.byref(n)) == _native.KWS_ESTATE
    ctx.stream_resample_close()  # closing twice is fine
    # equal rates: a copy without delay, any chunk size, no LDS limit
    plan = _native.host_stream_resample_plan(22050, 22050)
    assert plan == (1, 1, 0, 0)
    big = np.random.default_rng(9).integers(-32768, 32768, (3, 20000)).astype(np.int16)
    got = stream_run(ctx, big, (22050, 22050), 8000, [8000, 1, 1025])
    assert np.array_equal(got, big)
    torch.cuda.synchronize()
    assert (out == GUARD).all() and n.value == -7


def test_argument_errors(ctx):
    lib, h, Ct = ctx._lib, ctx._h, _native.C
    op = lib.kws_stream_resample_open
    assert op(None, 2, 48000, 16000, 480, 0) == _native.KWS_EINVAL
    for bad in ((0, 48000, 16000, 480, 0), (2, 48000, 16000, 0, 0), (2, 0, 16000, 480, 0), (2, 48000, -1, 480, 0), (2, 48000, 16000, 480, 4)):
        assert op(h, *bad) == _native.KWS_EINVAL, bad
    assert op(h, 2, 16001, 16000, 480, 0) == _native.KWS_EUNSUPPORTED and op(h, 2, 1025, 1, 480, 0) == _native.KWS_EUNSUPPORTED
    assert "1024" in lib.kws_last_error(h).decode()
    history = _native.host_stream_resample_plan(48000, 16000)[3]
    assert op(h, 2, 48000, 16000, 6144, 0) == _native.KWS_EUNSUPPORTED  # history + max_in beyond what a workgroup stages
    assert op(h, 2, 48000, 16000, 6144 - history + 1, 0) == _native.KWS_EUNSUPPORTED
    assert op(h, 2, 48000, 16000, 6144 - history, 0) == _native.KWS_OK
    assert op(h, 2, 48000, 16000, 480, 0) == _native.KWS_OK
    d_in = torch.zeros((2, 481), dtype=torch.int16, device=DEV)
    out = torch.full((2, 200), GUARD, dtype=torch.int16, device=DEV)
    n = Ct.c_int(-7)
    fn = lib.kws_stream_resample_i16
    assert fn(None, d_in.data_ptr(), 480, out.data_ptr(), 200, Ct.byref(n)) == _native.KWS_EINVAL
    assert fn(h, None, 480, out.data_ptr(), 200, Ct.byref(n)) == _native.KWS_EINVAL
    assert fn(h, d_in.data_ptr(), 480, None, 200, Ct.byref(n)) == _native.KWS_EINVAL
    assert fn(h, d_in.data_ptr(), 480, out.data_ptr(), 200, None) == _native.KWS_EINVAL
    assert fn(h, d_in.data_ptr(), 0, out.data_ptr(), 200, Ct.byref(n)) == _native.KWS_EINVAL
    assert fn(h, d_in.data_ptr(), 481, out.data_ptr(), 200, Ct.byref(n)) == _native.KWS_EINVAL  # beyond max_in
    assert fn(h, d_in.data_ptr(), 480, out.data_ptr(), 159, Ct.byref(n)) == _native.KWS_EINVAL  # out_cap below the 160 it emits
    assert n.value == -7
    torch.cuda.synchronize()
    assert (out == GUARD).all(), "a refused push wrote its output"
    # the refused pushes touched nothing: the next one is the first push of a fresh stream
    assert fn(h, d_in.data_ptr(), 480, out.data_ptr(), 200, Ct.byref(n)) == _native.KWS_OK and n.value == 160
    assert fn(h, d_in.data_ptr(), 1, out.data_ptr(), 200, Ct.byref(n)) == _native.KWS_OK and n.value == 0
    assert fn(h, d_in.data_ptr(), 2, out.data_ptr(), 200, Ct.byref(n)) == _native.KWS_OK and n.value == 1
    ctx.stream_resample_close()


# ---- 6. the fused push -------------------------------------------------------------------------------------------------------
def live_signal(e2e_golden, rate, n_samples, S=5):
    """S different streams of golden speech, upsampled to ``rate`` on the host with headroom."""
    from kws.libs.audio_processor import resample_host

    clips = e2e_golden["clips"]
    rows = []
    for s in range(S):
        pcm = np.concatenate([clips[(3 * s + i) % len(clips)] for i in range(2)]).astype(np.float64) * 0.7
        rows.append(ref.to_int16(resample_host(pcm, 16000, rate))[:n_samples])
    return np.stack(rows)


def model_ctx(e2e_golden, S, rate=None, max_in=0):
    c = _native.Context(0)
    c.use_torch_stream()
    c.load_dscnn(e2e_golden["he.blob"], 12)
    c.stream_open(S)
    if rate:
        c.stream_resample_open(S, rate, 16000, max_in)
    return c


@pytest.mark.parametrize("rate,hop_in", [(48000, 480), (44100, 441)])
def test_fused_push_equals_resample_then_push(e2e_golden, rate, hop_in):
    S, hops, Cn = 5, 120, 12
    x = live_signal(e2e_golden, rate, hops * hop_in)
    assert x.shape == (S, hops * hop_in)
    d_x = torch.from_numpy(np.ascontiguousarray(x.reshape(S, hops, hop_in).transpose(1, 0, 2))).to(DEV)  # [hops, S, hop_in]
    fused, split, host = (model_ctx(e2e_golden, S, rate, hop_in + 8) for _ in range(3))
    try:
        lg = torch.zeros((2, hops, S, Cn), dtype=torch.float32, device=DEV)
        lb = torch.full((2, hops, S), -1, dtype=torch.int32, device=DEV)
        hop = torch.full((S, 160), GUARD, dtype=torch.int16, device=DEV)
        host_lg, host_lb = np.zeros((hops, S, Cn), np.float32), np.zeros((hops, S), np.int32)
        odd = torch.zeros((S, hop_in + 3), dtype=torch.int16, device=DEV)
        odd_host = np.zeros((S, hop_in + 3), np.int16)
        for t in range(hops):
            if t == 60:  # a push that would emit 161 (159) samples is refused and touches nothing
                for n_in in (hop_in + 3, hop_in - 3):
                    rc = fused._lib.kws_stream_push_rate_i16(fused._h, odd.data_ptr(), n_in, lg[0, t].data_ptr(), lb[0, t].data_ptr())
                    assert rc == _native.KWS_EINVAL and "a hop is 160" in fused._lib.kws_last_error(fused._h).decode()
                    pl, py = _native.C.c_void_p(), _native.C.c_void_p()
                    rc = host._lib.kws_stream_push_host_rate_i16(host._h, odd_host.ctypes.data, n_in, _native.C.byref(pl), _native.C.byref(py))
                    assert rc == _native.KWS_EINVAL
            fused.stream_push_rate_i16(d_x[t], lg[0, t], lb[0, t])
            assert split.stream_resample_i16(d_x[t], hop) == 160
            split.stream_push_i16(hop, lg[1, t], lb[1, t])
            h_lg, h_lb = host.stream_push_host_rate_i16(np.ascontiguousarray(x[:, t * hop_in:(t + 1) * hop_in]), S)
            host_lg[t], host_lb[t] = h_lg, h_lb
        torch.cuda.synchronize()
        rings = []
        for c in (fused, split, host):
            ring = torch.zeros((S, 99, 10), dtype=torch.float32, device=DEV)
            c.stream_copy_features(ring)
            assert c.stream_state()[1] == hops
            rings.append(ring.cpu().numpy())
        lg, lb = lg.cpu().numpy(), lb.cpu().numpy()
        assert np.isfinite(lg).all() and np.abs(lg[1, -1]).max() > 0
        assert np.array_equal(lg[0].view(np.uint32), lg[1].view(np.uint32)) and np.array_equal(lb[0], lb[1])
        assert np.array_equal(host_lg.view(np.uint32), lg[0].view(np.uint32)) and np.array_equal(host_lb, lb[0])
        assert np.array_equal(rings[0], rings[1]) and np.array_equal(rings[0], rings[2]) and np.abs(rings[0]).max() > 0
    finally:
        for c in (fused, split, host):
            c.close()


def test_fused_push_state_errors(e2e_golden):
    S = 3
    d_in = torch.zeros((S, 480), dtype=torch.int16, device=DEV)
    lg = torch.zeros((S, 12), dtype=torch.float32, device=DEV)
    lb = torch.zeros((S,), dtype=torch.int32, device=DEV)
    c = _native.Context(0)
    c.use_torch_stream()
    try:
        c.load_dscnn(e2e_golden["he.blob"], 12)
        push = lambda n_in=480, p=d_in: c._lib.kws_stream_push_rate_i16(c._h, p.data_ptr() if p is not None else None, n_in, lg.data_ptr(), lb.data_ptr())
        assert push() == _native.KWS_ESTATE                      # no resampler
        c.stream_resample_open(S, 48000, 16000, 480)
        assert push() == _native.KWS_ESTATE                      # no kws_stream_open
        c.stream_open(S + 1)
        assert push() == _native.KWS_ESTATE                      # another n_streams
        c.stream_open(S)
        c.stream_resample_open(S, 48000, 8000, 480)
        assert push() == _native.KWS_ESTATE                      # another output rate than the front end's
        pl, py = _native.C.c_void_p(), _native.C.c_void_p()
        h_in = np.zeros((S, 480), np.int16)
        assert c._lib.kws_stream_push_host_rate_i16(c._h, h_in.ctypes.data, 480, _native.C.byref(pl), _native.C.byref(py)) == _native.KWS_ESTATE
        c.stream_resample_open(S, 48000, 16000, 480)
        assert push(p=None) == _native.KWS_EINVAL and push(n_in=0) == _native.KWS_EINVAL and push(n_in=481) == _native.KWS_EINVAL
        assert c._lib.kws_stream_push_host_rate_i16(c._h, None, 480, _native.C.byref(pl), _native.C.byref(py)) == _native.KWS_EINVAL
        assert c.stream_state()[1] == 0, "a refused push reached the streams"
        assert push() == _native.KWS_OK
        c.sync()
        assert c.stream_state()[1] == 1
    finally:
        c.close()


# ---- 7. Python ------------------------------------------------------------------------------------------------------------------
def test_streaming_spotter_at_48_khz(ctx, e2e_golden):
    from kws.common.errors import ModelError
    from kws.inference import StreamingSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=12)
    model.load_state_dict(_scan_ref.state_from_blob(e2e_golden["he.blob"]))
    S, hops = 5, 40
    x = live_signal(e2e_golden, 48000, hops * 480)
    hop16 = batch_window(ctx, x, "1/3", hops * 160)  # the delayed resampled signal: what the streams must hear
    plain = StreamingSpotter(S, model)
    at48 = StreamingSpotter(S, model, input_rate=48000)
    dev48 = StreamingSpotter(S, model, input_rate=48000, host_results=False)
    same = StreamingSpotter(S, model, input_rate=16000)
    try:
        assert (plain.hop_in, plain.delay_samples, at48.hop, at48.hop_in, at48.delay_samples) == (160, 0, 160, 480, 10)
        assert (same.hop_in, same.delay_samples) == (160, 0)
        for t in range(hops):
            want_lb, want_lg = plain.push(hop16[:, t * 160:(t + 1) * 160])
            chunk = x[:, t * 480:(t + 1) * 480]
            for sp, arg in ((at48, chunk), (dev48, torch.from_numpy(np.ascontiguousarray(chunk)).to(DEV)), (same, hop16[:, t * 160:(t + 1) * 160])):
                lb, lg = sp.push(arg)
                assert np.array_equal(lb, want_lb) and np.array_equal(lg.view(np.uint32), want_lg.view(np.uint32)), f"hop {t}"
        assert np.abs(want_lg).max() > 0
        with pytest.raises(ModelError, match="480"):
            at48.push(hop16[:, :160])
    finally:
        for sp in (plain, at48, dev48, same):
            sp.close()
    assert StreamingSpotter.__init__.__defaults__[-1] is None
    for rate, hop_in in ((44100, 441), (8000, 80)):
        sp = StreamingSpotter(1, model, input_rate=rate)
        assert sp.hop_in == hop_in and sp.delay_samples == (10 if rate > 16000 else 20)
        sp.close()
    with pytest.raises(ModelError, match=r"22050.*220\.5"):
        StreamingSpotter(1, model, input_rate=22050)
