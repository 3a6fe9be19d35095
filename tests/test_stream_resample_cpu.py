"""CPU tests of the streaming resampler's host side (kws_host_stream_resample_plan / kws_host_stream_resample_count) and of the
NumPy restatement test_stream_resample_gpu.py judges the kernel by: with the LIBRARY's history length, the restatement fed in
random chunks equals _resample_ref.resample_ref of the whole signal, shifted by the delay."""
import ctypes as C

import numpy as np
import pytest

import _resample_ref as ref
import _resample_stream_ref as sref

native = pytest.importorskip("kws._native")

PAIRS = dict(ref.PAIRS)
PAIRS["320/441"] = (44100, 32000)
# pair -> (delay in output samples, input samples of history the outputs reach back to: found by enumeration over chunkings)
DELAY = {"1/3": 10, "2/1": 20, "160/441": 10, "640/441": 15, "1/6": 10, "1/12": 10, "1/24": 10, "320/441": 10}
NEED = {"1/3": 62, "2/1": 20, "160/441": 58, "640/441": 22, "1/6": 125, "1/12": 251, "1/24": 503}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_plan(pair):
    rate_in, rate_out = PAIRS[pair]
    up, down, delay, history = native.host_stream_resample_plan(rate_in, rate_out)
    assert (up, down) == ref.ratio(rate_in, rate_out)
    half = 10 * max(up, down)
    assert delay == DELAY[pair] == sref.delay_of(up, down) == -(-half // down)
    rows = (2 * half + up) // up
    assert history <= rows + -(-(delay * down - half + down) // up), "more than the sufficient length"
    if pair in NEED:
        assert history >= NEED[pair]
    assert native.Context.host_stream_resample_plan(rate_in, rate_out) == (up, down, delay, history)


def test_plan_and_count_codes():
    plan, cnt = native.lib().kws_host_stream_resample_plan, native.lib().kws_host_stream_resample_count
    v = [C.c_int(-7) for _ in range(4)]
    assert plan(48000, 16000, None, None, None, None) == native.KWS_OK
    assert plan(48000, 16000, C.byref(v[0]), None, C.byref(v[2]), None) == native.KWS_OK and (v[0].value, v[2].value) == (1, 10)
    assert plan(0, 16000, *map(C.byref, v)) == native.KWS_EINVAL and plan(16000, -1, *map(C.byref, v)) == native.KWS_EINVAL
    assert plan(16001, 16000, *map(C.byref, v)) == native.KWS_EUNSUPPORTED and plan(1025, 1, *map(C.byref, v)) == native.KWS_EUNSUPPORTED
    assert plan(22050, 22050, *map(C.byref, v)) == native.KWS_OK and [x.value for x in v] == [1, 1, 0, 0]  # a copy: no delay, no history
    n = C.c_int(-7)
    assert cnt(48000, 16000, 0, 480, None) == native.KWS_EINVAL
    assert cnt(48000, 16000, 0, -1, C.byref(n)) == native.KWS_EINVAL
    assert cnt(0, 16000, 0, 480, C.byref(n)) == native.KWS_EINVAL and cnt(48000, 0, 0, 480, C.byref(n)) == native.KWS_EINVAL
    assert cnt(16001, 16000, 0, 480, C.byref(n)) == native.KWS_EUNSUPPORTED
    assert n.value == -7, "a refused call wrote its result"
    assert cnt(48000, 16000, 0, 0, C.byref(n)) == native.KWS_OK and n.value == 0
    assert cnt(48000, 16000, 2, 1, C.byref(n)) == native.KWS_OK and n.value == 1
    assert cnt(44100, 16000, 2 ** 63 + 5, 441, C.byref(n)) == native.KWS_OK and n.value == sref.count(2 ** 63 + 5, 441, 160, 441)
    assert native.Context.host_stream_resample_count(8000, 16000, 3, 80) == 160


@pytest.mark.parametrize("pair", list(PAIRS))
def test_counts_sum_to_the_floor_over_any_chunking(pair):
    rate_in, rate_out = PAIRS[pair]
    up, down = ref.ratio(rate_in, rate_out)
    rng = np.random.default_rng(sum(map(ord, pair)))
    for start in (0, down * 7, down * (2 ** 40 // down + 1), 2 ** 40 + 1):
        P, total = start, 0
        for n_in in rng.choice([1, 2, 3, 7, down, down + 1, 441, 480, 1000], 60):
            got = native.host_stream_resample_count(rate_in, rate_out, P, int(n_in))
            assert got == sref.count(P, n_in, up, down), (pair, P, n_in)
            total += got
            P += int(n_in)
        assert total == P * up // down - start * up // down
        if start % down == 0:
            assert total == (P - start) * up // down  # a start on a multiple of down counts as a start at zero


@pytest.mark.parametrize("pair", list(PAIRS))
def test_the_restatement_in_chunks_is_the_batch_definition(pair):
    rate_in, rate_out = PAIRS[pair]
    up, down, delay, history = native.host_stream_resample_plan(rate_in, rate_out)
    taps = native.host_resample_design(rate_in, rate_out)[4]
    rng = np.random.default_rng(1 + sum(map(ord, pair)))
    z = -(-delay // up)
    for trial, first in enumerate((0, down * 5, down * (2 ** 40 // down + 1))):
        sizes = [int(v) for v in rng.choice([1, 2, 3, 7, down, down + 1, 441, 480, 1000], 14)]
        if trial == 0:
            sizes = [1] * (3 * down + 5) + sizes  # every residue of the position modulo down, one sample at a time
        N = sum(sizes)
        x = rng.integers(-16384, 16384, (2, N)).astype(np.int16)
        st = sref.StreamRef(2, up, down, taps, history, first_sample=first)
        outs, at = [], 0
        for n_in in sizes:
            y, _ = st.push(x[:, at:at + n_in])  # raises when an output leaves history || chunk
            assert y.shape[1] == sref.count(first + at, n_in, up, down)
            outs.append(y)
            at += n_in
        got = np.concatenate(outs, axis=1)
        assert got.shape[1] == N * up // down
        want, _ = sref.batch_window(x, up, down, taps, delay, z, got.shape[1])
        assert np.array_equal(got, want), f"{pair} first_sample {first}: {(got != want).sum()} outputs differ from the batch definition"
        if trial == 0 and pair in NEED:
            assert st.history_used() == NEED[pair], "one-sample pushes reach exactly as far back as the enumeration found"


def test_the_restatement_notices_a_short_history():
    up, down, delay, history = native.host_stream_resample_plan(48000, 16000)
    taps = native.host_resample_design(48000, 16000)[4]
    st = sref.StreamRef(1, up, down, taps, NEED["1/3"] - 1)
    with pytest.raises(IndexError):
        for _ in range(3 * down + 1):
            st.push(np.zeros((1, 1), np.int16))
