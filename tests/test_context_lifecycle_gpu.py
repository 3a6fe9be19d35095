"""What a context leaves behind: nothing.

Every buffer of a context is released by the context itself, and nothing in the Python interface shows one that was forgotten.
These tests look from outside: the device's free memory (torch.cuda.mem_get_info, after torch.cuda.synchronize) across repeated
lifetimes of a context that has used every unit, across repeated re-opening of the sub-states that replace themselves, and the
bits of an inference after the sub-states were closed in different orders and after a refused load.

One cycle (``_cycle``): create, load both models (host load, then the device load in place), reserve(128) and infer_i16 of 128
clips, a scan without ``feat``, a ragged scan of three short recordings, segment_f32, the DS-CNN and the cnn-trad-fpool3 backward at
B = 2, eval open + update, resample 8000 -> 16000, stream_open(64) with host results, stream_smooth_f32 and stream_vad_f32, live
utterances and live events armed, the stream resampler, three pushes (device hop, device at 48 kHz, host at 48 kHz), one host
submit and wait, close.

The bound: 32 cycles may cost at most 8 MiB of free device memory, so a buffer of 256 KiB or more that leaks once per cycle is
seen.  At the shapes of the cycle that covers: both weight images (DS-CNN 0.5 MiB, cnn-trad-fpool3 10.5 MiB), the feature
workspace (128 clips, 495 KiB), the scan's frame workspace (8 x 824 frames, 258 KiB), the training workspace, the posterior
smoothing ring (64 x 128 x 12 floats, 384 KiB), the evaluation statistics (64 classes x 1024 bins, 1 MiB), the utterance history
(64 x 32960 samples, 4 MiB), both event queues (8192 records: 384 and 320 KiB), the detection ring (64 x 256 x 12 floats,
768 KiB) and the host-ingest slots' device input (64 clips, 2 MiB each).
Smaller than 256 KiB here, and therefore INVISIBLE one by one to this test: the front-end tables, the float64 twiddles of
kws_spec_f32 (not made), the refinement worklist (~50 KiB), the two loaders' statistics blocks, the convolution scratch (only
segment_f32 uses it in the cycle: 1 KiB), the ragged plan tables, the streams' PCM ring (80 KiB), feature ring (247.5 KiB: just
under), hop counter, cluster partials (64 KiB) and counts, the device copies of the host results, the smoothing sums and count,
the endpointer bits and counts (context's and the utterance set's), the loss partials, the resampler's tap tables, the stream
resampler's history and hop buffer, the utterance set's walk positions, the detection set's smoothed row, labels and refractory
marks, the queues' counter blocks, and the ingest slots' logits and labels.  Together the stream set's own five buffers are
456 KiB per cycle, so forgetting all of them is seen.
Pinned host memory (host results, the queues' mirrors, the stream resampler's input, the ingest slots' staging) is not device
memory: mem_get_info does not count it and this test cannot see it leak.

The reading is device-wide (other processes on the card move it); ten idle readings in a row are printed with their spread
(0 bytes when this was written).
The lifetimes are measured behind THREE unmeasured ones, not one.  The HIP runtime itself takes device memory during the first two
lifetimes of a process and none after them: cumulative loss after each of 48 cycles in a fresh process, in KiB, 174080, 313344,
313344, ... (46 times the same figure), the same for the library before and after the buffers got their owners, four processes of
four.  The 139264 KiB of the second lifetime are what a single warm-up cycle left inside the measured span; they are no buffer of
the context: each step of the cycle alone costs 0 bytes over eight lifetimes -- the host ingest after one step of 32768 KiB which
40 further lifetimes did not repeat.  Two warm-up cycles are what the runtime needs, the third is spare.  The measured span, the bound and what they detect are unchanged: 32 cycles, 8 MiB.
"""
import numpy as np
import pytest
import torch

from kws import _native
from kws.common.errors import ModelError
from oracle import cnn_trad as o_ct
from oracle import dscnn as o_dscnn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NC = 12
S = 64
CYCLES = 32
WARMUP_LIFETIMES = 3  # the runtime's own pools grow during a process's first two context lifetimes (see above)
BOUND = 8 << 20
SCAN_R, SCAN_N, SCAN_HOP = 8, 132000, 4
RAGGED_LEN = (16000, 20000, 17000)
UTT = dict(on=3, off=5, pre_roll=4, max_frames=200, max_events=8192)


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _make_data():
    """Every tensor the cycles touch."""
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    i16 = lambda *shape: rng.integers(-3000, 3000, size=shape, dtype=np.int16)
    ds_blob = o_dscnn.flatten_state(o_dscnn.random_state(3, num_classes=NC))
    ct_blob = o_ct.flatten_state(o_ct.random_state(1, num_classes=NC))
    F, W = _native.host_scan_shape(SCAN_N, hop_frames=SCAN_HOP)
    start = np.cumsum([0] + [(n + 7) // 8 * 8 for n in RAGGED_LEN[:-1]])
    W_pack = _native.host_ragged_plan(RAGGED_LEN)[4]
    d = {
        "ds_blob": ds_blob, "ct_blob": ct_blob, "ds_blob_dev": dev(ds_blob), "ct_blob_dev": dev(ct_blob),
        "clips": dev(i16(128, 16000)), "logits128": torch.empty((128, NC), device=DEV), "labels128": torch.empty(128, dtype=torch.int32, device=DEV),
        "pcm": dev(i16(SCAN_R, SCAN_N)), "scan_logits": torch.empty((SCAN_R, W, NC), device=DEV),
        "ragged": dev(i16(int(start[-1]) + RAGGED_LEN[-1])), "ragged_start": start, "ragged_logits": torch.empty((W_pack, NC), device=DEV),
        "feat": dev(rng.standard_normal((2, F, 10)).astype(np.float32)), "seg_count": torch.empty(2, dtype=torch.int32, device=DEV),
        "x2": dev(rng.standard_normal((2, 1, 99, 10)).astype(np.float32)), "dl2": dev(rng.standard_normal((2, NC)).astype(np.float32)),
        "ds_grad": torch.empty(ds_blob.size, device=DEV), "ct_grad": torch.empty(ct_blob.size, device=DEV),
        "eval_logits": dev(rng.standard_normal((128, 64)).astype(np.float32)), "truth": dev(rng.integers(0, 64, 128).astype(np.int32)),
        "pcm8k": dev(i16(1, 8000)), "pcm16k": torch.empty((1, _native.host_resample_len(8000, 8000, 16000)), dtype=torch.int16, device=DEV),
        "hop": dev(i16(S, 160)), "hop48": dev(i16(S, 480)), "hop48_host": i16(S, 480),
        "lg": torch.empty((S, NC), device=DEV), "lb": torch.empty(S, dtype=torch.int32, device=DEV),
        "smoothed": torch.empty((S, NC), device=DEV), "vad": torch.empty(S, dtype=torch.int32, device=DEV),
        "host_clips": i16(8, 16000), "host_logits": np.empty((8, NC), np.float32), "host_labels": np.empty(8, np.int32),
        "two": dev(i16(2, 16000)), "lg2": torch.empty((2, NC), device=DEV),
    }
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def data():
    """Made once: the measured spans allocate nothing through torch."""
    return _make_data()


def _load_both(c, d):
    c.load_dscnn(d["ds_blob"], NC)
    c.load_dscnn_device(d["ds_blob_dev"], NC)
    c.load_cnn_trad(d["ct_blob"], NC)
    c.load_cnn_trad_device(d["ct_blob_dev"], NC)


def _arm(c):
    H = _native.host_stream_utt_history(400, 160, UTT["pre_roll"], UTT["max_frames"], 0)
    c.stream_utt_open(0.0, UTT["on"], UTT["off"], UTT["pre_roll"], UTT["max_frames"], H, UTT["max_events"])
    c.stream_detect_open(NC, 256, 2, 0.5, 3, 0, UTT["max_events"])


def _open_streams(c):
    c.stream_open(S)
    _arm(c)
    c.stream_host_results(True)


def _cycle(d):
    c = _native.Context(0)
    try:
        _load_both(c, d)
        c.reserve(128)
        c.infer_i16(d["clips"], d["logits128"], d["labels128"])
        c.scan_i16(d["pcm"], SCAN_HOP, d["scan_logits"])
        c.scan_ragged_i16(d["ragged"], d["ragged_start"], RAGGED_LEN, 1, d["ragged_logits"])
        c.segment_f32(d["feat"], SCAN_N, 0.0, d["seg_count"])
        c.dscnn_backward_f32(d["x2"], 99, 10, d["dl2"], d["ds_grad"])
        c.cnn_trad_backward_f32(d["x2"], d["dl2"], d["ct_grad"])
        c.eval_open(64, 1024)
        c.eval_update_f32(d["eval_logits"], d["truth"])
        c.resample_i16(d["pcm8k"], 8000, 16000, d["pcm16k"])
        _open_streams(c)
        c.stream_resample_open(S, 48000, 16000, 480)
        c.stream_push_i16(d["hop"], d["lg"], d["lb"])
        c.stream_smooth_f32(d["lg"], 128, d["smoothed"])
        c.stream_vad_f32(0.0, 3, 5, d["vad"])
        c.stream_push_rate_i16(d["hop48"], d["lg"], d["lb"])
        c.stream_push_host_rate_i16(d["hop48_host"], S)
        c.ingest_config(64, 2, 1)
        _, _, ticket, _ = c.infer_host_submit_i16(d["host_clips"], d["host_logits"], d["host_labels"])
        c.infer_host_wait(ticket)
        c.sync()
    finally:
        c.close()


def _held(what, run, n=CYCLES, warmup=1):
    """`run` unmeasured `warmup` times, then n times: the free memory it cost, printed and held to the bound."""
    for _ in range(warmup):
        run()
    idle = [_free() for _ in range(10)]
    before = idle[-1]
    for _ in range(n):
        run()
    lost = before - _free()
    print(f"{what}: {n} rounds cost {lost} bytes of free device memory ({lost / 1024:.0f} KiB); "
          f"ten idle readings before them spread over {max(idle) - min(idle)} bytes")
    assert lost <= BOUND, f"{what}: {lost} bytes of device memory gone after {n} rounds"


# ---- 1. lifetimes -----------------------------------------------------------------------------------------------------------------
def test_repeated_lifetimes_do_not_eat_device_memory(data):
    _held("context lifetime", lambda: _cycle(data), warmup=WARMUP_LIFETIMES)


# ---- 2. re-opening replaces ---------------------------------------------------------------------------------------------------------
def test_reopening_replaces_rather_than_stacks(data):
    c = _native.Context(0)
    try:
        c.load_dscnn(data["ds_blob"], NC)
        _held("stream_open + utterances + events + host results", lambda: _open_streams(c))
        _held("eval_open", lambda: c.eval_open(64, 1024))
        _held("stream_resample_open", lambda: c.stream_resample_open(S, 48000, 16000, 480))
    finally:
        c.close()


# ---- 3. closes in any order ---------------------------------------------------------------------------------------------------------
def _infer_two(c, d):
    c.infer_i16(d["two"], d["lg2"])
    c.sync()
    return d["lg2"].cpu().numpy().view(np.uint32).copy()


ORDERS = {
    "inner-first": ("stream_detect_close", "stream_utt_close", "stream_resample_close", "stream_close"),
    "streams-first": ("stream_close", "stream_resample_close", "stream_utt_close", "stream_detect_close"),
}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_a_context_survives_its_sub_states_closes(data, order):
    fresh = _native.Context(0)
    c = _native.Context(0)
    try:
        fresh.load_dscnn(data["ds_blob"], NC)
        want = _infer_two(fresh, data)
        c.load_dscnn(data["ds_blob"], NC)
        _open_streams(c)
        c.stream_resample_open(S, 48000, 16000, 480)
        c.stream_push_rate_i16(data["hop48"], data["lg"], data["lb"])
        for name in ORDERS[order]:
            getattr(c, name)()
        assert np.array_equal(_infer_two(c, data), want)
    finally:
        c.close()
        fresh.close()


# ---- 4. a refused load keeps the model ----------------------------------------------------------------------------------------------
def test_a_failed_load_keeps_the_model(data):
    c = _native.Context(0)
    try:
        _load_both(c, data)
        ct = torch.empty((2, NC), device=DEV)

        def both():
            c.infer_cnn_trad_i16(data["two"], ct)
            return _infer_two(c, data), ct.cpu().numpy().view(np.uint32).copy()

        want = both()
        with pytest.raises(ModelError):
            c.load_dscnn_device(data["ds_blob_dev"][:-1], NC)
        with pytest.raises(ModelError):
            c.load_cnn_trad_device(data["ct_blob_dev"][:-1], NC)
        got = both()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        c.close()
