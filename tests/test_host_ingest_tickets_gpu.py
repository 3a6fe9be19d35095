"""Ticket semantics of the host ingest: kws_infer_host_submit_i16 / kws_infer_host_wait at the edges of their bookkeeping.

The path holds pack threads, two H2D streams, a D2H stream and a ring of staging slots that persists across calls; its bugs are
bookkeeping bugs, and those return plausible arrays.  So every destination array here starts out full of sentinels (NaN logits,
label -7) and "complete" means: no sentinel left and every row equal, bit for bit, to what the device-resident kws_infer_i16
returns for the same clip on the same context.  Those device results are themselves held once to the imported reference model's
logits for the 48 golden clips (within the suite's TOL, labels exactly), so no comparison is only HIP against HIP.

The ring is made tiny -- ``ingest_config(chunk_clips=2, n_slots=2, pack_threads=-1)`` unless a case says otherwise -- so that a
handful of clips reaches every edge: a batch of B <= 128 clips is cut into chunks of min(chunk_clips, B), so B = 3 fills both
slots and B = 5 wraps the ring inside one call.

Not covered, on purpose: a submit that fails after enqueuing some of its chunks, and a wait whose D2H failed.  Both need a HIP
call to fail, and no test here makes one fail.  Nor does any test destroy a context with batches in flight (except the
keep-alive case, whose tear-down is ``close()`` alone: it frees the ring and copies nothing to caller arrays)."""
import ctypes as C
import gc
import weakref

import numpy as np
import pytest
import torch

import _scan_ref
from conftest import synth_clips
from kws import _native
from kws.common.errors import ModelError
from oracle import dscnn as o_dscnn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NC = 12
TOL = 1e-4          # the suite's logit tolerance against the imported reference model (tests/test_gpu_parity.py)
BAD_LABEL = -7      # no class has it
TINY = (2, 2, -1)   # chunk_clips, n_slots, pack on the calling thread


def _device_results(c, clips, classes):
    """The device-resident fused call on context ``c``: (logits float32 [B, classes], labels int32 [B])."""
    wav = torch.from_numpy(np.ascontiguousarray(clips)).to(DEV)
    logits = torch.empty((len(clips), classes), dtype=torch.float32, device=DEV)
    labels = torch.empty((len(clips),), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()  # the context runs on a stream of its own
    c.infer_i16(wav, logits, labels)
    c.sync()
    return logits.cpu().numpy(), labels.cpu().numpy()


@pytest.fixture(scope="module")
def clips(e2e_golden):
    """64 clips: the 48 golden ones, then 16 synthetic (every 16th of those all-zero)."""
    return np.ascontiguousarray(np.concatenate([e2e_golden["clips"], synth_clips(16, 77, "gauss")]).astype(np.int16))


@pytest.fixture(scope="module")
def shared(e2e_golden):
    c = _native.Context(0)
    c.load_dscnn(e2e_golden["he.blob"], NC)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(shared, clips, e2e_golden):
    """Expected (logits, labels) of every clip: kws_infer_i16 on the shared context, computed once, anchored on the reference model."""
    logits, labels = _device_results(shared, clips, NC)
    assert np.abs(logits[:48] - e2e_golden["he.logits"][8:]).max() <= TOL
    assert np.array_equal(labels[:48], e2e_golden["he.label"][8:])
    assert np.isfinite(logits).all()  # NaN can serve as the sentinel
    logits.setflags(write=False)
    labels.setflags(write=False)
    return logits, labels


@pytest.fixture
def ctx(shared):
    """The shared context with nothing in flight and the tiny ring, before and after each test."""
    shared.infer_host_wait(0)
    shared.ingest_config(*TINY)
    yield shared
    shared.infer_host_wait(0)


class Batch:
    """Clips [lo, hi) of the pool with sentinel-filled destinations, one row longer than the batch."""

    def __init__(self, clips, want, lo, hi, classes=NC):
        self.src = clips[lo:hi].copy()
        self.B = hi - lo
        self.logits = np.full((self.B + 1, classes), np.nan, np.float32)
        self.label = np.full((self.B + 1,), BAD_LABEL, np.int32)
        self.want_logits, self.want_label = want[0][lo:hi], want[1][lo:hi]
        self.ticket = None

    def submit(self, c, src=None):
        _, _, self.ticket, _ = c.infer_host_submit_i16(self.src if src is None else src, self.logits[:self.B], self.label[:self.B])
        return self.ticket

    def rows(self):
        """Per row: 'pending' (all sentinel), 'done' (the expected bits) or 'torn' (anything else)."""
        out = []
        for i in range(self.B):
            if np.isnan(self.logits[i]).all() and self.label[i] == BAD_LABEL:
                out.append("pending")
            elif np.array_equal(self.logits[i], self.want_logits[i]) and self.label[i] == self.want_label[i]:
                out.append("done")
            else:
                out.append("torn")
        return out

    def guard_intact(self):
        return bool(np.isnan(self.logits[self.B]).all() and self.label[self.B] == BAD_LABEL)

    def assert_complete(self, what=""):
        assert self.rows() == ["done"] * self.B, (what, self.rows())
        assert np.array_equal(self.logits[:self.B], self.want_logits) and np.array_equal(self.label[:self.B], self.want_label), what
        assert self.guard_intact(), f"{what}: a row landed past the end of the batch's arrays"

    def assert_untorn(self, what=""):
        assert "torn" not in self.rows(), (what, self.rows())
        assert self.guard_intact(), f"{what}: a row landed past the end of the batch's arrays"


def _raw_submit(c, h_wav, B, h_logits, h_label):
    """kws_infer_host_submit_i16 with raw addresses (None: NULL) -> (return code, ticket)."""
    ticket = C.c_uint64(0)
    rc = _native.lib().kws_infer_host_submit_i16(c._h, C.c_void_p(h_wav), int(B), C.c_void_p(h_logits), C.c_void_p(h_label), C.byref(ticket))
    return rc, int(ticket.value)


# ---- 1. ticket numbering ------------------------------------------------------------------------------------------------------------
def test_ticket_numbering(ctx, clips, want):
    assert _native.lib().kws_infer_host_wait(ctx._h, C.c_uint64(0)) == _native.KWS_OK   # nothing in flight
    a, b, c3 = Batch(clips, want, 0, 1), Batch(clips, want, 1, 3), Batch(clips, want, 3, 4)
    try:
        tickets = [x.submit(ctx) for x in (a, b, c3)]
        assert all(t > 0 for t in tickets) and tickets[0] < tickets[1] < tickets[2], tickets
        for _ in range(2):                                                              # waiting twice is harmless
            assert _native.lib().kws_infer_host_wait(ctx._h, C.c_uint64(tickets[0])) == _native.KWS_OK
            a.assert_complete("a")
        b.assert_untorn("b")
        c3.assert_untorn("c")
        # a ticket above any issued: OK, and everything in flight is delivered
        assert _native.lib().kws_infer_host_wait(ctx._h, C.c_uint64(tickets[2] + 1000)) == _native.KWS_OK
        b.assert_complete("b")
        c3.assert_complete("c")
        later = Batch(clips, want, 4, 5)
        assert later.submit(ctx) > tickets[2]                                           # numbering goes on, unaffected by that wait
        ctx.infer_host_wait(later.ticket)
        later.assert_complete("later")
    finally:
        ctx.infer_host_wait(0)


# ---- 2. waiting for the older ticket --------------------------------------------------------------------------------------------------
def test_wait_for_an_older_ticket_leaves_the_newer_one_whole(ctx, clips, want):
    ctx.ingest_config(4, 4, -1)
    a, b, c3 = Batch(clips, want, 0, 3), Batch(clips, want, 3, 6), Batch(clips, want, 6, 9)   # one chunk each: all three in flight
    try:
        for x in (a, b, c3):
            x.submit(ctx)
        ctx.infer_host_wait(b.ticket)
        a.assert_complete("a after wait(b)")
        b.assert_complete("b after wait(b)")
        c3.assert_untorn("c after wait(b)")
        ctx.infer_host_wait(0)
        for x in (a, b, c3):
            x.assert_complete("after wait(0)")
    finally:
        ctx.infer_host_wait(0)


# ---- 3. the ring wraps across tickets ---------------------------------------------------------------------------------------------------
def test_ring_wrap_across_tickets(ctx, clips, want):
    a, b, c3 = Batch(clips, want, 0, 3), Batch(clips, want, 3, 8), Batch(clips, want, 8, 9)
    try:
        a.submit(ctx)                   # chunks of 2 + 1: both slots
        a.assert_untorn("a in flight")
        b.submit(ctx)                   # chunks of 2 + 2 + 1: takes both of a's slots, then its own first one again
        a.assert_complete("a, delivered while b recycled its slots")
        b.assert_untorn("b in flight")
        assert b.rows()[:2] == ["done", "done"], b.rows()   # b's first chunk was delivered when b's third needed the slot
        c3.submit(ctx)                  # one chunk: takes the slot of b's second chunk
        assert b.rows()[:4] == ["done"] * 4, b.rows()
        ctx.infer_host_wait(a.ticket)
        a.assert_complete("a after wait(a)")
        b.assert_untorn("b after wait(a)")
        c3.assert_untorn("c after wait(a)")
        ctx.infer_host_wait(0)
        for x in (a, b, c3):
            x.assert_complete("after wait(0)")
    finally:
        ctx.infer_host_wait(0)


# ---- 4. a refused submit between two good ones ------------------------------------------------------------------------------------------
def test_a_refused_submit_loses_nothing(ctx, clips, want):
    """The regression: a refusal used to synchronise the device and forget every slot, and the wait for the older ticket then
    returned KWS_OK over rows nobody had filled."""
    a, d = Batch(clips, want, 0, 3), Batch(clips, want, 3, 6)
    other = Batch(clips, want, 6, 8)    # the arrays of the refused calls: must stay untouched
    d_wav = torch.from_numpy(clips[6:8]).to(DEV)
    d_out = torch.empty((2, NC), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    src, lg, lb = other.src.ctypes.data, other.logits.ctypes.data, other.label.ctypes.data
    refusals = {
        "B = 0": (src, 0, lg, lb),
        "NULL h_wav": (None, 2, lg, lb),
        "device pointer as h_wav": (d_wav.data_ptr(), 2, lg, lb),
        "device pointer as h_logits": (src, 2, d_out.data_ptr(), lb),
    }
    try:
        a.submit(ctx)
        for what, args in refusals.items():
            rc, ticket = _raw_submit(ctx, *args)
            assert rc == _native.KWS_EINVAL, (what, rc)
            assert ticket == 0, what                       # no ticket is handed out by a refusal
            a.assert_untorn(f"a after the refusal '{what}'")
            assert other.rows() == ["pending"] * 2 and other.guard_intact(), what
        assert _native.lib().kws_infer_host_wait(ctx._h, C.c_uint64(a.ticket)) == _native.KWS_OK
        a.assert_complete("a after the refusals and wait(a)")
        assert d.submit(ctx) > a.ticket
        ctx.infer_host_wait(d.ticket)
        d.assert_complete("d: the context still works")
        assert other.rows() == ["pending"] * 2 and other.guard_intact()
    finally:
        ctx.infer_host_wait(0)


# ---- 5. the geometry changes while a batch is in flight --------------------------------------------------------------------------------
def test_geometry_change_in_flight(clips, want, e2e_golden):
    """kws_ingest_config and a submit after a model with another class count are refused (KWS_ESTATE) while a batch is in flight,
    and the batch is delivered whole into its 12-class arrays.  kws_load_dscnn itself is ordered behind the chunks in flight: it
    drains the context's stream, on which every chunk's kernels were enqueued by the submit, before it swaps the weight image
    -- so the batch submitted BEFORE the load has the 12-class model's bits."""
    blob5 = o_dscnn.flatten_state(o_dscnn.random_state(3, num_classes=5))
    assert np.isfinite(blob5).all()
    c = _native.Context(0)
    try:
        c.load_dscnn(e2e_golden["he.blob"], NC)
        c.ingest_config(*TINY)
        a = Batch(clips, want, 0, 3)
        a.submit(c)
        with pytest.raises(ModelError, match=rf"\(code {_native.KWS_ESTATE}\)"):
            c.ingest_config(8, 2, 0)
        a.assert_untorn("a after the refused ingest_config")
        c.infer_host_wait(a.ticket)
        a.assert_complete("a after the refused ingest_config and wait(a)")

        a = Batch(clips, want, 3, 6)
        a.submit(c)
        c.load_dscnn(blob5, 5)
        five = np.full((3, 5), np.nan, np.float32), np.full((3,), BAD_LABEL, np.int32)
        rc, ticket = _raw_submit(c, a.src.ctypes.data, 2, five[0].ctypes.data, five[1].ctypes.data)
        assert rc == _native.KWS_ESTATE and ticket == 0
        assert "geometry changed" in _native.lib().kws_last_error(c._h).decode()
        a.assert_untorn("a after the refused 5-class submit")
        assert _native.lib().kws_infer_host_wait(c._h, C.c_uint64(a.ticket)) == _native.KWS_OK
        a.assert_complete("a, submitted before the 5-class load, delivered after it")
        assert np.isnan(five[0]).all() and (five[1] == BAD_LABEL).all()
        c.infer_host_wait(0)

        want5 = _device_results(c, clips[6:9], 5)
        assert np.isfinite(want5[0]).all()
        b = Batch(clips, want5, 0, 3, classes=5)          # want5 is indexed from 0
        b.src = clips[6:9].copy()
        b.submit(c)
        c.infer_host_wait(b.ticket)
        b.assert_complete("the 5-class batch after wait(0)")
    finally:
        c.infer_host_wait(0)
        c.close()


# ---- 6. what the caller may do with its source ------------------------------------------------------------------------------------------
def test_source_reuse(ctx, clips, want):
    try:
        # pageable: packed into pinned staging by the time submit returns, so the caller may overwrite it at once
        a = Batch(clips, want, 0, 3)
        a.submit(ctx)
        a.src[:] = clips[10:13]
        ctx.infer_host_wait(a.ticket)
        a.assert_complete("pageable source overwritten after submit")
        # pinned: read by the DMA in place, left alone until the wait; the same bits
        pinned = torch.from_numpy(clips[0:3].copy()).pin_memory()
        assert pinned.is_pinned()
        p = Batch(clips, want, 0, 3)
        p.submit(ctx, pinned)
        ctx.infer_host_wait(p.ticket)
        p.assert_complete("pinned source")
        assert np.array_equal(p.logits, a.logits, equal_nan=True) and np.array_equal(p.label, a.label)
        # one pinned and one pageable batch in flight together
        pinned2 = torch.from_numpy(clips[20:22].copy()).pin_memory()
        p2, q = Batch(clips, want, 20, 22), Batch(clips, want, 22, 24)
        p2.submit(ctx, pinned2)
        q.submit(ctx)
        q.src[:] = 0
        p2.assert_untorn("pinned, in flight")
        q.assert_untorn("pageable, in flight")
        ctx.infer_host_wait(0)
        p2.assert_complete("pinned beside pageable")
        q.assert_complete("pageable beside pinned")
        assert np.array_equal(pinned2.numpy(), clips[20:22])   # the library only reads the caller's source
    finally:
        ctx.infer_host_wait(0)


# ---- 7. no label array ------------------------------------------------------------------------------------------------------------------
def test_null_label(ctx, clips, want):
    a = Batch(clips, want, 0, 3)
    try:
        rc, ticket = _raw_submit(ctx, a.src.ctypes.data, 3, a.logits.ctypes.data, None)
        assert rc == _native.KWS_OK and ticket > 0
        assert _native.lib().kws_infer_host_wait(ctx._h, C.c_uint64(ticket)) == _native.KWS_OK
        assert np.array_equal(a.logits[:3], a.want_logits) and np.isnan(a.logits[3]).all()
        assert (a.label == BAD_LABEL).all()
    finally:
        ctx.infer_host_wait(0)


# ---- 8. the threaded pack at its edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, threads", [(33, 5), (40, 64)])
def test_threaded_pack(ctx, clips, want, B, threads):
    """The pool engages for copies of 1 MiB and more: 33 clips of 32000 bytes are the first chunk that is.  40 clips on 64 threads:
    the 4 KiB-aligned slices (20480 bytes) overshoot the chunk, and the last thread gets an empty range."""
    assert 32 * 32000 < (1 << 20) <= 33 * 32000 and 40 * 32000 < 63 * 20480
    ctx.ingest_config(B, 2, threads)
    a = Batch(clips, want, 64 - B, 64)
    try:
        a.submit(ctx)
        ctx.infer_host_wait(a.ticket)
        a.assert_complete(f"one chunk of {B} clips packed by {threads} threads")
    finally:
        ctx.infer_host_wait(0)


# ---- 9. the Python side keeps what the library points into --------------------------------------------------------------------------------
def test_context_keeps_in_flight_arrays_alive(clips, e2e_golden):
    """infer_host_submit_i16 returns freshly allocated arrays to which the library holds raw pointers: the Context must keep them
    (and the source) referenced until infer_host_wait retires the ticket, whatever the caller does with the returned tuple.
    Tear-down is close() alone, which frees the ring and copies nothing to caller arrays."""
    c = _native.Context(0)
    try:
        c.load_dscnn(e2e_golden["he.blob"], NC)
        c.ingest_config(*TINY)
        got = c.infer_host_submit_i16(clips[0:3].copy())
        ticket = got[2]
        refs = [weakref.ref(got[0]), weakref.ref(got[1]), weakref.ref(got[3])]
        del got
        gc.collect()
        assert all(r() is not None for r in refs), "the context let go of arrays the library still points into"
        c.infer_host_wait(ticket)
        gc.collect()
        assert all(r() is None for r in refs), "the context still holds the arrays of a retired ticket"
        # wait(0) retires every ticket
        tickets = [c.infer_host_submit_i16(clips[i:i + 1].copy())[2] for i in range(2)]
        assert sorted(c._host_inflight) == tickets
        c.infer_host_wait(tickets[0])
        assert sorted(c._host_inflight) == tickets[1:]
        c.infer_host_wait(0)
        assert not c._host_inflight
    finally:
        c.close()
    assert not c._host_inflight


# ---- 10. infer_batches abandoned early ----------------------------------------------------------------------------------------------------
def test_infer_batches_abandoned_early(clips, want, e2e_golden):
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=NC)
    model.load_state_dict(_scan_ref.state_from_blob(e2e_golden["he.blob"]))
    spotter = KeywordSpotter(model)
    batches = [clips[0:3], clips[3:5], clips[5:8]]
    it = spotter.infer_batches(iter(batches))
    labels, logits = next(it)
    assert np.array_equal(logits, want[0][0:3]) and np.array_equal(labels, want[1][0:3])
    it.close()                                              # the second batch is in flight here
    labels, logits = spotter.infer_pcm16(clips[8:12])
    assert np.array_equal(logits, want[0][8:12]) and np.array_equal(labels, want[1][8:12])
    c = model._context(0)
    assert _native.lib().kws_infer_host_wait(c._h, C.c_uint64(0)) == _native.KWS_OK
    assert not c._host_inflight
