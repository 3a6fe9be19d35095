"""What the decision and endpointer entries over recordings refuse, word for word, and which refusal wins.

kws_scan_detect_f32, kws_scan_score_f32 and kws_segment_f32 and their ragged twins each refuse on the host, before any launch,
with a return code and a text that starts with the entry's own name.  The table below holds one row per refusal sentence of the
sources and rows with two faults at once that pin which of the two is reported; the texts are literals recorded from the library
before the twins shared their host code, and kws_last_error is compared byte for byte (the C symbols are called directly because
Context._check wraps the text).  Every device buffer is poisoned (NaN / -7) and must be untouched after every refusal.

Two sentences cannot be reached on a live context and have no row: "front end not configured" (kws_create configures one) and
"needs cepstrum 0 = log frame energy (appendEnergy)" (no entry switches it off)."""
import ctypes

import numpy as np
import pytest
import torch

from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
INV, UNS = _native.KWS_EINVAL, _native.KWS_EUNSUPPORTED
R, W, NC, K, M, F = 2, 4, 12, 3, 2, 20
NULL = None
P = 7  # the poison of the integer buffers is -P

i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
f32 = lambda *v: (ctypes.c_float * len(v))(*v)
rows4 = lambda *rows: i32(*[v for row in rows for v in row])


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


@pytest.fixture(scope="module")
def buf():
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    ints = lambda *shape: torch.full(shape, -P, dtype=torch.int32, device=DEV)
    b = {"logits": nan(R * W, NC), "smoothed": nan(R * W, NC), "count": ints(R), "ev_w": ints(R, M), "ev_k": ints(R, M), "ev_s": nan(R, M),
         "counts": torch.full((K, NC, 4), -P, dtype=torch.int64, device=DEV), "feat": nan(R * F, 10), "utt": ints(R, M, 5)}
    torch.cuda.synchronize()
    return b


def untouched(buf):
    torch.cuda.synchronize()
    return [k for k, t in buf.items() if not (torch.isnan(t).all() if t.is_floating_point() else (t == -P).all())]


# ---- the calls: valid arguments unless a row overrides them -------------------------------------------------------------------------
def _ptr(buf, key, given):
    return buf[key].data_ptr() if given is True else given


def detect(lib, h, b, logits=True, R=R, W=W, C=NC, S=3, fk=2, thr=0.5, refr=2, smoothed=True, ev_w=True, ev_k=True, ev_s=True, m=M,
           count=True):
    return lib.kws_scan_detect_f32(h, _ptr(b, "logits", logits), R, W, C, S, fk, thr, refr, _ptr(b, "smoothed", smoothed), _ptr(b, "ev_w", ev_w),
                                   _ptr(b, "ev_k", ev_k), _ptr(b, "ev_s", ev_s), m, _ptr(b, "count", count))


def detect_ragged(lib, h, b, logits=True, off=i32(0, W), win=i32(W, W), R=R, C=NC, S=3, fk=2, thr=0.5, refr=2, smoothed=True, ev_w=True,
                  ev_k=True, ev_s=True, m=M, count=True):
    return lib.kws_scan_detect_ragged_f32(h, _ptr(b, "logits", logits), off, win, R, C, S, fk, thr, refr, _ptr(b, "smoothed", smoothed),
                                          _ptr(b, "ev_w", ev_w), _ptr(b, "ev_k", ev_k), _ptr(b, "ev_s", ev_s), m, _ptr(b, "count", count))


TRUTH = rows4((0, 2, 0, 1), (1, 3, 2, 3))


def score(lib, h, b, logits=True, R=R, W=W, C=NC, S=3, fk=2, refr=2, th=f32(0.2, 0.5, 0.8), K=K, truth=TRUTH, N=2, counts=True):
    return lib.kws_scan_score_f32(h, _ptr(b, "logits", logits), R, W, C, S, fk, refr, th, K, truth, N, _ptr(b, "counts", counts))


def score_ragged(lib, h, b, logits=True, off=i32(0, W), win=i32(W, W), R=R, C=NC, S=3, fk=2, refr=2, th=f32(0.2, 0.5, 0.8), K=K, truth=TRUTH,
                 N=2, counts=True):
    return lib.kws_scan_score_ragged_f32(h, _ptr(b, "logits", logits), off, win, R, C, S, fk, refr, th, K, truth, N, _ptr(b, "counts", counts))


def segment(lib, h, b, feat=True, R=R, F=F, n=3520, thr=0.0, on=3, off=5, pre=2, max_frames=0, utt=True, m=M, count=True):
    return lib.kws_segment_f32(h, _ptr(b, "feat", feat), R, F, n, thr, on, off, pre, max_frames, _ptr(b, "utt", utt), m, _ptr(b, "count", count))


def segment_ragged(lib, h, b, feat=True, frame_off=i32(0, F), frames=i32(F, F), length=i32(3520, 3520), R=R, thr=0.0, on=3, off=5, pre=2,
                   max_frames=0, utt=True, m=M, count=True):
    return lib.kws_segment_ragged_f32(h, _ptr(b, "feat", feat), frame_off, frames, length, R, thr, on, off, pre, max_frames, _ptr(b, "utt", utt),
                                      m, _ptr(b, "count", count))


CALLS = {"kws_scan_detect_f32": detect, "kws_scan_detect_ragged_f32": detect_ragged, "kws_scan_score_f32": score,
         "kws_scan_score_ragged_f32": score_ragged, "kws_segment_f32": segment, "kws_segment_ragged_f32": segment_ragged}

# ---- the table: (entry, arguments, code, the text after "<entry>: ") ------------------------------------------------------------
SMOOTH = "smooth_window must be in [1, 256]"
REFR = "need refractory >= 1 and first_keyword >= 0"
ARRAYS = "max_events events need their three arrays"
SPANS = ("windows must not be negative and the recordings' windows must not overlap (win_off ascending, win_off[r] >= win_off[r - 1] + "
         "windows[r - 1])")
PACKED = "more than 2^30 packed windows in one call"
WINDOWS = "more than 2^30 windows in one call"
RECS = "more than 2^20 recordings in one call"
TABLE = ("the annotations need 0 <= recording < R, first_keyword <= label < C, 0 <= first_window <= last_window, and no two overlapping "
         "rows of one recording and label")
TABLE_BIG = "more than 2^24 annotations or 2^20 recordings in one call"
KN = "need K in [1, 1024] and N >= 0"
RC = "need R >= 1 and C in [1, 64]"
EP = "need 1 <= on_window <= off_window <= 1024"
PRE = "need pre_roll >= 0 and max_frames == 0 or >= 2"
UTTS = "max_utts utterances need d_utt"
MANY = 1 << 20
OVERLAP = dict(off=i32(0, W - 1))
BAD_ROW = dict(truth=rows4((0, 1, 0, 1)), N=1)  # a label below first_keyword

ROWS = []
e = "kws_scan_detect_f32"
NULLS = "d_logits / d_event_count is NULL"
SHAPE = "need R >= 1, W >= 1 and C in [1, 64]"
ROWS += [(e, dict(logits=NULL), INV, NULLS), (e, dict(count=NULL), INV, NULLS),
         (e, dict(m=-1), INV, ARRAYS), (e, dict(ev_w=NULL), INV, ARRAYS), (e, dict(ev_k=NULL), INV, ARRAYS), (e, dict(ev_s=NULL), INV, ARRAYS),
         (e, dict(R=0), INV, SHAPE), (e, dict(W=0), INV, SHAPE), (e, dict(C=0), INV, SHAPE), (e, dict(C=65), INV, SHAPE),
         (e, dict(S=0), INV, SMOOTH), (e, dict(S=257), INV, SMOOTH), (e, dict(refr=0), INV, REFR), (e, dict(fk=-1), INV, REFR),
         (e, dict(R=MANY, W=1025), UNS, WINDOWS),
         # two faults
         (e, dict(logits=NULL, C=65), INV, NULLS), (e, dict(m=-1, R=0), INV, ARRAYS), (e, dict(count=NULL, m=-1), INV, NULLS),
         (e, dict(W=0, S=0), INV, SHAPE), (e, dict(S=0, refr=0), INV, SMOOTH), (e, dict(refr=0, R=MANY, W=1025), INV, REFR),
         (e, dict(S=257, R=MANY, W=1025), INV, SMOOTH)]
e = "kws_scan_detect_ragged_f32"
NULLS = "d_logits / d_event_count / win_off / windows is NULL"
ROWS += [(e, dict(logits=NULL), INV, NULLS), (e, dict(count=NULL), INV, NULLS), (e, dict(off=NULL), INV, NULLS), (e, dict(win=NULL), INV, NULLS),
         (e, dict(m=-1), INV, ARRAYS), (e, dict(ev_k=NULL), INV, ARRAYS),
         (e, dict(R=0), INV, RC), (e, dict(C=0), INV, RC), (e, dict(C=65), INV, RC), (e, dict(R=MANY + 1), UNS, RECS),
         (e, dict(S=0), INV, SMOOTH), (e, dict(S=257), INV, SMOOTH), (e, dict(refr=0), INV, REFR), (e, dict(fk=-1), INV, REFR),
         (e, OVERLAP, INV, SPANS), (e, dict(win=i32(W, -1)), INV, SPANS), (e, dict(off=i32(0, 1 << 30)), UNS, PACKED),
         # two faults
         (e, dict(S=0, **OVERLAP), INV, SMOOTH), (e, dict(win=NULL, C=65), INV, NULLS), (e, dict(m=-1, win=NULL), INV, NULLS),
         (e, dict(C=65, R=MANY + 1), INV, RC), (e, dict(R=MANY + 1, S=0), UNS, RECS), (e, dict(refr=0, off=i32(0, 1 << 30)), INV, REFR),
         (e, dict(off=i32(1 << 30, 0)), UNS, PACKED),   # recording 0 runs past 2^30 before recording 1 is seen to overlap it
         (e, dict(m=-1, R=0), INV, ARRAYS)]
for e in ("kws_scan_score_f32", "kws_scan_score_ragged_f32"):
    NULLS = "d_logits / thresholds / d_counts is NULL"
    ROWS += [(e, dict(logits=NULL), INV, NULLS), (e, dict(th=NULL), INV, NULLS), (e, dict(counts=NULL), INV, NULLS),
             (e, dict(K=0), INV, KN), (e, dict(K=1025), INV, KN), (e, dict(N=-1), INV, KN),
             (e, dict(R=0), INV, RC), (e, dict(C=0), INV, RC), (e, dict(C=65), INV, RC),
             (e, dict(S=0), INV, SMOOTH), (e, dict(S=257), INV, SMOOTH), (e, dict(refr=0), INV, REFR), (e, dict(fk=-1), INV, REFR),
             (e, dict(N=(1 << 24) + 1), UNS, TABLE_BIG), (e, BAD_ROW, INV, TABLE), (e, dict(truth=NULL, N=1), INV, TABLE),
             (e, dict(truth=rows4((0, 2, 0, 2), (0, 2, 2, 3))), INV, TABLE), (e, dict(truth=rows4((2, 2, 0, 1)), N=1), INV, TABLE),
             # two faults
             (e, dict(logits=NULL, K=0), INV, NULLS), (e, dict(K=0, C=65), INV, KN), (e, dict(C=65, S=0), INV, RC),
             (e, dict(S=0, refr=0), INV, SMOOTH), (e, dict(refr=0, **BAD_ROW), INV, REFR)]
e = "kws_scan_score_f32"
ROWS += [(e, dict(W=0), INV, "need W >= 1"), (e, dict(R=MANY, W=1025), UNS, WINDOWS), (e, dict(R=MANY + 1), UNS, TABLE_BIG),
         # two faults: W is looked at after the shared arguments, before the table
         (e, dict(W=0, S=0), INV, SMOOTH), (e, dict(W=0, refr=0), INV, REFR), (e, dict(W=0, **BAD_ROW), INV, "need W >= 1"),
         (e, dict(R=MANY, W=1025, **BAD_ROW), UNS, WINDOWS), (e, dict(W=0, R=0), INV, RC)]
e = "kws_scan_score_ragged_f32"
ROWS += [(e, dict(off=NULL), INV, "win_off / windows is NULL"), (e, dict(win=NULL), INV, "win_off / windows is NULL"),
         (e, dict(R=MANY + 1), UNS, RECS), (e, OVERLAP, INV, SPANS), (e, dict(win=i32(-1, W)), INV, SPANS),
         (e, dict(off=i32(0, 1 << 30)), UNS, PACKED),
         # two faults
         (e, dict(off=NULL, refr=0), INV, REFR), (e, dict(off=NULL, R=MANY + 1), INV, "win_off / windows is NULL"),
         (e, dict(R=MANY + 1, **OVERLAP), UNS, RECS), (e, dict(**OVERLAP, **BAD_ROW), INV, SPANS),
         (e, dict(off=i32(0, 1 << 30), **BAD_ROW), UNS, PACKED),
         # a bad annotation row is refused although no recording has a window
         (e, dict(win=i32(0, 0), **BAD_ROW), INV, TABLE), (e, dict(win=i32(0, 0), N=(1 << 24) + 1), UNS, TABLE_BIG)]
e = "kws_segment_f32"
NULLS = "d_feat / d_count is NULL"
POS = "R, F_total and n_total must be positive"
ROWS += [(e, dict(feat=NULL), INV, NULLS), (e, dict(count=NULL), INV, NULLS),
         (e, dict(R=0), INV, POS), (e, dict(F=0), INV, POS), (e, dict(n=0), INV, POS),
         (e, dict(on=0), INV, EP), (e, dict(on=6), INV, EP), (e, dict(off=1025), INV, EP),
         (e, dict(pre=-1), INV, PRE), (e, dict(max_frames=1), INV, PRE), (e, dict(max_frames=-2), INV, PRE),
         (e, dict(m=-1), INV, UTTS), (e, dict(utt=NULL), INV, UTTS), (e, dict(R=MANY, F=257), UNS, "more than 2^28 frames in one call"),
         # two faults
         (e, dict(on=6, pre=-1), INV, EP), (e, dict(feat=NULL, R=0), INV, NULLS), (e, dict(R=0, on=0), INV, POS),
         (e, dict(pre=-1, m=-1), INV, PRE), (e, dict(utt=NULL, R=MANY, F=257), INV, UTTS), (e, dict(off=1025, max_frames=1), INV, EP)]
e = "kws_segment_ragged_f32"
NULLS = "d_feat / d_count / frame_off / frames / len is NULL"
ROWSPEC = "frames and len must be positive and the recordings' rows must not overlap (frame_off ascending)"
ROWS += [(e, dict(feat=NULL), INV, NULLS), (e, dict(count=NULL), INV, NULLS), (e, dict(frame_off=NULL), INV, NULLS),
         (e, dict(frames=NULL), INV, NULLS), (e, dict(length=NULL), INV, NULLS),
         (e, dict(R=0), INV, "R must be positive"), (e, dict(R=MANY + 1), UNS, RECS),
         (e, dict(on=0), INV, EP), (e, dict(on=6), INV, EP), (e, dict(off=1025), INV, EP),
         (e, dict(pre=-1), INV, PRE), (e, dict(max_frames=1), INV, PRE), (e, dict(m=-1), INV, UTTS), (e, dict(utt=NULL), INV, UTTS),
         (e, dict(frames=i32(F, 0)), INV, ROWSPEC), (e, dict(length=i32(0, 3520)), INV, ROWSPEC), (e, dict(frame_off=i32(0, F - 1)), INV, ROWSPEC),
         (e, dict(frame_off=i32(0, 1 << 28)), UNS, "more than 2^28 rows in the packed frame array"),
         # two faults
         (e, dict(on=6, pre=-1), INV, EP), (e, dict(R=0, frame_off=NULL), INV, NULLS), (e, dict(R=MANY + 1, on=0), UNS, RECS),
         (e, dict(pre=-1, frame_off=i32(0, F - 1)), INV, PRE), (e, dict(utt=NULL, frames=i32(F, 0)), INV, UTTS),
         (e, dict(R=0, on=0), INV, "R must be positive"), (e, dict(pre=-1, m=-1), INV, PRE)]


def test_rows_cover_every_entry():
    assert {r[0] for r in ROWS} == set(CALLS)


@pytest.mark.parametrize("entry", list(CALLS))
def test_refusals_word_for_word(ctx, buf, entry):
    """Every row of the entry: the code and kws_last_error, byte for byte; afterwards no buffer was written."""
    bad = []
    for name, args, code, text in ROWS:
        if name != entry:
            continue
        rc = CALLS[entry](ctx._lib, ctx._h, buf, **args)
        got = ctx._lib.kws_last_error(ctx._h).decode()
        shown = {k: (list(v) if isinstance(v, ctypes.Array) else v) for k, v in args.items()}
        if (rc, got) != (code, f"{entry}: {text}"):
            bad.append(f"{shown}: ({rc}, {got!r}), expected ({code}, {entry + ': ' + text!r})")
        written = untouched(buf)
        if written:
            bad.append(f"{shown}: wrote {written}")
    assert not bad, "\n".join(bad)


def test_a_null_context_is_refused_without_a_text(buf):
    lib = _native.lib()
    for entry, call in CALLS.items():
        assert call(lib, None, buf) == INV, entry
    assert not untouched(buf)
