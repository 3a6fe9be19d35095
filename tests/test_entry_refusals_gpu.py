"""What the C entry points refuse, word for word, and what they launch.

The fused clip entries (kws_infer_*), the cnn-trad-fpool3 forwards, the scans and the two stream pushes each refuse on the host,
before any launch, with a return code and a text that starts with the entry's own name.  The table below holds those texts as
literals, per context state, and the test compares kws_last_error byte for byte: the C symbols are called directly because
Context._check wraps the text.  Where two refusals apply at once the row pins which one wins.  One positive case counts the
launches kws_prof_read reports per kernel id for a fixed series of calls on both models."""
import pytest
import torch

from kws import _native
from oracle import cnn_trad as o_ct
from oracle import dscnn as o_dscnn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EINVAL, ESTATE, EUNSUPPORTED = _native.KWS_EINVAL, _native.KWS_ESTATE, _native.KWS_EUNSUPPORTED
NC = 12
HOP = 160


# ---- context states ---------------------------------------------------------------------------------------------------------------
def _load(ctx, dscnn=0, cnn_trad=False):
    if dscnn:
        ctx.load_dscnn(o_dscnn.flatten_state(o_dscnn.random_state(3, num_classes=NC, input_channels=dscnn)), NC, dscnn)
    if cnn_trad:
        ctx.load_cnn_trad(o_ct.flatten_state(o_ct.random_state(1, num_classes=NC)), NC)


def _step_armed_set(ctx, buf):
    """Arm live utterances on the open set and step them once with kws_stream_utt_step_i16: from then on a push is refused."""
    H = _native.host_stream_utt_history(400, HOP, 4, 12, 0)
    assert ctx._lib.kws_stream_utt_open(ctx._h, 0.0, 3, 5, 4, 12, H, 1) == 0, ctx._lib.kws_last_error(ctx._h)
    assert ctx._lib.kws_stream_utt_step_i16(ctx._h, buf["hop"].data_ptr(), None) == 0, ctx._lib.kws_last_error(ctx._h)


# name -> (DS-CNN input channels or 0, cnn-trad-fpool3 loaded, n_samples of the front end, stream set open, armed set stepped);
# 15840 samples are 98 frames: a map that is not 99 x 10
STATES = {
    "fresh": (0, False, 16000, False, False),
    "fresh+streams": (0, False, 16000, True, False),
    "dscnn": (1, False, 16000, False, False),
    "dscnn+streams": (1, False, 16000, True, False),
    "cnn_trad": (0, True, 16000, False, False),
    "cnn_trad+streams": (0, True, 16000, True, False),
    "dscnn2ch": (2, False, 16000, False, False),
    "dscnn2ch+streams": (2, False, 16000, True, False),
    "98frames": (1, True, 15840, False, False),
    "98frames+streams": (1, True, 15840, True, False),
    "98frames+dscnn2ch+streams": (2, True, 15840, True, False),
    "both+stepped": (1, True, 16000, True, True),
    "fresh+stepped": (0, False, 16000, True, True),
}


def _make(state, buf):
    dscnn, cnn_trad, n_samples, streams, stepped = STATES[state]
    ctx = _native.Context(0)
    try:
        _load(ctx, dscnn, cnn_trad)
        if n_samples != 16000:
            ctx.set_frontend(n_samples=n_samples)
        if streams:
            ctx.stream_open(1)  # after set_frontend, which retires an open set
        if stepped:
            _step_armed_set(ctx, buf)
        ctx.sync()
    except Exception:
        ctx.close()
        raise
    return ctx


@pytest.fixture(scope="module")
def buf():
    """One clip of every input kind, S = 1; no refused call reads or writes them."""
    b = {
        "i16": torch.zeros((1, 16000), dtype=torch.int16, device=DEV),
        "f32": torch.zeros((1, 16000), dtype=torch.float32, device=DEV),
        "feat": torch.zeros((1, 1, 99, 10), dtype=torch.float32, device=DEV),
        "frames": torch.zeros((1, 100, 10), dtype=torch.float32, device=DEV),
        "hop": torch.zeros((1, HOP), dtype=torch.int16, device=DEV),
        "logits": torch.zeros((8, NC), dtype=torch.float32, device=DEV),
        "conv2": torch.zeros((64 * 297,), dtype=torch.float32, device=DEV),
    }
    torch.cuda.synchronize()
    return b


# ---- the calls --------------------------------------------------------------------------------------------------------------------
def _call(ctx, buf, entry, inp=True, logits=True, B=1, conv2=True, F=99, hop_frames=1):
    """entry(...) with one clip (or S = 1); inp / logits / conv2 = False pass NULL, B is the batch or the recording count."""
    lib, h = ctx._lib, ctx._h
    lg = buf["logits"].data_ptr() if logits else None
    p = lambda key: buf[key].data_ptr() if inp else None
    if entry in ("kws_infer_i16", "kws_infer_cnn_trad_i16"):
        return getattr(lib, entry)(h, p("i16"), B, lg, None)
    if entry in ("kws_infer_f32", "kws_infer_cnn_trad_f32"):
        return getattr(lib, entry)(h, p("f32"), B, lg, None)
    if entry == "kws_forward_cnn_trad_f32":
        return lib.kws_forward_cnn_trad_f32(h, p("feat"), B, lg, None)
    if entry == "kws_forward_cnn_trad_debug_f32":
        return lib.kws_forward_cnn_trad_debug_f32(h, p("feat"), B, lg, None, buf["conv2"].data_ptr() if conv2 else None, None)
    if entry == "kws_forward_cnn_trad_windows_f32":
        return lib.kws_forward_cnn_trad_windows_f32(h, p("frames"), B, F, hop_frames, lg, None)
    if entry in ("kws_scan_i16", "kws_scan_cnn_trad_i16"):
        return getattr(lib, entry)(h, p("i16"), B, 16000, hop_frames, lg, None, None)
    if entry == "kws_stream_push_i16":
        return lib.kws_stream_push_i16(h, p("hop"), lg, None, 0)
    if entry == "kws_stream_push_cnn_trad_i16":
        return lib.kws_stream_push_cnn_trad_i16(h, p("hop"), lg, None)
    raise KeyError(entry)


NULL_IN, NULL_LOGITS, B0 = dict(inp=False), dict(logits=False), dict(B=0)
INFER = ["kws_infer_i16", "kws_infer_f32", "kws_infer_cnn_trad_i16", "kws_infer_cnn_trad_f32"]
STEPPED = ": this utterance set was stepped by kws_stream_utt_step_i16; a push would let its two counters drift apart"
ONE_CHANNEL = ": the MFCC front end yields one channel; the model was loaded with more"

# (state, entry, arguments, code, text): the texts are those of the sources before the entries shared their code
ROWS = []
# the argument checks come first in every entry, whatever the state
for e in INFER + ["kws_forward_cnn_trad_f32"]:
    ROWS += [("fresh", e, NULL_IN, EINVAL, e + ": input pointer is NULL"),
             ("fresh", e, B0, EINVAL, e + ": B must be positive"),
             ("fresh", e, dict(inp=False, B=0), EINVAL, e + ": input pointer is NULL")]
# the fused clip entries: readiness, then what the model asks of the front end; d_logits is looked at by the forward only
for e in ("kws_infer_i16", "kws_infer_f32"):
    ROWS += [("fresh", e, {}, ESTATE, e + ": front end or model not configured"),
             ("fresh", e, NULL_LOGITS, ESTATE, e + ": front end or model not configured"),
             ("cnn_trad", e, {}, ESTATE, e + ": front end or model not configured"),
             ("dscnn2ch", e, {}, EUNSUPPORTED, e + ONE_CHANNEL),
             ("dscnn2ch", e, NULL_LOGITS, EUNSUPPORTED, e + ONE_CHANNEL),
             ("dscnn2ch", e, B0, EINVAL, e + ": B must be positive")]
for e in ("kws_infer_cnn_trad_i16", "kws_infer_cnn_trad_f32"):
    ROWS += [("fresh", e, {}, ESTATE, e + ": front end or model not configured (kws_load_cnn_trad)"),
             ("fresh", e, NULL_LOGITS, ESTATE, e + ": front end or model not configured (kws_load_cnn_trad)"),
             ("dscnn", e, {}, ESTATE, e + ": front end or model not configured (kws_load_cnn_trad)"),
             ("98frames", e, {}, EUNSUPPORTED, e + ": the kernels are built for a 99 x 10 feature map"),
             ("98frames", e, NULL_IN, EINVAL, e + ": input pointer is NULL")]
# the cnn-trad-fpool3 forwards: d_logits before the model
e = "kws_forward_cnn_trad_f32"
ROWS += [("fresh", e, {}, ESTATE, e + ": no model loaded (kws_load_cnn_trad)"),
         ("dscnn", e, {}, ESTATE, e + ": no model loaded (kws_load_cnn_trad)"),
         ("fresh", e, NULL_LOGITS, EINVAL, e + ": d_logits is NULL"),
         ("cnn_trad", e, NULL_LOGITS, EINVAL, e + ": d_logits is NULL")]
e = "kws_forward_cnn_trad_debug_f32"
ROWS += [("cnn_trad", e, dict(conv2=False), EINVAL, e + ": d_conv2 is NULL"),
         ("fresh", e, dict(conv2=False, inp=False, B=0), EINVAL, e + ": d_conv2 is NULL"),
         ("cnn_trad", e, NULL_IN, EINVAL, e + ": input pointer is NULL"),
         ("cnn_trad", e, B0, EINVAL, e + ": B must be positive"),
         ("cnn_trad", e, NULL_LOGITS, EINVAL, e + ": d_logits is NULL"),
         ("fresh", e, {}, ESTATE, e + ": no model loaded (kws_load_cnn_trad)")]
e = "kws_forward_cnn_trad_windows_f32"
ROWS += [("cnn_trad", e, dict(F=98, hop_frames=0), EINVAL, e + ": R and hop_frames must be positive"),
         ("cnn_trad", e, dict(F=98, hop_frames=0, logits=False), EINVAL, e + ": d_frames / d_logits is NULL"),
         ("cnn_trad", e, dict(F=98, hop_frames=0, inp=False), EINVAL, e + ": d_frames / d_logits is NULL"),
         ("cnn_trad", e, dict(F=98, hop_frames=1, B=0), EINVAL, e + ": R and hop_frames must be positive"),
         ("cnn_trad", e, dict(F=98, hop_frames=1), EINVAL, e + ": a recording of fewer than 99 frames has no window"),
         ("fresh", e, dict(F=98, hop_frames=1), EINVAL, e + ": a recording of fewer than 99 frames has no window"),
         ("fresh", e, dict(F=100, hop_frames=1), ESTATE, e + ": no model loaded (kws_load_cnn_trad)"),
         ("dscnn", e, dict(F=100, hop_frames=1), ESTATE, e + ": no model loaded (kws_load_cnn_trad)")]
# the scans (one entry per model: the i16 / f32 and the ragged entries share the flow)
e = "kws_scan_i16"
ROWS += [("dscnn", e, NULL_IN, EINVAL, e + ": d_pcm / d_logits is NULL"),
         ("dscnn", e, NULL_LOGITS, EINVAL, e + ": d_pcm / d_logits is NULL"),
         ("dscnn", e, B0, EINVAL, e + ": R, n_total and hop_frames must be positive"),
         ("fresh", e, dict(hop_frames=0), EINVAL, e + ": R, n_total and hop_frames must be positive"),
         ("fresh", e, {}, ESTATE, e + ": front end or model not configured"),
         ("cnn_trad", e, {}, ESTATE, e + ": front end or model not configured"),
         ("98frames", e, {}, EUNSUPPORTED, e + ": the strided DS-CNN kernel is built for windows of 99 x 10 features"),
         ("98frames+dscnn2ch+streams", e, {}, EUNSUPPORTED, e + ": the strided DS-CNN kernel is built for windows of 99 x 10 features"),
         ("dscnn2ch", e, {}, EUNSUPPORTED, e + ONE_CHANNEL)]
e = "kws_scan_cnn_trad_i16"
ROWS += [("cnn_trad", e, NULL_IN, EINVAL, e + ": d_pcm / d_logits is NULL"),
         ("cnn_trad", e, NULL_LOGITS, EINVAL, e + ": d_pcm / d_logits is NULL"),
         ("cnn_trad", e, B0, EINVAL, e + ": R, n_total and hop_frames must be positive"),
         ("fresh", e, {}, ESTATE, e + ": front end or model not configured (kws_load_cnn_trad)"),
         ("dscnn", e, {}, ESTATE, e + ": front end or model not configured (kws_load_cnn_trad)"),
         ("98frames", e, {}, EUNSUPPORTED, e + ": the kernels are built for a 99 x 10 feature map")]
# the pushes: the set, the arguments, the model (only where logits are asked for), the armed set's driver
e = "kws_stream_push_i16"
ROWS += [("dscnn", e, {}, ESTATE, e + ": call kws_stream_open first"),
         ("fresh", e, NULL_IN, ESTATE, e + ": call kws_stream_open first"),
         ("dscnn+streams", e, NULL_IN, EINVAL, e + ": d_hop is NULL"),
         ("fresh+streams", e, NULL_IN, EINVAL, e + ": d_hop is NULL"),
         ("fresh+streams", e, {}, ESTATE, e + ": no model loaded (kws_load_dscnn)"),
         ("cnn_trad+streams", e, {}, ESTATE, e + ": no model loaded (kws_load_dscnn)"),
         ("dscnn2ch+streams", e, {}, EUNSUPPORTED, e + ": the model was loaded with more than one input channel"),
         ("98frames+streams", e, {}, EUNSUPPORTED, e + ": the DS-CNN kernel is built for a 99 x 10 feature map"),
         ("98frames+dscnn2ch+streams", e, {}, EUNSUPPORTED, e + ": the model was loaded with more than one input channel"),
         ("both+stepped", e, {}, ESTATE, e + STEPPED),
         ("both+stepped", e, NULL_LOGITS, ESTATE, e + STEPPED),
         ("both+stepped", e, NULL_IN, EINVAL, e + ": d_hop is NULL"),
         ("fresh+stepped", e, NULL_LOGITS, ESTATE, e + STEPPED),
         ("fresh+stepped", e, {}, ESTATE, e + ": no model loaded (kws_load_dscnn)")]
e = "kws_stream_push_cnn_trad_i16"
ROWS += [("cnn_trad", e, {}, ESTATE, e + ": call kws_stream_open first"),
         ("fresh", e, dict(inp=False, logits=False), ESTATE, e + ": call kws_stream_open first"),
         ("cnn_trad+streams", e, NULL_IN, EINVAL, e + ": d_hop / d_logits is NULL"),
         ("cnn_trad+streams", e, NULL_LOGITS, EINVAL, e + ": d_hop / d_logits is NULL"),
         ("fresh+streams", e, NULL_LOGITS, EINVAL, e + ": d_hop / d_logits is NULL"),
         ("fresh+streams", e, {}, ESTATE, e + ": no model loaded (kws_load_cnn_trad)"),
         ("dscnn+streams", e, {}, ESTATE, e + ": no model loaded (kws_load_cnn_trad)"),
         ("98frames+streams", e, {}, EUNSUPPORTED, e + ": the kernels are built for a 99 x 10 feature map"),
         ("both+stepped", e, {}, ESTATE, e + STEPPED),
         ("both+stepped", e, NULL_LOGITS, EINVAL, e + ": d_hop / d_logits is NULL"),
         ("fresh+stepped", e, {}, ESTATE, e + ": no model loaded (kws_load_cnn_trad)")]


def test_rows_cover_every_state_and_entry():
    assert {r[0] for r in ROWS} == set(STATES)
    assert {r[1] for r in ROWS} == set(INFER) | {"kws_forward_cnn_trad_f32", "kws_forward_cnn_trad_debug_f32",
                                                 "kws_forward_cnn_trad_windows_f32", "kws_scan_i16", "kws_scan_cnn_trad_i16",
                                                 "kws_stream_push_i16", "kws_stream_push_cnn_trad_i16"}


@pytest.mark.parametrize("state", list(STATES))
def test_refusals_word_for_word(state, buf):
    """Every row of the state: the code and kws_last_error, byte for byte; afterwards nothing was pushed and nothing written."""
    ctx = _make(state, buf)
    try:
        bad = []
        for st, entry, args, code, text in ROWS:
            if st != state:
                continue
            rc = _call(ctx, buf, entry, **args)
            got = ctx._lib.kws_last_error(ctx._h).decode()
            if (rc, got) != (code, text):
                bad.append(f"{entry}{args}: ({rc}, {got!r}), expected ({code}, {text!r})")
        assert not bad, "\n".join(bad)
        ctx.sync()
        if STATES[state][3]:
            assert ctx.stream_state()[1] == 0, "a refused push took its hop"
        assert not buf["logits"].any()
    finally:
        ctx.close()


# ---- the launches -----------------------------------------------------------------------------------------------------------------
def test_launch_counts_per_kernel_id(buf):
    """Both models on one context, every launch timed: one kws_infer_i16, one kws_infer_cnn_trad_i16 (B = 1), one
    kws_forward_cnn_trad_windows_f32 over R = 1, F = 100, hop 1 (two windows, one chunk), three pushes of each model at S = 1.
    A windows call is 1 conv + 1 dense, a cnn-trad-fpool3 push 1 frame + 1 conv + 1 dense, a DS-CNN push that asks for logits one
    DS-CNN launch and no frame launch; a fused call is one MFCC launch, its refinement and the model's.  The counts are those of the sources
    before the entries shared their code."""
    ctx = _native.Context(0)
    try:
        _load(ctx, 1, True)
        ctx.stream_open(1)
        lib, h = ctx._lib, ctx._h
        assert lib.kws_prof_enable(h, 1) == 0 and lib.kws_prof_reset(h) == 0
        logits = torch.zeros((2, NC), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        ok = lambda rc: rc == 0 or pytest.fail(lib.kws_last_error(h).decode())
        ok(lib.kws_infer_i16(h, buf["i16"].data_ptr(), 1, logits.data_ptr(), None))
        ok(lib.kws_infer_cnn_trad_i16(h, buf["i16"].data_ptr(), 1, logits.data_ptr(), None))
        ok(lib.kws_forward_cnn_trad_windows_f32(h, buf["frames"].data_ptr(), 1, 100, 1, logits.data_ptr(), None))
        for _ in range(3):
            ok(lib.kws_stream_push_i16(h, buf["hop"].data_ptr(), logits.data_ptr(), None, 0))
        for _ in range(3):
            ok(lib.kws_stream_push_cnn_trad_i16(h, buf["hop"].data_ptr(), logits.data_ptr(), None))
        ctx.sync()
        got, k = {}, 0
        while _native.kernel_name(k):  # every kernel id the library knows: "" ends the list
            got[_native.kernel_name(k)] = ctx.prof_read(k)[1]
            k += 1
        assert ctx.stream_state()[1] == 6 and torch.isfinite(logits).all()
        assert got == {
            "kws_mfcc_i16_kernel": 2,
            "kws_dscnn_fwd_kernel": 1 + 3,
            "kws_cnntrad_conv_kernel": 1 + 1 + 3,
            "kws_cnntrad_dense_kernel": 1 + 1 + 3,
            "kws_stream_frame_kernel": 3,
            "kws_mfcc_f64_kernel": 0,
            "kws_mfcc_refine_kernel": 2,  # the float64 refinement's launch behind each MFCC launch (kws_set_frontend_refine's default)
            "kws_ds_load_stats_kernel": 0,
            "kws_ds_load_pack_kernel": 0,
            "kws_ds_load_fill_kernel": 0,
            "kws_resample_kernel": 0,
        }
    finally:
        ctx.close()
