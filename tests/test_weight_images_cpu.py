"""CPU tests of the device weight images: kws_host_dscnn_image / kws_host_cnn_trad_image (the exact words the loaders upload)
against a NumPy restatement of the layouts documented in csrc/kws_internal.h (DscnnWeights, CnnTradWeights), word for word, and
the by-value scalars exactly.

The restatement gathers each section with fancy indexing and splits whole arrays at once:
  bf16 triple  piece p = top 16 bits of the running remainder, three times (view(uint32) & 0xffff0000)
  f16 pair     hi = float16(x), lo = float16((x - hi) * s) in float32, x = w * 2^k; s = 1 (DS-CNN), 2^11 (cnn-trad-fpool3)
Eight values of one lane fill four words per piece: value 2i in the low half of word i, 2i + 1 in the high half."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO

native = pytest.importorskip("kws._native")

LANE = np.arange(64)[:, None]   # [lane, 1]
J = np.arange(8)[None, :]       # [1, j]
ROW = LANE & 31                 # MFMA 32x32x16: the row / column a lane serves
HALF = LANE >> 5                # ... and which eight of the sixteen k values


def _words(pieces16):
    """uint16 [..., 8] -> uint32 [..., 4]"""
    p = pieces16.astype(np.uint32)
    return p[..., 0::2] | (p[..., 1::2] << 16)


def bf16_triple(v):
    """float32 [..., lane, 8] -> uint32 [..., piece 3, lane, 4]"""
    r = np.ascontiguousarray(v, dtype=np.float32)
    out = []
    for _ in range(3):
        u = r.view(np.uint32) & np.uint32(0xFFFF0000)
        out.append(_words((u >> 16).astype(np.uint16)))
        r = r - u.view(np.float32)
    return np.stack(out, axis=-3)


def f16_pair(v, scale, resid):
    """float32 [..., lane, 8] -> uint32 [..., piece 2, lane, 4]"""
    with np.errstate(all="ignore"):
        x = np.ascontiguousarray(v, dtype=np.float32) * np.float32(scale)
        hi = x.astype(np.float16)
        lo = ((x - hi.astype(np.float32)) * np.float32(resid)).astype(np.float16)
    return np.stack([_words(hi.view(np.uint16)), _words(lo.view(np.uint16))], axis=-3)


def scale_exponent(w):
    """k with max|w| 2^k < 2^15 (0 for an all-zero or non-finite layer), clamped to +-100"""
    m = np.float32(np.max(np.abs(w)))
    if not (m > 0) or not np.isfinite(m):
        return 0
    return int(np.clip(15 - int(np.frexp(m)[1]), -100, 100))


def row_abs_bound(w2d):
    """largest row sum of |w| (one float64 chain per row, in order), rounded up"""
    sums = np.cumsum(np.abs(w2d.astype(np.float64)), axis=1)[:, -1]
    return np.float32(sums.max() * 1.0000002)


def _pad4(parts):
    n = sum(p.size for p in parts)
    parts.append(np.zeros(-n % 4, np.uint32))


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


# ---- DS-CNN ----------------------------------------------------------------------------------------------------------------------
def dscnn_image(blob, C, Cin):
    from oracle import dscnn as o_dscnn

    st, off = {}, 0
    for k, shp in o_dscnn.state_shapes(C, Cin).items():
        n = int(np.prod(shp))
        st[k] = blob[off:off + n].reshape(shp)
        off += n
    assert off == blob.size
    w1 = st["conv1.weight"].reshape(64, Cin, 100)
    dw_w = np.stack([st[f"dsconv{i}.depthwise.weight"].reshape(64, 9) for i in range(1, 5)])
    dw_b = np.stack([st[f"dsconv{i}.depthwise.bias"] for i in range(1, 5)])
    pw_w = np.stack([st[f"dsconv{i}.pointwise.weight"].reshape(64, 64) for i in range(1, 5)])
    pw_b = np.stack([st[f"dsconv{i}.pointwise.bias"] for i in range(1, 5)])
    one = Cin == 1

    # depthwise: channel pairs interleaved, 24 floats per pair: taps at 2t + (ch & 1), biases at 18 + (ch & 1), 4 pad
    dw = np.zeros((4, 32, 24), np.float32)
    dw[:, :, :18] = dw_w.reshape(4, 32, 2, 9).transpose(0, 1, 3, 2).reshape(4, 32, 18)
    dw[:, :, 18:20] = dw_b.reshape(4, 32, 2)

    # pointwise fragments [b][ct][m][lane][j]: cout = 32 ct + (lane & 31), cin = 16 m + 8 (lane >> 5) + j
    ct, m = np.arange(2)[:, None, None, None], np.arange(4)[None, :, None, None]
    pw_frag = pw_w[:, 32 * ct + ROW, 16 * m + 8 * HALF + J]
    k_pw = [scale_exponent(pw_w[b]) for b in range(4)]
    pw_pair = np.stack([f16_pair(pw_frag[b], np.ldexp(1.0, k_pw[b]), 1.0) for b in range(4)])

    # conv1 fragments [ct][kb][lane][j], two K orders over the taps of kernel rows 5 (lane >> 5) .. + 4
    ct, kb = np.arange(2)[:, None, None, None], np.arange(7)[None, :, None, None]
    co = np.broadcast_to(32 * ct + ROW, (2, 7, 64, 8))
    if one:
        w1p = np.concatenate([w1[:, 0, :], np.zeros((64, 1), np.float32)], axis=1)  # tap 100 = the zero padding of a K order
        # bf16 image: offset f = 8 kb + j walks 10 (kh % 5) + kw up to 50
        f = 8 * kb + J
        tap = np.where(f < 50, (f // 10 + 5 * HALF) * 10 + f % 10, 100)
        c1_split = bf16_triple(w1p[co, np.broadcast_to(tap, co.shape)])
        # f16 image: kb < 5: row kb, kw = j; kb = 5: row j >> 1, kw = 8 + (j & 1); kb = 6: row 4, kw = 8 + j for j < 2
        tap = np.empty((7, 64, 8), np.int64)
        tap[:5] = (5 * HALF + np.arange(5)[:, None, None]) * 10 + J
        tap[5] = (5 * HALF + (J >> 1)) * 10 + 8 + (J & 1)
        tap[6] = np.where(J < 2, (5 * HALF + 4) * 10 + 8 + J, 100)
        k_c1 = scale_exponent(w1)
        c1_pair = f16_pair(w1p[co, np.broadcast_to(tap, co.shape)], np.ldexp(1.0, k_c1), 1.0)
        c1_w = w1[:, 0, :].T
        c1_abs, c1_bmax = row_abs_bound(w1[:, 0, :]), np.float32(np.abs(st["conv1.bias"]).max())
    else:  # the fused kernel's conv1 images exist for the single-channel model only
        c1_split, c1_pair = np.zeros((2, 7, 3, 64, 4), np.uint32), np.zeros((2, 7, 2, 64, 4), np.uint32)
        c1_w, k_c1, c1_abs, c1_bmax = np.zeros((100, 64), np.float32), 0, np.float32(0), np.float32(0)

    parts = [_u32(c1_w), _u32(st["conv1.bias"]), _u32(dw), _u32(pw_w.transpose(0, 2, 1)), _u32(pw_b), _u32(st["fc.weight"]),
             _u32(st["fc.bias"])]
    _pad4(parts)
    parts += [bf16_triple(pw_frag).reshape(-1), c1_split.reshape(-1), _u32(w1.transpose(1, 2, 0)), _u32(blob)]
    _pad4(parts)
    parts += [pw_pair.reshape(-1), c1_pair.reshape(-1)]
    scalars = np.array([k_c1] + k_pw + [c1_abs, c1_bmax] + [row_abs_bound(dw_w[b]) for b in range(4)] +
                       list(np.abs(dw_b).max(axis=1)) + [row_abs_bound(pw_w[b]) for b in range(4)] + list(np.abs(pw_b).max(axis=1)),
                       dtype=np.float32)
    return np.concatenate(parts), scalars


def _dscnn_blob(seed, C, Cin):
    from oracle import dscnn as o_dscnn

    return o_dscnn.flatten_state(o_dscnn.random_state(seed, num_classes=C, input_channels=Cin))


def _golden_blob():
    return np.load(os.path.join(REPO, "tests", "golden", "e2e_golden.npz"))["he.blob"].astype(np.float32)


@pytest.mark.parametrize("C,Cin,seed", [(12, 1, 1), (35, 1, 2), (12, 3, 3), (1, 1, 4), (64, 1, 5), (12, 1, None)])
def test_dscnn_image_word_for_word(C, Cin, seed):
    blob = _golden_blob() if seed is None else _dscnn_blob(seed, C, Cin)
    words, scalars = native.host_dscnn_image(blob, C, Cin)
    want_words, want_scalars = dscnn_image(blob, C, Cin)
    assert words.shape == want_words.shape
    bad = np.flatnonzero(words != want_words)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[:5]}"
    assert scalars.tobytes() == want_scalars.tobytes(), (scalars, want_scalars)
    if Cin == 1:  # every section really carries weights
        assert np.count_nonzero(words[-2 * 7 * 2 * 64 * 4:]) > 1000 and scalars[5] > 0


# ---- cnn-trad-fpool3 -------------------------------------------------------------------------------------------------------------
FLAT = 64 * 297


def cnn_trad_image(blob, C):
    from oracle import cnn_trad as o_ct

    st, off = {}, 0
    for k, shp in o_ct.state_shapes(C).items():
        n = int(np.prod(shp))
        st[k] = blob[off:off + n].reshape(shp)
        off += n
    assert off == blob.size
    w1, w2, wl = st["conv1.weight"].reshape(64, 20, 8), st["conv2.weight"], st["lin.weight"]
    # conv1 [kb 10][ct 2][lane][j]: cout = 32 ct + (lane & 31), kernel row 2 kb + (lane >> 5), kernel columns j
    kb, ct = np.arange(10)[:, None, None, None], np.arange(2)[None, :, None, None]
    f1 = w1[32 * ct + ROW, 2 * kb + HALF, J]
    # conv2 [kk 40][cb 4][ct 2][lane][j]: tap kk = 4 kh + kw, cout as above, cin = 16 cb + 8 (lane >> 5) + j
    kk, cb, ct = np.arange(40)[:, None, None, None, None], np.arange(4)[None, :, None, None, None], np.arange(2)[None, None, :, None, None]
    f2 = w2[32 * ct + ROW, 16 * cb + 8 * HALF + J, kk >> 2, kk & 3]
    # lin [kb 1188][lane][j]: output lane & 31, inputs 16 kb + 8 (lane >> 5) + j
    fl = wl[ROW, 16 * np.arange(FLAT // 16)[:, None, None] + 8 * HALF + J]
    k = [scale_exponent(w) for w in (w1, w2, wl)]
    sw = [np.float32(np.ldexp(1.0, e)) for e in k]
    parts = [bf16_triple(f1).reshape(-1), bf16_triple(f2).reshape(-1), _u32(st["conv1.bias"]), _u32(st["conv2.bias"]),
             bf16_triple(fl).reshape(-1), _u32(st["lin.bias"]), _u32(st["dnn.weight"]), _u32(st["dnn.bias"]), _u32(st["fc.weight"]),
             _u32(st["fc.bias"])]
    _pad4(parts)
    parts += [f16_pair(f, s, 2048.0).reshape(-1) for f, s in zip((f1, f2, fl), sw)] + [_u32(blob)]
    _pad4(parts)
    one = np.float32(1)
    scalars = np.array([one / sw[0], one / sw[1], one / sw[2], row_abs_bound(w1.reshape(64, 160)), np.abs(st["conv1.bias"]).max(),
                        row_abs_bound(w2.reshape(64, 2560)), np.abs(st["conv2.bias"]).max()], dtype=np.float32)
    return np.concatenate(parts), scalars


def _cnn_trad_blob(C, kind):
    from kws.libs.models import CnnTradFpool3
    from oracle import cnn_trad as o_ct

    if kind == "zero":
        return np.zeros(sum(int(np.prod(s)) for s in o_ct.state_shapes(C).values()), np.float32)
    torch.manual_seed(3)  # the state of test_device_load_is_bit_identical_to_the_host_load
    state = {k: v.detach().clone() for k, v in CnnTradFpool3(C).state_dict().items()}
    state["conv2.weight"][0, 0, 0, 0] = 5e-41  # a subnormal weight, and a large one that sets conv2's scale
    state["conv2.weight"][1, 2, 3, 1] = -70000.0
    return o_ct.flatten_state(state)


@pytest.mark.parametrize("C,kind", [(12, "planted"), (35, "planted"), (12, "zero")])
def test_cnn_trad_image_word_for_word(C, kind):
    blob = _cnn_trad_blob(C, kind)
    words, scalars = native.host_cnn_trad_image(blob, C)
    want_words, want_scalars = cnn_trad_image(blob, C)
    assert words.shape == want_words.shape
    bad = np.flatnonzero(words != want_words)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[:5]}"
    assert scalars.tobytes() == want_scalars.tobytes(), (scalars, want_scalars)
    if kind == "zero":
        assert not words.any() and list(scalars) == [1, 1, 1, 0, 0, 0, 0]
    else:
        assert scalars[1] == 4.0  # 70000 < 2^17: conv2's scale is 2^-2
        assert blob[10240 + 64] == np.float32(5e-41) and 0 < blob[10240 + 64] < np.finfo(np.float32).tiny


def test_image_exports_check_their_arguments():
    from kws.common.errors import ModelError

    blob = _dscnn_blob(1, 12, 1)
    with pytest.raises(ModelError, match="expected 26444 floats"):
        native.host_dscnn_image(blob[:-1], 12)
    with pytest.raises(ModelError, match="num_classes must be in"):
        native.host_cnn_trad_image(blob, 65)
    C = native.C
    need = C.c_size_t(0)
    small = np.zeros(8, np.uint32)
    rc = native.lib().kws_host_dscnn_image(blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, 12, 1,
                                           small.ctypes.data_as(C.POINTER(C.c_uint32)), small.size, C.byref(need), None)
    assert rc == native.KWS_EINVAL and need.value > small.size and not small.any()
