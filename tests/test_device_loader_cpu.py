"""CPU tests of the resident training loader: the NumPy restatement of the device draws (Philox4x32-10 and the mapping of its
words, the oracle of tests/test_device_loader_gpu.py), the header / binding / class surface, and the refusal without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
SILENCE_INDEX = 0


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) on arrays:
    counter = four uint32 arrays, key = two uint32 values -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]), int(key[1])
    lo32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def below(u, m):
    """word -> integer in [0, m)"""
    return ((u.astype(np.uint64) * np.asarray(m, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def unit(u):
    """word -> float32 in [0, 1), exact"""
    return (u >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def draws(seed, epoch, index, labels, S, bg_starts, bg_lens, n, bg_volume, bg_frequency, use_background=True):
    """The draws kws_augment_draw documents (include/kws_hip.h) for the dataset indices ``index``:
    (shift int32, offset int32, volume float32, silence uint8).  labels: per dataset index, or None."""
    index = np.asarray(index, dtype=np.int64)
    w = philox4x32_10([index.astype(np.uint32), np.uint32(epoch), np.uint32(0), np.uint32(0)],
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    sil = np.zeros(len(index), bool) if labels is None else np.asarray(labels)[index] == SILENCE_INDEX
    shift = below(w[0], 2 * S) - S if S > 0 else np.zeros(len(index), np.int64)
    off, vol = np.zeros(len(index), np.int64), np.zeros(len(index), np.float32)
    K = len(bg_lens)
    if K:
        mixed = sil | bool(use_background)
        k = below(w[1], K)
        room = np.asarray(bg_lens, dtype=np.int64)[k] - n
        off = np.where(mixed, np.asarray(bg_starts, dtype=np.int64)[k] + below(w[2], np.maximum(room, 0)), 0)
        u, f = unit(w[3]), np.float32(bg_frequency)
        with np.errstate(divide="ignore", invalid="ignore"):
            scaled = (u / f).astype(np.float32) * np.float32(bg_volume)   # two float32 roundings
        vol = np.where(sil, u, np.where(u < f, scaled, np.float32(0))).astype(np.float32)
        vol = np.where(mixed, vol, np.float32(0)).astype(np.float32)
    return shift.astype(np.int32), off.astype(np.int32), vol, sil.astype(np.uint8)


def test_philox_known_answers():
    """The known answers of the Random123 distribution (kat_vectors, philox4x32 10 rounds)."""
    kat = [
        ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, want in kat:
        got = philox4x32_10([np.array([x], np.uint32) for x in ctr], key)
        assert " ".join(f"{int(x[0]):08x}" for x in got) == want


def test_draws_stay_in_range_and_follow_the_reference_distributions():
    N, n, S = 100_000, 16000, 1600
    bg_lens = [20000, 48000, 16001, 960000, 32000, 61234]
    bg_starts = np.cumsum([0] + bg_lens[:-1])
    volume, freq = 0.1, 0.8
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 12, N)
    idx = np.arange(N)
    shift, off, vol, sil = draws(1234, 3, idx, labels, S, bg_starts, bg_lens, n, volume, freq)
    assert np.array_equal(sil, (labels == SILENCE_INDEX).astype(np.uint8))
    assert shift.min() >= -S and shift.max() < S
    # every offset lies inside one file and leaves room for a whole clip
    k = np.searchsorted(bg_starts, off, side="right") - 1
    rel = off - bg_starts[k]
    assert (rel >= 0).all() and (rel < np.asarray(bg_lens)[k] - n).all()
    s = sil.astype(bool)
    assert (vol >= 0).all() and (vol[s] < 1).all() and (vol[~s] < np.float32(volume)).all()
    # background_frequency: the share of non-silence clips with noise, within four binomial standard deviations
    m = int((~s).sum())
    share = float((vol[~s] > 0).mean())
    assert abs(share - freq) <= 4 * np.sqrt(freq * (1 - freq) / m), share
    # the mixed volumes fill [0, background_volume): mean within four standard deviations of a uniform variable's
    mixed = vol[~s][vol[~s] > 0]
    assert abs(float(mixed.mean()) - volume / 2) <= 4 * (volume / np.sqrt(12)) / np.sqrt(len(mixed))
    # every shift value's count within five standard deviations of uniform
    counts = np.bincount(shift + S, minlength=2 * S)
    p = 1 / (2 * S)
    assert np.abs(counts - N * p).max() <= 5 * np.sqrt(N * p * (1 - p))
    # every file is chosen, about equally often
    fc = np.bincount(k, minlength=len(bg_lens))
    assert np.abs(fc - N / 6).max() <= 5 * np.sqrt(N * (1 / 6) * (5 / 6))
    # a pure function of (seed, epoch, index): order and company do not matter; epoch and seed do
    sub = rng.permutation(N)[:1000]
    again = draws(1234, 3, sub, labels, S, bg_starts, bg_lens, n, volume, freq)
    for a, b in zip(again, (shift, off, vol, sil)):
        assert np.array_equal(a, b[sub])
    assert not np.array_equal(draws(1234, 4, idx, labels, S, bg_starts, bg_lens, n, volume, freq)[0], shift)
    assert not np.array_equal(draws(1235, 3, idx, labels, S, bg_starts, bg_lens, n, volume, freq)[0], shift)
    # time_shift 0: no shift; no use_background_noise: noise in silence clips only; no pool: nothing
    z = draws(1234, 3, idx, labels, 0, bg_starts, bg_lens, n, volume, freq, use_background=False)
    assert not z[0].any() and not z[2][~s].any() and not z[1][~s].any() and (z[2][s] > 0).mean() > 0.99
    e = draws(1234, 3, idx, labels, S, [], [], n, volume, freq)
    assert not e[1].any() and not e[2].any()


def test_header_bindings_and_loader_surface():
    native = pytest.importorskip("kws._native")
    text = open(os.path.join(REPO, "include", "kws_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("kws_augment_draw", "kws_mfcc_augment_i16"):
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} is not declared in kws_hip.h"
        assert name in native.SIGNATURES
        assert hasattr(native.lib(), name)
    assert len(native.SIGNATURES["kws_augment_draw"][1]) == 19
    assert len(native.SIGNATURES["kws_mfcc_augment_i16"][1]) == 12
    # the documentation cites the reference lines the entries replace
    for cite in ("audio_processor.py:151-159, 172-233", "data_loader.py:96-105", "train.py:108-121"):
        assert cite in text

    from kws.libs.data_loader import DeviceBatchLoader

    p = inspect.signature(DeviceBatchLoader.__init__).parameters
    assert list(p) == ["self", "source", "batch_size", "shuffle", "drop_last", "seed", "augment", "device"]
    assert (p["shuffle"].default, p["drop_last"].default, p["seed"].default, p["augment"].default, p["device"].default) == \
        (True, False, 0, True, None)
    q = inspect.signature(DeviceBatchLoader.from_arrays).parameters
    assert list(q) == ["pcm", "labels", "audio_processor", "batch_size", "shuffle", "drop_last", "seed", "augment", "device"]
    for attr in ("__iter__", "__len__", "set_epoch"):
        assert hasattr(DeviceBatchLoader, attr)


def test_loader_refuses_bad_arguments_and_a_host_without_gpu():
    import torch

    from kws.common.errors import DatasetError
    from kws.libs.audio_processor import AudioProcessor
    from kws.libs.data_loader import DeviceBatchLoader

    ap = AudioProcessor(None)
    pcm, labels = np.zeros((4, 16000), np.int16), np.arange(4)
    with pytest.raises(DatasetError, match="batch_size"):
        DeviceBatchLoader.from_arrays(pcm, labels, ap, 0)
    with pytest.raises(DatasetError, match="int16"):
        DeviceBatchLoader.from_arrays(pcm.astype(np.float32), labels, ap, 2)
    with pytest.raises(DatasetError, match="int16"):
        DeviceBatchLoader.from_arrays(pcm[:, :8000], labels, ap, 2)
    with pytest.raises(DatasetError, match="empty"):
        DeviceBatchLoader.from_arrays(pcm[:0], labels[:0], ap, 2)
    with pytest.raises(DatasetError, match="one label per clip"):
        DeviceBatchLoader.from_arrays(pcm, labels[:3], ap, 2)
    if not torch.cuda.is_available():
        with pytest.raises(DatasetError, match="no CPU fallback"):
            DeviceBatchLoader.from_arrays(pcm, labels, ap, 2)
