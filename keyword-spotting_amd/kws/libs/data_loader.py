"""Dataset wrapper + batched device collate.

Drop-in for ``kws/libs/data_loader.py``: ``SpeechCommandsDataLoader(dataset, audio_processor, split)``
with ``__len__``, ``__getitem__ -> (float32[1,99,10], int)`` and ``get_class_mapping`` (``:14-123``).
``collate_pcm16`` is the batched path: it packs int16 clips into one pinned host buffer, copies once
and computes all MFCCs in a single kernel launch, producing the same ``float32[B,1,T,F]`` /
``int64[B]`` pair torch's default collate builds from per-sample ``__getitem__`` calls
(reference ``train.py:108-121``).  ``DeviceBatchLoader`` is the training route: the split's PCM lives in device
memory and every augmented batch is produced there, with no per-batch host work and no worker processes.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from kws.common.errors import DatasetError, handle_error
from kws.libs.audio_processor import SILENCE_INDEX, AudioProcessor, fix_length, load_pcm16


class SpeechCommandsDataLoader(Dataset):
    VALID_SPLITS = ["training", "validation", "testing"]

    def __init__(self, dataset, audio_processor: AudioProcessor, split: str = "training") -> None:
        try:
            self.ap = audio_processor
            self.word_to_index = dataset.word_to_index
            if split not in self.VALID_SPLITS:
                raise DatasetError(f"Invalid split: {split}. Must be one of {self.VALID_SPLITS}")
            self.data = dataset.get_data(split)
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        except Exception as e:
            handle_error(e, DatasetError, f"Failed to initialize data loader for {split} split")

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, index: int) -> Tuple[torch.Tensor, int]:
        if index >= len(self.data):
            raise IndexError(f"Index {index} out of bounds for dataset of size {len(self.data)}")
        try:
            sample = self.data[index]
            label_idx = self.word_to_index[sample["label"]]
            feats = self.ap.transform(sample["file"], label_idx)
            return torch.tensor(feats, dtype=torch.float32).unsqueeze(0), label_idx
        except Exception as e:
            handle_error(e, DatasetError, f"Error processing sample at index {index}", re_raise=True)

    def get_class_mapping(self) -> Dict[int, str]:
        return {idx: word for word, idx in self.word_to_index.items()}

    # ------------------------------------------------------------------ batched path
    def _pcm16_clip(self, index: int) -> np.ndarray:
        """File ``index`` of the split as ``int16[n]``: mono mix-down, trimmed or zero-padded to the clip length."""
        clip = load_pcm16(self.data[index]["file"], self.ap.config.sample_rate)
        if clip.ndim == 2:
            clip = clip.astype(np.int32).mean(axis=1).astype(np.int16)
        return fix_length(clip, self.ap.config.desired_samples)

    def collate_pcm16(self, indices: Sequence[int], device=None):
        """Un-augmented batch for evaluation/inference: files -> int16 [B,n] (pinned) -> one H2D copy ->
        one MFCC launch.  Returns (``float32[B,1,T,F]`` on the device, ``int64[B]`` labels)."""
        n = self.ap.config.desired_samples
        pcm = torch.empty((len(indices), n), dtype=torch.int16).pin_memory() if torch.cuda.is_available() else torch.empty((len(indices), n), dtype=torch.int16)
        labels: List[int] = []
        for row, i in enumerate(indices):
            pcm[row] = torch.from_numpy(self._pcm16_clip(i).copy())
            labels.append(self.word_to_index[self.data[i]["label"]])
        dev = device or torch.device("cuda", self.ap.device)
        feats = self.ap.extract_features_batch(pcm.to(dev, non_blocking=True))
        return feats, torch.tensor(labels, dtype=torch.int64, device=dev)


class ResidentClips:
    """What ``DeviceBatchLoader.from_arrays`` exposes as ``.dataset``: the clip count and the host labels."""

    def __init__(self, labels: np.ndarray) -> None:
        self.labels = labels

    def __len__(self) -> int:
        return len(self.labels)


class DeviceBatchLoader:
    """Training batches from a split that lives in device memory.

    Replaces ``DataLoader(SpeechCommandsLoader(...), batch_size=1028, shuffle=True, num_workers=8, pin_memory=True)``
    (reference ``train.py:108-121``): iteration yields the ``(float32[B,1,frames,numcep], int64[B])`` pairs torch's
    default collate builds from the reference's ``__getitem__`` (``kws/libs/data_loader.py:96-105``), on the device.
    Construction decodes every file once (threads, never processes) and uploads ``int16[N, n]``, the labels and the
    background pool; ``nbytes`` is what that takes.  Per batch the host slices the epoch's permutation (already on the
    device), makes two ABI calls -- ``kws_augment_draw`` and ``kws_mfcc_augment_i16`` -- and one ``index_select`` for the
    labels: no synchronisation, no NumPy, everything on torch's current stream.

    A clip's random draws are a pure function of ``(seed, epoch, dataset index)``; the order is
    ``torch.randperm(N)`` from a generator seeded with ``(seed, epoch)``.  Each ``__iter__`` starts the next epoch
    (``set_epoch`` overrides it).  ``augment=True`` is the default for every split because the reference's ``transform``
    augments whatever the split is (``audio_processor.py:130-165``); ``augment=False`` gives the features of
    ``collate_pcm16``, bit for bit.

    Where the fused kernel does not apply (float64 front end, ``nfft != 512``) the loader composes ``index_select``,
    ``kws_augment_i16`` and ``kws_mfcc_f32`` with the same device draws; ``fused`` says which route is active.
    """

    def __init__(self, source: SpeechCommandsDataLoader, batch_size: int, shuffle: bool = True, drop_last: bool = False,
                 seed: int = 0, augment: bool = True, device=None) -> None:
        n_clips = len(source)
        if n_clips == 0:
            raise DatasetError("DeviceBatchLoader: the split is empty")
        self._require_gpu()
        labels = np.array([source.word_to_index[s["label"]] for s in source.data], dtype=np.int64)
        pcm = np.empty((n_clips, source.ap.config.desired_samples), dtype=np.int16)

        def decode(i: int) -> None:
            pcm[i] = source._pcm16_clip(i)

        try:
            with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
                list(pool.map(decode, range(n_clips)))
        except Exception as e:
            handle_error(e, DatasetError, "DeviceBatchLoader: decoding the split failed")
        self._setup(pcm, labels, source.ap, source, batch_size, shuffle, drop_last, seed, augment, device)

    @classmethod
    def from_arrays(cls, pcm, labels, audio_processor: AudioProcessor, batch_size: int, shuffle: bool = True,
                    drop_last: bool = False, seed: int = 0, augment: bool = True, device=None) -> "DeviceBatchLoader":
        """The same loader over clips already decoded: ``pcm int16[N, n]`` with ``n == config.desired_samples``."""
        self = cls.__new__(cls)
        labels = np.asarray(labels)
        self._setup(np.asarray(pcm), labels.astype(np.int64), audio_processor, ResidentClips(labels), batch_size, shuffle,
                    drop_last, seed, augment, device)
        return self

    @staticmethod
    def _require_gpu() -> None:
        if not torch.cuda.is_available():
            raise DatasetError("DeviceBatchLoader needs a ROCm GPU: the split lives in device memory and there is no CPU fallback")

    def _setup(self, pcm, labels, ap, dataset, batch_size, shuffle, drop_last, seed, augment, device) -> None:
        c = ap.config
        if int(batch_size) < 1:
            raise DatasetError("DeviceBatchLoader: batch_size must be at least 1")
        if pcm.dtype != np.int16 or pcm.ndim != 2 or pcm.shape[1] != c.desired_samples:
            raise DatasetError(f"DeviceBatchLoader: pcm must be int16[N, {c.desired_samples}]")
        if pcm.shape[0] == 0:
            raise DatasetError("DeviceBatchLoader: the split is empty")
        if labels.shape != (pcm.shape[0],):
            raise DatasetError("DeviceBatchLoader: one label per clip is required")
        self._require_gpu()
        dev = torch.device("cuda", ap.device)
        if device is not None and torch.device(device) not in (dev, torch.device("cuda")):
            raise DatasetError(f"DeviceBatchLoader: the audio processor computes on {dev}, not on {device}")
        self.ap, self.dataset, self.device = ap, dataset, dev
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.augment = int(seed), bool(augment)
        self.epoch, self._next_epoch = -1, 0
        n = c.desired_samples
        self._ctx = ap._context(n, c.sample_rate, c.num_cepstral_coeffs, c.frame_length, c.frame_step, c.num_mel_filters)
        self._shape = self._ctx.frontend_shape()
        # the pool is mixed into every clip, or -- without use_background_noise -- into silence clips only (audio_processor.py:158)
        pool = starts = lens = None
        if self.augment and ap.background_data and (c.use_background_noise or bool((labels == SILENCE_INDEX).any())):
            pool, starts, lens = ap.background_pool(n)
        self.nbytes = pcm.nbytes + 12 * len(labels) + (pool.nbytes if pool is not None else 0)
        try:
            self._pcm = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
            self._labels = torch.from_numpy(labels).to(dev)
            self._labels32 = self._labels.to(torch.int32)
            self._bg = torch.from_numpy(pool).to(dev) if pool is not None else None
            self._bg_start = torch.from_numpy(np.asarray(starts, dtype=np.int32)).to(dev) if pool is not None else None
            self._bg_len = torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(dev) if pool is not None else None
            B = min(self.batch_size, len(labels))
            self._shift = torch.empty(B, dtype=torch.int32, device=dev)
            self._off = torch.empty(B, dtype=torch.int32, device=dev)
            self._vol = torch.empty(B, dtype=torch.float32, device=dev)
            self._sil = torch.empty(B, dtype=torch.uint8, device=dev)
        except RuntimeError as e:
            raise DatasetError(f"DeviceBatchLoader: the split needs {self.nbytes} bytes of device memory: {e}") from e
        # which route: ask the fused entry once, for one clip
        from kws import _native

        self._ctx.use_torch_stream()
        probe = torch.empty((1, 1) + self._shape, dtype=torch.float32, device=dev)
        self.fused = self._ctx.mfcc_augment_i16(self._pcm, torch.zeros(1, dtype=torch.int32, device=dev), probe) == _native.KWS_OK

    def __len__(self) -> int:
        n, b = len(self.dataset), self.batch_size
        return n // b if self.drop_last else (n + b - 1) // b

    def set_epoch(self, epoch: int) -> None:
        """The next ``__iter__`` runs epoch ``epoch`` (order and draws), the ones after it ``epoch + 1, ...``."""
        self._next_epoch = int(epoch)

    def _order(self, epoch: int):
        n = len(self.dataset)
        if not self.shuffle:
            return torch.arange(n, dtype=torch.int32, device=self.device)
        g = torch.Generator()
        g.manual_seed((self.seed * 0x9E3779B97F4A7C15 + epoch) & 0x7FFFFFFFFFFFFFFF)
        return torch.randperm(n, generator=g).to(self.device, dtype=torch.int32)

    def _batch(self, idx, epoch: int):
        ctx, c, B = self._ctx, self.ap.config, idx.numel()
        out = torch.empty((B, 1) + self._shape, dtype=torch.float32, device=self.device)
        labels = self._labels.index_select(0, idx)
        ctx.use_torch_stream()
        kw = {}
        if self.augment:
            shift, off, vol, sil = self._shift[:B], self._off[:B], self._vol[:B], self._sil[:B]
            ctx.augment_draw(self.seed, epoch, idx, shift, off, vol, sil, labels=self._labels32, time_shift=c.time_shift,
                             bg_start=self._bg_start, bg_len=self._bg_len, bg_volume=c.background_volume,
                             bg_frequency=c.background_frequency, use_background=c.use_background_noise, n_samples=c.desired_samples)
            kw = dict(shift=shift, silence=sil)
            if self._bg is not None:
                kw.update(bg=self._bg, bg_off=off, bg_vol=vol)
        if self.fused:
            ctx.mfcc_augment_i16(self._pcm, idx, out, **kw)
        else:  # the composed route: the same draws through the separate kernels
            rows = self._pcm.index_select(0, idx)
            if self.augment:
                sig = torch.empty(rows.shape, dtype=torch.float32, device=self.device)
                ctx.augment_i16(rows, sig, **kw)
                ctx.mfcc_f32(sig, out)
            else:
                ctx.mfcc_i16(rows, out)
        return out, labels

    def __iter__(self):
        epoch = self.epoch = self._next_epoch
        self._next_epoch = epoch + 1
        order = self._order(epoch)
        for k in range(len(self)):
            yield self._batch(order[k * self.batch_size:(k + 1) * self.batch_size], epoch)
