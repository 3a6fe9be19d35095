"""wav -> label, the shape of the reference's ``inference(test_audio)``
(``kws/inference/inference_local.py:67-81``: load -> fix length to 1 s -> MFCC -> model -> argmax ->
word), on the fused MI355X path and for whole batches of files."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from kws.common.errors import AudioProcessingError, ModelError
from kws.datasets.speech_commands import DEFAULT_WORDS, SpeechCommandDataset
from kws.libs.audio_processor import AudioConfig, fix_length, load_audio, load_pcm16, read_wav
from kws.libs.models import DepthwiseSeparableConv, KeywordSpottingModel

WANTED_WORDS = [SpeechCommandDataset.SILENCE_LABEL, SpeechCommandDataset.UNKNOWN_LABEL] + DEFAULT_WORDS


WINDOW_FRAMES = 99  # frames per window of a scan: the model's clip length


def _round_half_up(x: float) -> int:
    return int(np.floor(x + 0.5))  # psf's rounding of winlen * samplerate


def scan_window_times(n_windows: int, hop_frames: int, frame_len: int = 400, frame_step: int = 160, sample_rate: int = 16000,
                      window_frames: int = WINDOW_FRAMES, n_total: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(start_s [W], end_s [W]) of a scan's windows: window w covers samples [w * hop_frames * frame_step,
    w * hop_frames * frame_step + (window_frames - 1) * frame_step + frame_len), clipped to ``n_total`` when given."""
    start = np.arange(int(n_windows), dtype=np.int64) * (int(hop_frames) * int(frame_step))
    end = start + (int(window_frames) - 1) * int(frame_step) + int(frame_len)
    if n_total is not None:
        end = np.minimum(end, int(n_total))
    return start / float(sample_rate), end / float(sample_rate)


@dataclass
class ScanResult:
    """What ``KeywordSpotter.scan`` returns.  ``events`` is None unless a threshold was given: one list per recording of
    ``(time_s, index, word, score)``, ``time_s`` being the end of the window that fired."""
    labels: np.ndarray           # int32 [R, W]
    logits: np.ndarray           # float32 [R, W, C]
    window_start_s: np.ndarray   # float64 [W]
    events: Optional[List[List[Tuple[float, int, str, float]]]] = None


UTTERANCE_REASONS = ("endpoint", "max_length", "end_of_recording")  # kws_segment_f32's reasons 0, 1, 2


@dataclass
class Utterance:
    """One utterance ``KeywordSpotter.segment`` found: where it lies in its recording (seconds), why it closed and what the
    model says about its normalised, one-second clip.  ``start_s`` is ``pre_roll`` frames before ``open_s``, the frame at which
    the endpointer triggered; ``end_s`` is the end of the closing frame ``close_s`` starts; ``peak`` is the largest sample
    magnitude of the span before normalisation: an int for int16 PCM, a float in full-scale units for float32 samples."""
    recording: int
    start_s: float
    end_s: float
    open_s: float
    close_s: float
    reason: str
    label: int
    word: str
    logits: np.ndarray  # float32 [C]
    peak: float  # int for int16 PCM


def _classify_spans(ctx, model, device, words, num_classes: int, clip_samples: int, rate: float, frame_step: int, rows, cut,
                    f32: bool = False) -> List[Utterance]:
    """The tail ``segment`` and ``pop_utterances`` share: ``rows`` of ``(recording, start, end, open, close, reason)``, samples
    and frames; ``cut(clips, peaks)`` launches the cut of row ``u`` into ``clips[u]`` and ``peaks[u]``.  Then the model once per
    clip (``model``'s fused entry, through its hooks) and ONE read of logits, labels and peaks.  ``f32``: float32 clips and peaks
    (``kws_cut_f32``, ``kws_infer_f32`` / ``kws_infer_cnn_trad_f32``)."""
    U, C = len(rows), num_classes
    clips = torch.empty((U, clip_samples), dtype=torch.float32 if f32 else torch.int16, device=device)
    out = torch.empty((U * (C + 2),), dtype=torch.float32, device=device)  # logits [U, C], then labels [U] (int32) and peaks [U]
    logits, ints = out[:U * C].view(U, C), out[U * C:].view(torch.int32)
    torch.cuda.current_stream(device).synchronize()  # a context may run on its own stream
    if f32:
        cut(clips, out[U * C + U:])
        model._native_infer_f32(ctx, clips, logits, ints[:U])
    else:
        cut(clips, ints[U:])
        model._native_infer_i16(ctx, clips, logits, ints[:U])
    ctx.sync()
    host = out.cpu()  # the one read
    logits, ints = host[:U * C].view(U, C).numpy(), host[U * C:].view(torch.int32).numpy()
    peaks = host[U * C + U:].numpy() if f32 else ints[U:]
    return [Utterance(int(r), int(start) / rate, int(end) / rate, int(opened) * frame_step / rate, int(closed) * frame_step / rate,
                      UTTERANCE_REASONS[int(reason)], int(ints[u]), words[int(ints[u])], logits[u].copy(),
                      float(peaks[u]) if f32 else int(peaks[u]))
            for u, (r, start, end, opened, closed, reason) in enumerate(rows)]


@dataclass
class UtteranceConfig:
    """``StreamingSpotter(utterances=...)``: the reference's live loop on the streams.  A frame is voiced when its log energy
    exceeds ``threshold``; an utterance opens when more than 80 % of the last ``on_window`` frames are voiced, closes when more
    than 90 % of the last ``off_window`` are not or after ``max_seconds`` (a live history is bounded: there is no "never"),
    starts ``pre_roll`` frames before it opened and is scaled to a peak of ``normalize`` (0: as it is) before the model sees it.
    ``max_events``: records the device queue keeps (None: ``max(n_streams, 64)``); ``slack_hops``: hops that may be pushed
    between a close and the ``pop_utterances`` that cuts it."""
    threshold: float
    on_window: int = 40
    off_window: int = 80
    pre_roll: int = 60
    max_seconds: float = 10.0
    normalize: int = 16384
    max_events: Optional[int] = None
    slack_hops: int = 8


@dataclass
class DetectConfig:
    """``StreamingSpotter(detect=...)``: the decision layer of ``KeywordSpotter.scan`` on the streams, one decision per push
    (``kws_stream_detect_open``).  The posteriors of every hop are averaged over the last ``smooth_window`` decisions; a stream
    fires when the top class is at least ``first_keyword`` (classes below it, _silence_ and _unknown_, never fire) and its
    smoothed posterior at least ``threshold``, and then stays quiet for ``refractory`` decisions.  ``max_events``: records the
    device queue keeps (None: ``max(n_streams, 64)``).  ``skip_partial_windows``: no decision before the one-second window holds
    99 real frames -- decision d is then window d of ``scan(pcm, hop_frames=1)`` over the same audio; False: every push decides,
    from the first."""
    threshold: float
    smooth_window: int = 1
    refractory: int = 50
    first_keyword: int = 2
    max_events: Optional[int] = None
    skip_partial_windows: bool = True


@dataclass
class KeywordEvent:
    """One event of ``StreamingSpotter.pop_events``: class ``index`` (``word``) fired on ``stream`` with the smoothed posterior
    ``score``.  ``time_s`` is the end of the window that fired, in seconds of the stream since the spotter was created at
    ``config.sample_rate`` -- the convention of ``ScanResult.events``; ``decision`` counts the decisions since the arming and
    ``hop`` the pushes (from 1)."""
    stream: int
    time_s: float
    index: int
    word: str
    score: float
    decision: int
    hop: int


class KeywordSpotter:
    """Holds a model on one GPU and maps wav files / PCM batches to (index, word).  ``model``: a ``DepthwiseSeparableConv`` (the
    default), a ``DepthwiseSeparableConvBN`` (served by its fold) or a ``CnnTradFpool3``; every method runs the model through its
    hooks (``kws/libs/models.py``), so clips, files, ``scan*`` and ``segment*`` work for all three."""

    def __init__(self, model: Optional[KeywordSpottingModel] = None, words: Sequence[str] = WANTED_WORDS,
                 config: Optional[AudioConfig] = None, device: int = 0):
        self.config = config or AudioConfig()
        self.words = list(words)
        self.model = model if model is not None else DepthwiseSeparableConv(num_classes=len(self.words))
        if self.model.num_classes != len(self.words):
            raise ModelError(f"model has {self.model.num_classes} classes but {len(self.words)} words were given")
        self.device = torch.device("cuda", device)

    def load_weights(self, path: str) -> None:
        self.model.load(path, device=torch.device("cpu"))  # parameters are packed from the host copy

    def infer_pcm16(self, pcm: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """``int16[B,n]`` host array -> (labels int32[B], logits float32[B,C]) through the library's host-ingest
        pipeline (``kws_infer_host_i16``: pack into pinned staging, H2D, MFCC + DS-CNN and D2H overlapped chunk by chunk).
        A ``CnnTradFpool3`` has no such pipeline: the batch is uploaded and classified by ``kws_infer_cnn_trad_i16``, with the same
        results and nothing overlapped."""
        clips = fix_length(np.atleast_2d(np.asarray(pcm, dtype=np.int16)), self.config.desired_samples)
        ctx = self.model._context(self.device.index or 0)
        if not self.model._host_ingest:
            return self._infer_uploaded(ctx, torch.from_numpy(np.ascontiguousarray(clips)))
        logits, labels = ctx.infer_host_i16(np.ascontiguousarray(clips))
        return labels, logits

    def _infer_uploaded(self, ctx, clips: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
        """One int16 (or float32) ``[B, n]`` batch: upload, the model's fused entry, read back -> (labels, logits)."""
        x = clips.to(self.device).contiguous()
        logits = torch.empty((x.shape[0], self.model.num_classes), dtype=torch.float32, device=self.device)
        labels = torch.empty((x.shape[0],), dtype=torch.int32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()  # a context may run on its own stream
        (self.model._native_infer_f32 if x.dtype == torch.float32 else self.model._native_infer_i16)(ctx, x, logits, labels)
        ctx.sync()
        return labels.cpu().numpy(), logits.cpu().numpy()

    def infer_batches(self, batches: Iterable[np.ndarray], max_batch: Optional[int] = None
                      ) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
        """Host ingest for many batches: every ``int16[B,n]`` host batch (numpy array, or a CPU
        torch tensor -- a pinned one is read by the DMA directly, without the pack stage) goes through the library's
        pipeline: a pool of host threads packs chunk k+1 into pinned staging while chunk k crosses PCIe on a copy stream,
        chunk k-1 runs MFCC + DS-CNN and the results of chunk k-2 return on a second copy stream.  The pipeline stays
        full ACROSS batches: batch k+1 is submitted (``kws_infer_host_submit_i16``) before batch k's results are waited
        for, so its pack and H2D run under batch k's kernels -- with the reference's own batch size (1028, ``train.py:110``)
        a batch is also cut into as many chunks as the ring has slots.  Yields ``(labels int32[B], logits float32[B,C])``
        per batch, in order.  ``max_batch``: clips per chunk of the staging ring (default 1024).

        A ``CnnTradFpool3`` has no host-ingest pipeline: every batch is uploaded and classified by ``kws_infer_cnn_trad_i16``
        before the next one is touched -- the same results in the same order, no pipelining; ``max_batch`` is ignored."""
        n = self.config.desired_samples
        ctx = self.model._context(self.device.index or 0)
        if not self.model._host_ingest:
            for batch in batches:
                src = batch if torch.is_tensor(batch) and batch.dtype == torch.int16 and batch.dim() == 2 and batch.shape[1] == n \
                    else torch.from_numpy(np.ascontiguousarray(fix_length(np.atleast_2d(np.asarray(batch, dtype=np.int16)), n)))
                yield self._infer_uploaded(ctx, src)
            return
        if max_batch:
            ctx.infer_host_wait(0)
            ctx.ingest_config(chunk_clips=int(max_batch))
        pending = None  # (logits, labels, ticket, keepalive) of the batch submitted last
        try:
            for batch in batches:
                if torch.is_tensor(batch) and batch.dtype == torch.int16 and batch.dim() == 2 and batch.shape[1] == n \
                        and not batch.is_cuda and batch.is_contiguous():
                    src = batch
                else:
                    src = np.ascontiguousarray(fix_length(np.atleast_2d(np.asarray(batch, dtype=np.int16)), n))
                nxt = ctx.infer_host_submit_i16(src)
                if pending is not None:
                    ctx.infer_host_wait(pending[2])
                    yield pending[1], pending[0]
                pending = nxt
            if pending is not None:
                ctx.infer_host_wait(pending[2])
                yield pending[1], pending[0]
                pending = None
        finally:
            if pending is not None:  # the consumer stopped early: nothing may stay in flight into freed arrays
                ctx.infer_host_wait(0)

    def infer_files(self, paths: Sequence[str], resample=False) -> List[Tuple[int, str]]:
        """wav files -> (index, word).  16-bit mono files at the configured rate go through the int16 path (the PCM
        itself is the device input); anything else -- other bit depths, float, stereo, and with ``resample=True`` other
        rates -- is decoded to float32 mono as ``librosa.load`` does and takes the float32 path (``kws_infer_f32``).
        ``resample="device"`` serves any rate on the device instead (``_infer_files_device``)."""
        if isinstance(resample, str):
            if resample != "device":
                raise AudioProcessingError(f"infer_files: resample must be False, True or 'device', got {resample!r}")
            return self._infer_files_device(paths)
        n = self.config.desired_samples
        clips, all_i16 = [], True
        for p in paths:
            try:
                x = load_pcm16(p, self.config.sample_rate)
                if x.ndim == 2:
                    raise ValueError("stereo: mix down in float")
            except Exception:
                x = load_audio(p, self.config.sample_rate, resample)
                all_i16 = False
            clips.append(fix_length(x, n))
        if all_i16:
            labels, _ = self.infer_pcm16(np.stack(clips))
        else:
            f32 = np.stack([c.astype(np.float32) / np.float32(32768.0) if c.dtype == np.int16 else c for c in clips])
            labels, _ = self.infer_f32(f32)
        return [(int(i), self.words[int(i)]) for i in labels]

    def _infer_files_device(self, paths: Sequence[str]) -> List[Tuple[int, str]]:
        """``infer_files(resample="device")``: every file is decoded at its own rate (``read_wav``: 16-bit mono stays int16,
        anything else is float32 mono) and the files are grouped by (rate, sample type).  A group is uploaded as one batch padded
        to its longest file, resampled to the configured rate and cut or zero-padded to a clip in ONE launch
        (``kws_resample_i16`` / ``kws_resample_f32`` with the true lengths and ``n_out = desired_samples``: ``fix_length`` after
        resampling, the reference's order) and classified where it lies (``kws_infer_i16`` / ``kws_infer_f32``).  Results come
        back in the order of ``paths``.  Parity against librosa's soxr resampler is unpinned, as with ``resample=True``."""
        cfg = self.config
        decoded = [read_wav(p) for p in paths]
        groups: dict = {}
        for i, (x, rate) in enumerate(decoded):
            groups.setdefault((rate, x.dtype == np.int16), []).append(i)
        ctx = self.model._context(self.device.index or 0)
        result = np.empty(len(decoded), np.int32)
        for (rate, is_i16), members in groups.items():
            clips = [decoded[i][0] for i in members]
            batch = np.zeros((len(clips), max(1, max(len(x) for x in clips))), np.int16 if is_i16 else np.float32)
            for row, x in zip(batch, clips):
                row[:len(x)] = x
            x = torch.from_numpy(batch).to(self.device)
            lengths = torch.tensor([len(c) for c in clips], dtype=torch.int32, device=self.device)
            y = torch.empty((len(clips), cfg.desired_samples), dtype=x.dtype, device=self.device)
            logits = torch.empty((len(clips), self.model.num_classes), dtype=torch.float32, device=self.device)
            labels = torch.empty((len(clips),), dtype=torch.int32, device=self.device)
            if is_i16:
                ctx.resample_i16(x, rate, cfg.sample_rate, y, lengths)
                self.model._native_infer_i16(ctx, y, logits, labels)
            else:
                ctx.resample_f32(x, rate, cfg.sample_rate, y, lengths)
                self.model._native_infer_f32(ctx, y, logits, labels)
            result[members] = labels.cpu().numpy()
        return [(int(i), self.words[int(i)]) for i in result]

    def infer_f32(self, signals: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """``float32[B,n]`` host signals in [-1, 1] -> (labels int32[B], logits float32[B,C]) (``kws_infer_f32``, for a
        ``CnnTradFpool3`` ``kws_infer_cnn_trad_f32``)."""
        x = torch.from_numpy(np.ascontiguousarray(fix_length(np.atleast_2d(np.asarray(signals, dtype=np.float32)),
                                                             self.config.desired_samples))).to(self.device)
        ctx = self.model._context(self.device.index or 0)
        logits = torch.empty((x.shape[0], self.model.num_classes), dtype=torch.float32, device=self.device)
        labels = torch.empty((x.shape[0],), dtype=torch.int32, device=self.device)
        self.model._native_infer_f32(ctx, x, logits, labels)
        return labels.cpu().numpy(), logits.cpu().numpy()


    def scan(self, pcm, hop_frames: int = 1, smooth_window: int = 1, threshold: Optional[float] = None, refractory: int = 50,
             first_keyword: int = 2, max_events: int = 1024, sample_rate: Optional[int] = None) -> ScanResult:
        """Where are the keywords in a recording longer than a clip?  ``pcm``: int16 ``[n]`` or ``[R, n]`` (R recordings of
        equal length), a host array or a device tensor.  One MFCC pass per recording, then the model on every window of 99
        frames, ``hop_frames`` frames (10 ms each) apart (``kws_scan_i16``).  With a ``threshold`` the windows' posteriors are
        smoothed over ``smooth_window`` windows and turned into events at least ``refractory`` windows apart, classes below
        ``first_keyword`` (_silence_, _unknown_) never firing (``kws_scan_detect_f32``); at most ``max_events`` per recording
        are returned.  A recording shorter than one window raises ``ModelError``.  ``sample_rate``: the rate of ``pcm`` when it
        is not the configured one; the recordings are then resampled on the device to their natural length at the configured
        rate (``kws_resample_i16``) and the result is scanned, so window and event times stay in seconds of the recording."""
        return self._scan(self._recordings(pcm, "scan"), "scan", hop_frames, smooth_window, threshold, refractory, first_keyword,
                          max_events, sample_rate)

    def scan_f32(self, signal, hop_frames: int = 1, smooth_window: int = 1, threshold: Optional[float] = None, refractory: int = 50,
                 first_keyword: int = 2, max_events: int = 1024, sample_rate: Optional[int] = None) -> ScanResult:
        """``scan`` for float32 samples in [-1, 1], the reference's native sample type: ``signal`` float32 ``[n]`` or ``[R, n]``, a
        host array or a device tensor, taken as it is -- nothing is quantised (``kws_scan_f32``; ``sample_rate`` goes through
        ``kws_resample_f32``).  For ``signal = pcm / 32768`` the result equals ``scan(pcm)`` bit for bit.  Anything that is not
        float32 raises ``ModelError``."""
        return self._scan(self._recordings(signal, "scan_f32", f32=True), "scan_f32", hop_frames, smooth_window, threshold, refractory,
                          first_keyword, max_events, sample_rate)

    def _frame_geometry(self) -> Tuple[int, int]:
        """(frame_len, frame_step) in samples at the configured rate."""
        cfg = self.config
        return _round_half_up(cfg.frame_length * cfg.sample_rate), _round_half_up(cfg.frame_step * cfg.sample_rate)

    @staticmethod
    def _decision_args(what: str, hop_frames, smooth_window, refractory, first_keyword, max_events=None, decide: bool = True) -> None:
        """The argument checks the scan and score methods share (no device needed): the hop, then -- when decisions are asked
        for -- the rules; ``max_events`` joins the last sentence for the methods that take it."""
        if int(hop_frames) < 1:
            raise ModelError(f"{what}: hop_frames must be at least 1")
        if not decide:
            return
        if not 1 <= int(smooth_window) <= 256:
            raise ModelError(f"{what}: smooth_window must be in [1, 256]")
        if int(refractory) < 1 or int(first_keyword) < 0 or (max_events is not None and int(max_events) < 0):
            rest = " and first_keyword >= 0" if max_events is None else ", first_keyword >= 0 and max_events >= 0"
            raise ModelError(f"{what}: need refractory >= 1{rest}")

    def _scan_logits(self, x: torch.Tensor, what: str, hop_frames, sample_rate, want_labels: bool):
        """Recordings ``[R, n]`` -> (ctx, logits [R, W, C] and labels [R, W] (or None) on the device, window start and end times,
        frame_step): the resampling, the shape refusal and the scan ``scan`` and ``score`` share."""
        from kws import _native

        cfg, hop = self.config, int(hop_frames)
        x = self._at_configured_rate(x, sample_rate, what)
        frame_len, frame_step = self._frame_geometry()
        R, n = int(x.shape[0]), int(x.shape[1])
        frames, W = (0, 0) if n < 1 else _native.host_scan_shape(n, frame_len, frame_step, WINDOW_FRAMES, hop)
        if W < 1:
            raise ModelError(f"{what}: a recording of {n} samples ({frames} frames) is shorter than one window of {WINDOW_FRAMES} frames")
        ctx = self.model._context(self.device.index or 0)
        x = x.to(self.device).contiguous()
        logits = torch.empty((R, W, self.model.num_classes), dtype=torch.float32, device=self.device)
        labels = torch.empty((R, W), dtype=torch.int32, device=self.device) if want_labels else None
        self.model._native_scan(ctx, x, hop, logits, labels)
        start_s, end_s = scan_window_times(W, hop, frame_len, frame_step, cfg.sample_rate, WINDOW_FRAMES, n)
        return ctx, logits, labels, start_s, end_s, frame_step

    def _events(self, detect, end_times, max_events) -> List[List[Tuple[float, int, str, float]]]:
        """The count and the three event arrays of R = ``len(end_times)`` recordings, ``detect(count, window, label, score,
        max_events)`` over them, the read-back, and per recording its events as ``(time_s, index, word, score)``;
        ``end_times[r]``: the end of each window of recording ``r`` in seconds."""
        R, m = len(end_times), int(max_events)
        count = torch.empty((R,), dtype=torch.int32, device=self.device)
        ev_w = torch.empty((R, m), dtype=torch.int32, device=self.device)
        ev_k = torch.empty((R, m), dtype=torch.int32, device=self.device)
        ev_s = torch.empty((R, m), dtype=torch.float32, device=self.device)
        detect(count, ev_w if m else None, ev_k if m else None, ev_s if m else None, m)
        count, ev_w, ev_k, ev_s = count.cpu().numpy(), ev_w.cpu().numpy(), ev_k.cpu().numpy(), ev_s.cpu().numpy()
        return [[(float(end_times[r][ev_w[r, i]]), int(ev_k[r, i]), self.words[int(ev_k[r, i])], float(ev_s[r, i]))
                 for i in range(min(int(count[r]), m))] for r in range(R)]

    def _scan(self, x: torch.Tensor, what: str, hop_frames, smooth_window, threshold, refractory, first_keyword, max_events,
              sample_rate) -> ScanResult:
        """``scan`` / ``scan_f32`` behind their argument's type check; the sample type of ``x`` picks the entries."""
        self._decision_args(what, hop_frames, smooth_window, refractory, first_keyword, max_events, decide=threshold is not None)
        ctx, logits, labels, start_s, end_s, _ = self._scan_logits(x, what, hop_frames, sample_rate, True)
        events = None
        if threshold is not None:
            events = self._events(lambda *out: ctx.scan_detect_f32(logits, smooth_window, first_keyword, threshold, refractory, *out),
                                  [end_s] * logits.shape[0], max_events)
        return ScanResult(labels.cpu().numpy(), logits.cpu().numpy(), start_s, events)

    def score(self, pcm, truth, thresholds, hop_frames: int = 1, smooth_window: int = 1, refractory: int = 50, first_keyword: int = 2,
              tolerance_s: float = 1.0, sample_rate: Optional[int] = None):
        """How many keywords would ``scan`` find, miss and invent at each of ``thresholds``?  ``pcm`` as ``scan`` takes it;
        ``truth``: per recording a list of ``(word_or_index, t0, t1)`` in seconds (for one recording ``[n]`` the list itself),
        mapped to windows by ``kws.libs.evaluation.truth_windows`` with ``tolerance_s``.  Returns a ``DetectionReport``: per
        threshold and class the hits, false alarms and duplicates of exactly the events ``scan(threshold=t, smooth_window=...,
        refractory=..., first_keyword=...)`` fires, matched in time order against the annotations, and the hits' latency.

        On the device: the scan (``kws_scan_i16``), then ``kws_scan_score_f32`` -- the smoothing once, one walk per recording and
        threshold.  The logits stay on the device; the one read-back is the ``K * C * 4`` counters."""
        return self._score(self._recordings(pcm, "score"), "score", truth, thresholds, hop_frames, smooth_window, refractory,
                           first_keyword, tolerance_s, sample_rate)

    def score_f32(self, signal, truth, thresholds, hop_frames: int = 1, smooth_window: int = 1, refractory: int = 50,
                  first_keyword: int = 2, tolerance_s: float = 1.0, sample_rate: Optional[int] = None):
        """``score`` for float32 samples in [-1, 1] (``scan_f32``): for ``signal = pcm / 32768`` the counts equal ``score(pcm)``'s."""
        return self._score(self._recordings(signal, "score_f32", f32=True), "score_f32", truth, thresholds, hop_frames, smooth_window,
                           refractory, first_keyword, tolerance_s, sample_rate)

    @staticmethod
    def _score_args(what: str, thresholds, hop_frames, smooth_window, refractory, first_keyword) -> np.ndarray:
        """The argument checks ``score`` and ``score_batch`` share (no device needed) -> the thresholds as float32 [K]."""
        th = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
        if not 1 <= len(th) <= 1024:
            raise ModelError(f"{what}: between 1 and 1024 thresholds are needed, got {len(th)}")
        KeywordSpotter._decision_args(what, hop_frames, smooth_window, refractory, first_keyword)
        return th

    @staticmethod
    def _truth_lists(what: str, truth, R: int) -> list:
        """``truth`` -> one list of annotations per recording; a single recording may give its list directly."""
        lists = list(truth) if truth is not None else []
        if R == 1 and (not lists or (len(lists[0]) == 3 and (isinstance(lists[0][0], str) or np.ndim(lists[0][0]) == 0))):
            lists = [lists]
        if len(lists) != R:
            raise ModelError(f"{what}: {len(lists)} annotation lists for {R} recordings")
        return [list(t) for t in lists]

    def _score_report(self, ctx, score_call, th, truths, end_times, tolerance_s, hours, hop_frames, frame_step):
        """Annotations -> the window table, the native call, the one read-back, the report."""
        from kws.libs.evaluation import DetectionReport, truth_windows

        C = self.model.num_classes
        n_truth, undetectable, rows = np.zeros(C, np.int64), np.zeros(C, np.int64), []
        for r, (t, end_s) in enumerate(zip(truths, end_times)):
            table, n, u = truth_windows(t, end_s, tolerance_s, self.words, C, r)
            rows.append(table)
            n_truth += n
            undetectable += u
        counts = torch.empty((len(th), C, 4), dtype=torch.int64, device=self.device)
        score_call(np.concatenate(rows) if rows else None, counts)
        ctx.sync()
        return DetectionReport(counts.cpu().numpy(), n_truth, undetectable, th, hours, int(hop_frames) * frame_step / self.config.sample_rate,
                               self.words)

    def _score(self, x: torch.Tensor, what: str, truth, thresholds, hop_frames, smooth_window, refractory, first_keyword, tolerance_s,
               sample_rate):
        """``score`` / ``score_f32`` behind their argument's type check; the sample type of ``x`` picks the entries."""
        th = self._score_args(what, thresholds, hop_frames, smooth_window, refractory, first_keyword)
        R = int(x.shape[0])
        truths = self._truth_lists(what, truth, R)
        hours = float(R) * float(x.shape[1]) / float(sample_rate or self.config.sample_rate) / 3600.0
        ctx, logits, _, _, end_s, frame_step = self._scan_logits(x, what, hop_frames, sample_rate, False)
        call = lambda table, counts: ctx.scan_score_f32(logits, smooth_window, first_keyword, refractory, th, table, counts)
        return self._score_report(ctx, call, th, truths, [end_s] * R, tolerance_s, hours, hop_frames, frame_step)

    def scan_file(self, path: str, resample: bool = False, decode: str = "pcm16", **kwargs) -> ScanResult:
        """``scan`` over a whole wav file (no trimming or padding to a clip).  The file must be 16-bit mono PCM at the
        configured rate: anything else raises ``AudioProcessingError`` with the reason.  With ``resample=True`` a 16-bit mono
        file at another rate is uploaded at its own rate and resampled on the device (``scan`` with ``sample_rate``); any other
        encoding at another rate is still refused under this default ``decode``, in the words it always had.

        ``decode="any"``: ``read_wav`` decodes the file.  16-bit mono goes down the int16 path unchanged; every other encoding
        (24-bit, 32-bit, float, stereo) is float32 mono and goes down the float path (``scan_f32``), and with ``resample=True`` the
        rate change runs on the device in the file's own sample type."""
        decode_one = self._decode_any if self._decode_mode(decode, "scan_file") else self._decode_file
        x, rate = decode_one(path, resample, "scan_file")
        return (self.scan if x.dtype == np.int16 else self.scan_f32)(x, sample_rate=rate, **kwargs)

    def _recordings(self, pcm, what: str, f32: bool = False) -> torch.Tensor:
        """int16 ``[n]`` or ``[R, n]``, host array or device tensor -> an int16 tensor ``[R, n]`` (the checks of ``scan``);
        ``f32``: the same for float32 samples (the checks of ``scan_f32``)."""
        kind, t_dtype, n_dtype = ("float32 samples", torch.float32, np.float32) if f32 else ("int16 PCM", torch.int16, np.int16)
        if torch.is_tensor(pcm):
            if pcm.dtype != t_dtype:
                raise ModelError(f"{what} expects {kind}, got {pcm.dtype}")
            x = pcm
        else:
            a = np.asarray(pcm)
            if a.dtype != n_dtype:
                raise ModelError(f"{what} expects {kind}, got {a.dtype}")
            x = torch.from_numpy(np.ascontiguousarray(a))
        if x.dim() == 1:
            x = x[None, :]
        if x.dim() != 2 or x.shape[0] < 1:
            raise ModelError(f"{what} expects {'float32' if f32 else 'int16'} [n] or [R, n], got shape {tuple(x.shape)}")
        return x

    @staticmethod
    def _decode_mode(decode: str, what: str) -> bool:
        """The ``decode`` argument of the file methods -> True for ``"any"``, False for ``"pcm16"`` (today's rules)."""
        if decode not in ("pcm16", "any"):
            raise AudioProcessingError(f"{what}: decode must be 'pcm16' or 'any', got {decode!r}")
        return decode == "any"

    def _decode_any(self, path: str, resample: bool, what: str) -> Tuple[np.ndarray, int]:
        """One wav file under ``decode="any"`` -> (int16 [n] for 16-bit mono, else float32 [n] mono; its rate)."""
        x, rate = read_wav(path)
        if int(rate) != self.config.sample_rate and not resample:
            raise AudioProcessingError(f"{path}: sample rate {rate} != {self.config.sample_rate}; pass resample=True to {what} to "
                                       "resample on the device")
        return x, int(rate)

    def _at_configured_rate(self, x: torch.Tensor, sample_rate: Optional[int], what: str) -> torch.Tensor:
        """Recordings at ``sample_rate`` -> the same at the configured rate, resampled on the device to their natural length
        (``kws_resample_i16``, ``kws_resample_f32`` for float32 samples); ``x`` itself when the rate is the configured one."""
        from kws import _native

        cfg = self.config
        if sample_rate is None or int(sample_rate) == cfg.sample_rate:
            return x
        if x.shape[1] < 1:
            raise ModelError(f"{what}: the recording is empty")
        src = x.to(self.device).contiguous()
        y = torch.empty((src.shape[0], _native.host_resample_len(src.shape[1], sample_rate, cfg.sample_rate)), dtype=src.dtype,
                        device=self.device)
        ctx = self.model._context(self.device.index or 0)
        (ctx.resample_f32 if src.dtype == torch.float32 else ctx.resample_i16)(src, sample_rate, cfg.sample_rate, y)
        return y

    def segment(self, pcm, threshold: float, on_window: int = 40, off_window: int = 80, pre_roll: int = 60, max_seconds: float = 10.0,
                normalize: int = 16384, max_utterances: int = 1024, sample_rate: Optional[int] = None,
                keep_unfinished: bool = True) -> List[List[Utterance]]:
        """Which utterances are in this audio, and what was said in each?  The reference's live loop
        (``kws/inference/inference_local.py:114-192``) over recordings: ``pcm`` int16 ``[n]`` or ``[R, n]``, a host array or a
        device tensor, ``sample_rate`` as in ``scan``.  One list of ``Utterance`` per recording, in time order.

        On the device, in this order: the MFCC frames of each recording as one clip (``kws_frames_i16``); the energy endpointer
        walked over them (``kws_segment_f32``) -- a frame is voiced when its log energy exceeds ``threshold``, an utterance opens
        when more than 80 % of the last ``on_window`` frames are voiced and closes when more than 90 % of the last ``off_window``
        are not (400 / 800 ms by default), after ``max_seconds`` (0: never) or with the recording, and starts ``pre_roll`` frames
        (600 ms) before it opened; then ONE device-to-host read of the counts and spans -- the only synchronisation before the
        results, needed because the number of clips sizes what follows; the spans cut, scaled to a peak of ``normalize`` (0: as
        they are) and padded or trimmed to a clip (``kws_cut_i16``); and the model once per clip (``kws_infer_i16``).  With no
        utterance nothing further is launched.  At most ``max_utterances`` per recording are returned;
        ``keep_unfinished=False`` drops those the end of the recording closed."""
        return self._segment(self._recordings(pcm, "segment"), "segment", threshold, on_window, off_window, pre_roll, max_seconds,
                             normalize, max_utterances, sample_rate, keep_unfinished)

    def segment_f32(self, signal, threshold: float, on_window: int = 40, off_window: int = 80, pre_roll: int = 60,
                    max_seconds: float = 10.0, normalize: int = 16384, max_utterances: int = 1024, sample_rate: Optional[int] = None,
                    keep_unfinished: bool = True) -> List[List[Utterance]]:
        """``segment`` for float32 samples in [-1, 1]: ``signal`` float32 ``[n]`` or ``[R, n]``, a host array or a device tensor
        (``kws_frames_f32``, ``kws_cut_f32``, ``kws_infer_f32``).  ``normalize`` stays in int16 units -- 16384 scales a span to a
        peak of 16384 / 32768 = 0.5 in float64 with one rounding to float32 and no truncation -- and ``Utterance.peak`` is a float
        in full-scale units.  With ``normalize=0`` and ``signal = pcm / 32768`` the spans, labels and logits are those of
        ``segment(pcm, normalize=0)``.  Anything that is not float32 raises ``ModelError``."""
        return self._segment(self._recordings(signal, "segment_f32", f32=True), "segment_f32", threshold, on_window, off_window, pre_roll,
                             max_seconds, normalize, max_utterances, sample_rate, keep_unfinished)

    def _segment_args(self, what: str, on_window, off_window, pre_roll, max_seconds, normalize, max_utterances) -> int:
        """The argument checks ``segment`` and ``segment_batch`` share (no device needed) -> ``max_frames``."""
        if not 1 <= int(on_window) <= int(off_window) <= 1024:
            raise ModelError(f"{what}: need 1 <= on_window <= off_window <= 1024")
        if int(pre_roll) < 0 or int(max_utterances) < 0 or not 0 <= int(normalize) <= 32767:
            raise ModelError(f"{what}: need pre_roll >= 0, max_utterances >= 0 and normalize in [0, 32767]")
        max_frames = int(round(float(max_seconds) * self.config.sample_rate / self._frame_geometry()[1]))
        if max_frames == 1 or max_frames < 0:
            raise ModelError(f"{what}: max_seconds must be 0 (no limit) or at least two frames")
        return max_frames

    def _utterances(self, ctx, found: np.ndarray, R: int, m: int, keep_unfinished: bool, source: torch.Tensor, sample_off, normalize
                    ) -> List[List[Utterance]]:
        """The host copy of the endpointer's answer -- the counts [R], then the slots [R, m, 5] -- -> one list of ``Utterance``
        per recording: the compact rows in recording and time order, their spans cut from ``source`` and classified
        (``_classify_spans``; nothing is launched without a row).  ``source`` is ``[R, n]`` with ``sample_off`` None, or the whole
        buffer of a batch as ONE recording ``[1, n_pcm]``, where a span of recording ``r`` lies ``sample_off[r]`` samples on."""
        counts, slots = found[:R], found[R:].reshape(R, m, 5)
        rows = []  # (recording, start, end, open, close, reason)
        for r in range(R):
            for i in range(min(int(counts[r]), m)):
                start, end, opened, closed, reason = (int(v) for v in slots[r, i])
                if reason == 2 and not keep_unfinished:
                    continue
                rows.append((r, start, end, opened, closed, reason))
        out: List[List[Utterance]] = [[] for _ in range(R)]
        if not rows:
            return out
        span = torch.tensor([(r, s, e) if sample_off is None else (0, int(sample_off[r]) + s, int(sample_off[r]) + e)
                             for r, s, e, _, _, _ in rows], dtype=torch.int32).to(self.device)
        f32 = source.dtype == torch.float32
        cut = (lambda clips, peaks: ctx.cut_f32(source, span, clips, int(normalize) / 32768.0, peaks)) if f32 else \
              (lambda clips, peaks: ctx.cut_i16(source, span, clips, int(normalize), peaks))
        cfg = self.config
        for utt in _classify_spans(ctx, self.model, self.device, self.words, self.model.num_classes, cfg.desired_samples, float(cfg.sample_rate),
                                   self._frame_geometry()[1], rows, cut, f32):
            out[utt.recording].append(utt)
        return out

    def _segment(self, x: torch.Tensor, what: str, threshold, on_window, off_window, pre_roll, max_seconds, normalize, max_utterances,
                 sample_rate, keep_unfinished) -> List[List[Utterance]]:
        """``segment`` / ``segment_f32`` behind their argument's type check; the sample type of ``x`` picks the entries."""
        from kws import _native

        max_frames = self._segment_args(what, on_window, off_window, pre_roll, max_seconds, normalize, max_utterances)
        x = self._at_configured_rate(x, sample_rate, what)
        R, n = int(x.shape[0]), int(x.shape[1])
        if n < 1:
            raise ModelError(f"{what}: the recording is empty")
        F, _ = _native.host_scan_shape(n, *self._frame_geometry(), WINDOW_FRAMES, 1)
        ctx = self.model._context(self.device.index or 0)
        x = x.to(self.device).contiguous()
        m = int(max_utterances)
        feat = torch.empty((R, F, self.config.num_cepstral_coeffs), dtype=torch.float32, device=self.device)
        found = torch.empty((R + 5 * R * m,), dtype=torch.int32, device=self.device)  # the counts [R], then the slots [R, m, 5]
        (ctx.frames_f32 if x.dtype == torch.float32 else ctx.frames_i16)(x, feat)
        ctx.segment_f32(feat, n, threshold, found[:R], found[R:] if m else None, m, on_window, off_window, pre_roll, max_frames)
        host = found.cpu().numpy()  # the one device-to-host read (it waits for the stream): counts and spans together
        return self._utterances(ctx, host, R, m, keep_unfinished, x, None, normalize)

    def segment_file(self, path: str, resample: bool = False, decode: str = "pcm16", **kwargs) -> List[Utterance]:
        """``segment`` over a whole wav file; the file's utterances.  The file must be 16-bit mono PCM at the configured rate;
        with ``resample=True`` a 16-bit mono file at another rate is resampled on the device (as ``scan_file``).
        ``decode="any"``: every encoding ``read_wav`` decodes, as ``scan_file`` routes it."""
        decode_one = self._decode_any if self._decode_mode(decode, "segment_file") else self._decode_file
        x, rate = decode_one(path, resample, "segment_file")
        return (self.segment if x.dtype == np.int16 else self.segment_f32)(x, sample_rate=rate, **kwargs)[0]

    # -- batches of recordings of unequal length ---------------------------------------------------------------------------
    def _batch_recordings(self, recordings, sample_rate, what: str, f32: bool = False) -> Tuple[List[torch.Tensor], List[int]]:
        """The argument checks of ``scan_batch`` / ``segment_batch`` (no device needed): a non-empty sequence of int16 ``[n_r]``
        host arrays or tensors, none of them empty, and one rate or one rate per recording -> (1-D int16 tensors, rates).
        ``f32``: float32 ``[n_r]`` members (``scan_batch_f32`` / ``segment_batch_f32``)."""
        if torch.is_tensor(recordings) or isinstance(recordings, np.ndarray):
            recordings = list(recordings) if recordings.ndim == 2 else [recordings]
        recs = list(recordings)
        if not recs:
            raise ModelError(f"{what}: no recordings were given")
        out = []
        for r, rec in enumerate(recs):
            try:
                x = self._recordings(rec, what, f32)
            except ModelError as e:
                raise ModelError(f"{what}: recording {r}: {e.args[0]}") from None
            if x.shape[0] != 1:
                raise ModelError(f"{what}: recording {r} must be one {'float32' if f32 else 'int16'} [n] array, got shape {tuple(x.shape)}")
            if x.shape[1] < 1:
                raise ModelError(f"{what}: recording {r} is empty")
            out.append(x[0])
        cfg = self.config
        if sample_rate is None or np.ndim(sample_rate) == 0:
            rates = [cfg.sample_rate if sample_rate is None else int(sample_rate)] * len(out)
        else:
            rates = [cfg.sample_rate if s is None else int(s) for s in sample_rate]
            if len(rates) != len(out):
                raise ModelError(f"{what}: {len(rates)} sample rates for {len(out)} recordings")
        if any(s < 1 for s in rates):
            raise ModelError(f"{what}: sample rates must be positive")
        return out, rates

    def _pack_batch(self, recs: List[torch.Tensor], rates: List[int]):
        """Recordings -> ONE device buffer of their sample type (int16 or float32) at the configured rate: ``(buffer [n_pcm], start
        int64 [R], length int32 [R])``.
        Recordings at the configured rate are packed one after another, each start rounded up to 8 samples.  The others are
        grouped by rate; a group is padded to its longest, resampled with its true lengths in one launch (``kws_resample_i16`` / ``kws_resample_f32``
        with ``d_len``) straight into a rectangular block of the buffer whose rows are the group's recordings -- the natural
        length of each (``kws_host_resample_len``) is its length."""
        from kws import _native

        cfg = self.config
        R = len(recs)
        up8 = lambda n: (int(n) + 7) & ~7
        length = np.zeros(R, np.int32)
        start = np.zeros(R, np.int64)
        groups: dict = {}
        at = 0
        for r, (x, rate) in enumerate(zip(recs, rates)):
            if rate == cfg.sample_rate:
                length[r], start[r] = x.shape[0], at
                at += up8(x.shape[0])
            else:
                length[r] = _native.host_resample_len(int(x.shape[0]), rate, cfg.sample_rate)
                if length[r] < 1:
                    raise ModelError(f"recording {r} is empty at the configured rate")
                groups.setdefault(rate, []).append(r)
        blocks = []
        for rate, members in groups.items():
            n_out = up8(max(int(length[r]) for r in members))
            for i, r in enumerate(members):
                start[r] = at + i * n_out
            blocks.append((rate, members, at, n_out))
            at += len(members) * n_out
        dtype = recs[0].dtype  # one sample type per batch (_batch_recordings)
        buf = torch.empty((max(at, 8),), dtype=dtype, device=self.device)
        native = [r for r in range(R) if rates[r] == cfg.sample_rate]
        if native and not any(recs[r].is_cuda for r in native):  # host recordings: packed on the host, one upload
            last = native[-1]
            host = np.zeros(int(start[last]) + up8(int(length[last])), np.float32 if dtype == torch.float32 else np.int16)
            for r in native:
                host[int(start[r]):int(start[r]) + int(length[r])] = recs[r].numpy()
            buf[:host.shape[0]].copy_(torch.from_numpy(host))
        else:
            for r in native:
                buf[int(start[r]):int(start[r]) + int(length[r])].copy_(recs[r])
        ctx = self.model._context(self.device.index or 0)
        for rate, members, first, n_out in blocks:
            n_in = max(int(recs[r].shape[0]) for r in members)
            src = torch.zeros((len(members), n_in), dtype=dtype, device=self.device)
            for i, r in enumerate(members):
                src[i, :recs[r].shape[0]].copy_(recs[r])
            lengths = torch.tensor([int(recs[r].shape[0]) for r in members], dtype=torch.int32, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()  # a context may run on its own stream
            (ctx.resample_f32 if dtype == torch.float32 else ctx.resample_i16)(
                src, rate, cfg.sample_rate, buf[first:first + len(members) * n_out].view(len(members), n_out), lengths)
        torch.cuda.current_stream(self.device).synchronize()
        return buf, start, length

    def scan_batch(self, recordings, hop_frames: int = 1, smooth_window: int = 1, threshold: Optional[float] = None, refractory: int = 50,
                   first_keyword: int = 2, max_events: int = 1024, sample_rate=None) -> List[ScanResult]:
        """``scan`` for a batch of recordings of unequal length in one pass: ``recordings`` is a sequence of int16 ``[n_r]`` host
        arrays or device tensors, ``sample_rate`` one rate or one rate per recording (``None``: the configured one).  Element
        ``r`` of the result equals ``scan(recordings[r], ...)`` in every field -- labels ``[1, W_r]``, logits ``[1, W_r, C]``,
        window start times, events -- bit for bit, except that a recording shorter than one window gives a result with zero
        windows instead of raising.  An empty recording raises ``ModelError`` naming its index.

        On the device: the recordings in one buffer (``_pack_batch``), the front end over all of them in one launch and the model
        over the packed frame array as one recording (``kws_scan_ragged_i16``), the decisions per recording
        (``kws_scan_detect_ragged_f32``).  The windows that straddle two recordings are computed and dropped."""
        return self._scan_batch(recordings, "scan_batch", False, hop_frames, smooth_window, threshold, refractory, first_keyword,
                                max_events, sample_rate)

    def scan_batch_f32(self, recordings, hop_frames: int = 1, smooth_window: int = 1, threshold: Optional[float] = None,
                       refractory: int = 50, first_keyword: int = 2, max_events: int = 1024, sample_rate=None) -> List[ScanResult]:
        """``scan_batch`` for a sequence of float32 ``[n_r]`` recordings (``kws_scan_ragged_f32``): element ``r`` equals
        ``scan_f32(recordings[r], ...)``.  A member that is not float32 raises ``ModelError`` naming its index."""
        return self._scan_batch(recordings, "scan_batch_f32", True, hop_frames, smooth_window, threshold, refractory, first_keyword,
                                max_events, sample_rate)

    def _scan_logits_batch(self, recs, rates, hop: int, want_labels: bool):
        """Recordings of a batch -> (ctx, packed logits [W_pack, C] and labels [W_pack] (or None) on the device, windows [R],
        win_off [R], length [R], per recording its window (start, end) times, frame_step): the packing, the plan and the ragged
        scan ``scan_batch`` and ``score_batch`` share."""
        from kws import _native

        frame_len, frame_step = self._frame_geometry()
        buf, start, length = self._pack_batch(recs, rates)
        _, _, windows, win_off, W_pack = _native.host_ragged_plan(length, frame_len, frame_step, WINDOW_FRAMES, hop)
        ctx = self.model._context(self.device.index or 0)
        logits = torch.empty((max(W_pack, 1), self.model.num_classes), dtype=torch.float32, device=self.device)
        labels = torch.empty((max(W_pack, 1),), dtype=torch.int32, device=self.device) if want_labels else None
        self.model._native_scan_ragged(ctx, buf, start, length, hop, logits, labels)
        times = [scan_window_times(int(windows[r]), hop, frame_len, frame_step, self.config.sample_rate, WINDOW_FRAMES, int(length[r]))
                 for r in range(len(recs))]
        return ctx, logits, labels, windows, win_off, times, frame_step

    def _scan_batch(self, recordings, what: str, f32: bool, hop_frames, smooth_window, threshold, refractory, first_keyword, max_events,
                    sample_rate) -> List[ScanResult]:
        recs, rates = self._batch_recordings(recordings, sample_rate, what, f32)
        self._decision_args(what, hop_frames, smooth_window, refractory, first_keyword, max_events, decide=threshold is not None)
        ctx, logits, labels, windows, win_off, times, _ = self._scan_logits_batch(recs, rates, int(hop_frames), True)
        events = None
        if threshold is not None:
            def detect(*out):
                ctx.scan_detect_ragged_f32(logits, win_off, windows, smooth_window, first_keyword, threshold, refractory, *out)
                ctx.sync()
            events = self._events(detect, [end_s for _, end_s in times], max_events)
        ctx.sync()
        labels_h, logits_h = labels.cpu().numpy(), logits.cpu().numpy()
        out = []
        for r, (start_s, _) in enumerate(times):
            W, o = int(windows[r]), int(win_off[r])
            out.append(ScanResult(labels_h[o:o + W][None, :].copy(), logits_h[o:o + W][None, :, :].copy(), start_s,
                                  None if events is None else [events[r]]))
        return out

    def score_batch(self, recordings, truths, thresholds, hop_frames: int = 1, smooth_window: int = 1, refractory: int = 50,
                    first_keyword: int = 2, tolerance_s: float = 1.0, sample_rate=None):
        """``score`` for a batch of recordings of unequal length in one pass (``recordings`` and ``sample_rate`` as ``scan_batch``;
        ``truths``: one annotation list per recording).  The report's counts equal the sum of ``score(recordings[r], truths[r],
        ...)`` over the recordings; a recording shorter than one window has no windows, so its annotations are undetectable
        (``kws_scan_ragged_i16``, ``kws_scan_score_ragged_f32``)."""
        return self._score_batch(recordings, "score_batch", False, truths, thresholds, hop_frames, smooth_window, refractory, first_keyword,
                                 tolerance_s, sample_rate)

    def score_batch_f32(self, recordings, truths, thresholds, hop_frames: int = 1, smooth_window: int = 1, refractory: int = 50,
                        first_keyword: int = 2, tolerance_s: float = 1.0, sample_rate=None):
        """``score_batch`` for a sequence of float32 ``[n_r]`` recordings (``kws_scan_ragged_f32``)."""
        return self._score_batch(recordings, "score_batch_f32", True, truths, thresholds, hop_frames, smooth_window, refractory,
                                 first_keyword, tolerance_s, sample_rate)

    def _score_batch(self, recordings, what: str, f32: bool, truths, thresholds, hop_frames, smooth_window, refractory, first_keyword,
                     tolerance_s, sample_rate):
        recs, rates = self._batch_recordings(recordings, sample_rate, what, f32)
        th = self._score_args(what, thresholds, hop_frames, smooth_window, refractory, first_keyword)
        lists = [list(t) if t is not None else [] for t in (truths if truths is not None else [[]] * len(recs))]
        if len(lists) != len(recs):
            raise ModelError(f"{what}: {len(lists)} annotation lists for {len(recs)} recordings")
        hours = sum(float(x.shape[0]) / float(rate) for x, rate in zip(recs, rates)) / 3600.0
        ctx, logits, _, windows, win_off, times, frame_step = self._scan_logits_batch(recs, rates, int(hop_frames), False)
        call = lambda table, counts: ctx.scan_score_ragged_f32(logits, win_off, windows, smooth_window, first_keyword, refractory, th, table,
                                                               counts)
        return self._score_report(ctx, call, th, lists, [end_s for _, end_s in times], tolerance_s, hours, int(hop_frames), frame_step)

    def segment_batch(self, recordings, threshold: float, on_window: int = 40, off_window: int = 80, pre_roll: int = 60,
                      max_seconds: float = 10.0, normalize: int = 16384, max_utterances: int = 1024, sample_rate=None,
                      keep_unfinished: bool = True) -> List[List[Utterance]]:
        """``segment`` for a batch of recordings of unequal length in one pass (``recordings`` and ``sample_rate`` as
        ``scan_batch``).  Element ``r`` equals ``segment(recordings[r], ...)[0]`` with ``Utterance.recording = r``.

        On the device: the recordings in one buffer, their frames in one launch (``kws_frames_ragged_i16``), the endpointer per
        recording (``kws_segment_ragged_f32``), then the ONE device-to-host read of counts and spans, the cut over the whole
        buffer as one recording with each recording's start added to its spans (``kws_cut_i16``) and the model once per clip."""
        return self._segment_batch(recordings, "segment_batch", False, threshold, on_window, off_window, pre_roll, max_seconds, normalize,
                                   max_utterances, sample_rate, keep_unfinished)

    def segment_batch_f32(self, recordings, threshold: float, on_window: int = 40, off_window: int = 80, pre_roll: int = 60,
                          max_seconds: float = 10.0, normalize: int = 16384, max_utterances: int = 1024, sample_rate=None,
                          keep_unfinished: bool = True) -> List[List[Utterance]]:
        """``segment_batch`` for a sequence of float32 ``[n_r]`` recordings (``kws_frames_ragged_f32``, ``kws_cut_f32`` over the
        buffer as one recording): element ``r`` equals ``segment_f32(recordings[r], ...)[0]`` with ``Utterance.recording = r``."""
        return self._segment_batch(recordings, "segment_batch_f32", True, threshold, on_window, off_window, pre_roll, max_seconds,
                                   normalize, max_utterances, sample_rate, keep_unfinished)

    def _segment_batch(self, recordings, what: str, f32: bool, threshold, on_window, off_window, pre_roll, max_seconds, normalize,
                       max_utterances, sample_rate, keep_unfinished) -> List[List[Utterance]]:
        from kws import _native

        recs, rates = self._batch_recordings(recordings, sample_rate, what, f32)
        max_frames = self._segment_args(what, on_window, off_window, pre_roll, max_seconds, normalize, max_utterances)
        buf, start, length = self._pack_batch(recs, rates)
        R, m = len(recs), int(max_utterances)
        frames, frame_off, _, _, _ = _native.host_ragged_plan(length, *self._frame_geometry(), WINDOW_FRAMES, 1)
        ctx = self.model._context(self.device.index or 0)
        feat = torch.empty((int(frame_off[R]), self.config.num_cepstral_coeffs), dtype=torch.float32, device=self.device)
        found = torch.empty((R + 5 * R * m,), dtype=torch.int32, device=self.device)  # the counts [R], then the slots [R, m, 5]
        (ctx.frames_ragged_f32 if f32 else ctx.frames_ragged_i16)(buf, start, length, 1, feat)
        ctx.segment_ragged_f32(feat, frame_off, frames, length, threshold, found[:R], found[R:] if m else None, m, on_window, off_window,
                               pre_roll, max_frames)
        ctx.sync()
        host = found.cpu().numpy()  # the one device-to-host read: counts and spans together
        return self._utterances(ctx, host, R, m, keep_unfinished, buf[None, :], start, normalize)

    def _decode_file(self, path: str, resample: bool, what: str) -> Tuple[np.ndarray, int]:
        """One wav file under the decode rules and error messages of ``scan_file`` / ``segment_file`` -> (int16 [n], rate)."""
        if resample:
            x, rate = read_wav(path)
            if rate != self.config.sample_rate:
                if x.dtype != np.int16:
                    tail = " (there is no float32 scan)" if what == "scan_file" else ""
                    raise AudioProcessingError(f"{path}: sample rate {rate} != {self.config.sample_rate} and the file is not 16-bit mono "
                                               f"PCM; the device resampler of {what} takes int16 only{tail}")
                return x, int(rate)
        x = load_pcm16(path, self.config.sample_rate)
        if x.ndim == 2:
            raise AudioProcessingError(f"{path}: {x.shape[1]} channels; {what} takes mono files")
        return x, self.config.sample_rate

    def _files_by_type(self, paths: Sequence[str], resample: bool, what: str, run_i16, run_f32) -> list:
        """The plural file methods under ``decode="any"``: the files decoded by ``read_wav``, ONE ragged pass per sample type
        (``run_i16`` / ``run_f32``: recordings, rates -> one result per recording), the results in input order."""
        decoded = [self._decode_any(p, resample, what) for p in paths]
        out: list = [None] * len(decoded)
        for is_i16, run in ((True, run_i16), (False, run_f32)):
            members = [i for i, (x, _) in enumerate(decoded) if (x.dtype == np.int16) == is_i16]
            if members:
                for i, res in zip(members, run([decoded[i][0] for i in members], [decoded[i][1] for i in members])):
                    out[i] = res
        return out

    def scan_files(self, paths: Sequence[str], resample: bool = False, decode: str = "pcm16", **kwargs) -> List[ScanResult]:
        """``scan_batch`` over whole wav files, one result per path: each file is decoded under the rules of ``scan_file`` (16-bit
        mono PCM at the configured rate; with ``resample=True`` also 16-bit mono at another rate).  Files at other rates are
        grouped by rate, resampled on the device with one launch per group, and scanned with the rest in one pass.
        ``decode="any"``: every encoding ``read_wav`` decodes; 16-bit mono files go through ``scan_batch`` and the others, as
        float32, through ``scan_batch_f32`` -- one ragged pass per sample type, results in the order of ``paths``."""
        if self._decode_mode(decode, "scan_files"):
            return self._files_by_type(paths, resample, "scan_files",
                                       lambda recs, rates: self.scan_batch(recs, sample_rate=rates, **kwargs),
                                       lambda recs, rates: self.scan_batch_f32(recs, sample_rate=rates, **kwargs))
        decoded = [self._decode_file(p, resample, "scan_file") for p in paths]
        return self.scan_batch([x for x, _ in decoded], sample_rate=[rate for _, rate in decoded], **kwargs)

    def segment_files(self, paths: Sequence[str], resample: bool = False, decode: str = "pcm16", **kwargs) -> List[List[Utterance]]:
        """``segment_batch`` over whole wav files, one list of utterances per path (decode rules of ``segment_file``;
        ``decode="any"`` as ``scan_files``, ``Utterance.recording`` being the index into ``paths``)."""
        if self._decode_mode(decode, "segment_files"):
            out = self._files_by_type(paths, resample, "segment_files",
                                      lambda recs, rates: self.segment_batch(recs, sample_rate=rates, **kwargs),
                                      lambda recs, rates: self.segment_batch_f32(recs, sample_rate=rates, **kwargs))
            for i, utts in enumerate(out):
                for u in utts:
                    u.recording = i
            return out
        decoded = [self._decode_file(p, resample, "segment_file") for p in paths]
        return self.segment_batch([x for x, _ in decoded], sample_rate=[rate for _, rate in decoded], **kwargs)


_default: Optional[KeywordSpotter] = None


def inference(test_audio, spotter: Optional[KeywordSpotter] = None):
    """Classify one wav file; prints and returns ``(index, word)`` like the reference script prints."""
    global _default
    if spotter is None:
        if _default is None:
            _default = KeywordSpotter()
        spotter = _default
    idx, word = spotter.infer_files([test_audio])[0]
    print(idx, word)
    return idx, word


class StreamingSpotter:
    """Sliding-window spotting over concurrent live streams (10 ms hops).

    The reference's live path captures a VAD-segmented utterance, writes a wav and classifies it once
    (``kws/inference/inference_local.py:114-192``).  Here every ``push`` of ``frame_step`` new samples per
    stream adds one MFCC frame to a 99-frame ring on the GPU and re-classifies the last second of every
    stream (``kws_stream_push_i16``); with ``use_graph`` the two launches of a push replay as one hipGraph.

    ``input_rate``: the rate the audio arrives at, when it is not ``config.sample_rate``.  Every ``push`` then takes ``hop_in``
    samples per stream at that rate (480 at 48 kHz, 441 at 44.1 kHz, 80 at 8 kHz for the default 10 ms hop) and a stateful
    polyphase resampler on the device turns them into the hop (``kws_stream_push_rate_i16`` /
    ``kws_stream_push_host_rate_i16``: the bits of ``kws_resample_i16`` over the whole signal, delayed).  ``hop_in = hop * down /
    up`` must be integral -- 22.05 kHz (220.5) raises ``ModelError``; ``use_graph`` does not apply to these pushes.

    ``utterances``: an ``UtteranceConfig`` arms the reference's live loop on the device (``kws_stream_utt_open``): every push is
    followed by one more launch that appends the hop to a per-stream history, walks one frame of the energy endpointer and
    queues the utterances that closed; ``pop_utterances()`` cuts, normalises and classifies them, ``flush()`` closes what is
    still open.  ``push`` keeps its signature, its results and its zero-copy path; at most 1024 streams.

    ``detect``: a ``DetectConfig`` arms the scan's decision layer on the device (``kws_stream_detect_open``): every push is followed
    by one more launch that takes its logits through softmax, a causal mean, threshold and refractory and queues the keyword
    events; ``pop_events()`` returns them, ``smoothed()`` reads the newest decision's posteriors.  ``push`` keeps its signature,
    its results (raw logits) and its zero-copy path; at most 1024 streams.  May be combined with ``utterances``.

    ``reset(streams)`` hands single slots of the set to new callers while the others run on (``kws_stream_reset``): from the next
    push on a reset stream behaves as if it had heard silence ever since the spotter was created -- its rings, its resampler
    history, its endpointer and its posterior window start over, an utterance open on it closes with ``"end_of_recording"`` --
    and every other stream keeps its bits.  Times and hop numbers of ``Utterance`` and ``KeywordEvent`` stay in set coordinates;
    ``stream_origin`` turns them into a stream's own.  Not with ``smooth_window`` > 0 (one hop count for all streams): use ``detect``.

    ``deactivate(streams)`` / ``activate(streams)`` take slots out of the set and bring them back (``kws_stream_deactivate``,
    ``kws_stream_activate``), ``active`` (``np.bool_[S]``) says which are in, and the ``active=`` argument (bool ``[S]``) sets the
    initial set.  A push launches, reads and writes for the active streams alone: ``push`` keeps its signature and takes full
    ``[S, hop_in]`` arrays, but the rows of inactive streams are NOT READ (with ``input_rate`` the resampler still reads them; what
    they hold does not matter) and their rows of the returned labels and logits are STALE -- whatever the stream's last active push
    left.  An inactive stream yields no utterance and no event.  A stream that is activated starts over as after ``reset``.  A set sized
    for its peak then costs what its active streams cost.  DS-CNN models only, and not with ``use_graph=True``, ``smooth_window`` > 0 or
    ``vad_log_energy``: those raise ``ModelError``.

    Attributes: ``stream_origin`` -- ``np.int64[S]``, the hop count at each stream's last ``reset`` (zeros at creation);
    ``hop`` -- samples per hop at ``config.sample_rate``; ``hop_in`` -- samples ``push`` takes per stream (``hop``
    without ``input_rate``); ``delay_samples`` -- the resampler's delay in samples at ``config.sample_rate`` (10 = 0.625 ms for
    every rate above 16 kHz, 20 for 8 kHz, 0 without ``input_rate``): what the streams hear lags the input by that much.

    ``model``: a ``DepthwiseSeparableConv`` (the default), a ``DepthwiseSeparableConvBN`` (served by its fold) or a
    ``CnnTradFpool3``.  With a ``CnnTradFpool3`` a push is three launches (``kws_stream_push_cnn_trad_i16``: the frame, the
    convolutions over every stream's window of the feature ring read in place, the dense tail), the results are read from the
    device -- one synchronise and one read per push, ``host_results`` is off -- ``use_graph=True`` raises ``ModelError``, and
    ``input_rate`` resamples into the hop buffer (``kws_stream_resample_i16``) in front of the push.  ``utterances``, ``detect``,
    ``smooth_window`` and ``vad_log_energy`` work as for the DS-CNN.
    """

    def __init__(self, n_streams: int, model: Optional[KeywordSpottingModel] = None, words: Sequence[str] = WANTED_WORDS,
                 config: Optional[AudioConfig] = None, device: int = 0, use_graph: bool = False, smooth_window: int = 0,
                 vad_log_energy: Optional[float] = None, vad_windows: Tuple[int, int] = (40, 80), host_results: bool = True,
                 input_rate: Optional[int] = None, utterances: Optional[UtteranceConfig] = None,
                 detect: Optional[DetectConfig] = None, active=None):
        from kws import _native

        self.config = config or AudioConfig()
        self.words = list(words)
        self.model = model if model is not None else DepthwiseSeparableConv(num_classes=len(self.words))
        self.n_streams = int(n_streams)
        self.hop = int(round(self.config.frame_step * self.config.sample_rate))
        self.input_rate = int(input_rate) if input_rate is not None else None
        self._resample = self.input_rate is not None and self.input_rate != self.config.sample_rate
        self.hop_in, self.delay_samples = self.hop, 0
        if self._resample:
            up, down, self.delay_samples, _ = _native.host_stream_resample_plan(self.input_rate, self.config.sample_rate)
            if (self.hop * down) % up:
                raise ModelError(f"input_rate {self.input_rate}: a hop of {self.hop} samples at {self.config.sample_rate} Hz is "
                                 f"{self.hop * down}/{up} = {self.hop * down / up:g} samples at the input rate, not a whole number")
            self.hop_in = self.hop * down // up
        self.device = torch.device("cuda", device)
        self.use_graph = use_graph
        if use_graph and not self.model._stream_graph:
            raise ModelError(f"use_graph=True: {type(self.model).__name__} has no captured-graph push (it is DS-CNN only)")
        self._ctx = _native.Context(device, ModelError)
        cfg = self.config
        frame_len = int(round(cfg.frame_length * cfg.sample_rate))
        if (cfg.sample_rate, cfg.desired_samples, frame_len, self.hop, cfg.fft_size, cfg.num_mel_filters, cfg.num_cepstral_coeffs) != \
                (16000, 16000, 400, 160, 512, 26, 10):  # a non-default AudioConfig: tell the front end (nfft as audio_processor.py:268 derives it)
            self._ctx.set_frontend(cfg.sample_rate, cfg.desired_samples, frame_len, self.hop, max(cfg.fft_size, frame_len),
                                   cfg.num_mel_filters, cfg.num_cepstral_coeffs)
        self.model._native_stream_load(self._ctx)
        self._ctx.stream_open(self.n_streams)
        if self._resample:
            self._ctx.stream_resample_open(self.n_streams, self.input_rate, cfg.sample_rate, self.hop_in)
        self._hop_buf = torch.zeros((self.n_streams, self.hop_in), dtype=torch.int16, device=self.device)
        # a model without the DS-CNN's rate push: the resampler writes the hop here and the model's own push takes it
        self._hop16 = torch.zeros((self.n_streams, self.hop), dtype=torch.int16, device=self.device) \
            if self._resample and not self.model._stream_zero_copy else None
        self._logits = torch.zeros((self.n_streams, self.model.num_classes), dtype=torch.float32, device=self.device)
        self._labels = torch.zeros((self.n_streams,), dtype=torch.int32, device=self.device)
        self._pushes = 0  # hops pushed so far: the origin the next reset records
        self.stream_origin = np.zeros(self.n_streams, dtype=np.int64)
        # posterior smoothing: softmax of every hop's logits averaged over the last
        # `smooth_window` hops per stream on the device (kws_stream_smooth_f32); 0 = raw logits / argmax
        self.smooth_window = int(smooth_window)
        self._smoothed = torch.zeros_like(self._logits) if self.smooth_window > 0 else None
        # energy endpointer (stands in for the reference's webrtcvad gate,
        # kws/inference/inference_local.py:131-166): per stream, bit 0 of `vad_state` = inside an utterance,
        # bits 1-2 = opened (1) / closed (2) at the last hop; None = off
        self.vad_log_energy = vad_log_energy
        self.vad_windows = (int(vad_windows[0]), int(vad_windows[1]))
        self._vad = torch.zeros((self.n_streams,), dtype=torch.int32, device=self.device) if vad_log_energy is not None else None
        self.vad_state: Optional[np.ndarray] = None
        # zero-copy delivery (kws_stream_host_results): the push's own kernel writes logits and labels to pinned host memory
        # and raises a flag there, so a plain push returns without a stream synchronise or a device-to-host copy
        self._host = bool(host_results) and self.smooth_window == 0 and self._vad is None and self.model._stream_zero_copy
        if self._host:
            self._ctx.stream_host_results(True)
        # live utterances (kws_stream_utt_*): armed, every push also appends its hop to a per-stream history on the device, walks
        # one frame of the endpointer and queues the utterances that close; push itself is unchanged, zero-copy path included
        self.utterances = utterances
        self._utt_seq = 0  # the next sequence number pop_utterances hands out
        if utterances is not None:
            u = utterances
            max_frames = int(round(float(u.max_seconds) * cfg.sample_rate / self.hop))
            if max_frames < 2:
                raise ModelError("utterances: max_seconds must be at least two frames (a live history is bounded: there is no 'never')")
            if not 0 <= int(u.normalize) <= 32767:
                raise ModelError("utterances: normalize must be in [0, 32767]")
            self._utt_frame_len = frame_len
            self._utt_max_events = int(u.max_events) if u.max_events is not None else max(self.n_streams, 64)
            history = _native.host_stream_utt_history(frame_len, self.hop, int(u.pre_roll), max_frames, int(u.slack_hops))
            self._ctx.stream_utt_open(u.threshold, u.on_window, u.off_window, u.pre_roll, max_frames, history, self._utt_max_events)
        # live keyword events (kws_stream_detect_*): armed, every push is also followed by one decision per stream on the device
        # (softmax, causal mean, threshold, refractory) and the events are queued; push itself is unchanged, zero-copy path included
        self.detect = detect
        self._det_seq = 0  # the next sequence number pop_events hands out
        if detect is not None:
            d = detect
            if not 1 <= int(d.smooth_window) <= 256:
                raise ModelError("detect: smooth_window must be in [1, 256]")
            if int(d.refractory) < 1 or int(d.first_keyword) < 0:
                raise ModelError("detect: need refractory >= 1 and first_keyword >= 0")
            self._det_lag = -(-frame_len // self.hop)  # K: hops a frame spans; push h completes frame h - K
            self._det_frame_len = frame_len
            self._det_max_events = int(d.max_events) if d.max_events is not None else max(self.n_streams, 64)
            first_hop = WINDOW_FRAMES + self._det_lag - 1 if d.skip_partial_windows else 0
            self._ctx.stream_detect_open(self.model.num_classes, d.smooth_window, d.first_keyword, d.threshold, d.refractory, first_hop,
                                         self._det_max_events)
        # sparse sets (kws_stream_deactivate / kws_stream_activate): which streams the pushes serve; all of them unless told otherwise
        self._active = np.ones(self.n_streams, dtype=np.bool_)
        if active is not None:
            initial = np.asarray(active)
            if initial.shape != (self.n_streams,) or initial.dtype != np.bool_:
                raise ModelError(f"active expects bool [{self.n_streams}]")
            if not initial.all():
                self.deactivate(np.flatnonzero(~initial))
        torch.cuda.synchronize(self.device)

    def load_model(self, model: KeywordSpottingModel) -> None:
        """Swap the classifier while the streams keep running (their PCM and feature rings are untouched); a captured
        hipGraph is re-captured on the next push (``kws_load_dscnn`` retires it: it holds the old weights).  The new model must be
        of the family the spotter was created with (DS-CNN, folded BatchNorm DS-CNN included, or cnn-trad-fpool3)."""
        if model._family != self.model._family:
            raise ModelError(f"load_model: the streams run {type(self.model).__name__}; a {type(model).__name__} is another model "
                             "family -- create a new StreamingSpotter for it")
        if model.num_classes != self.model.num_classes:
            raise ModelError(f"the streams were opened for {self.model.num_classes} classes, the new model has {model.num_classes}")
        self.model = model
        model._native_stream_load(self._ctx)

    def push(self, samples) -> Tuple[np.ndarray, np.ndarray]:
        """``int16[n_streams, hop_in]`` (host array or device tensor) -> (labels int32[S], logits float32[S,C]);
        with ``smooth_window`` > 0 the second array holds the smoothed posteriors and the labels are their argmax."""
        if self._host and not isinstance(samples, torch.Tensor):
            # host samples in, host results out, one call: the kernel reads the hop from pinned host memory and writes the
            # results back there (kws_stream_push_host_i16) -- no H2D copy, no synchronise, no D2H copy
            h = np.ascontiguousarray(samples, dtype=np.int16)
            if h.shape != (self.n_streams, self.hop_in):
                raise ModelError(f"push expects int16 [{self.n_streams}, {self.hop_in}]")
            if self._resample:
                lg, lb = self._ctx.stream_push_host_rate_i16(h, self.n_streams)
            else:
                lg, lb = self._ctx.stream_push_host_i16(h, self.n_streams)
            self._pushes += 1
            return lb.copy(), lg.copy()
        x = samples if isinstance(samples, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int16))
        if tuple(x.shape) != (self.n_streams, self.hop_in) or x.dtype != torch.int16:
            raise ModelError(f"push expects int16 [{self.n_streams}, {self.hop_in}]")
        self._hop_buf.copy_(x, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()  # the context runs on its own stream
        if self._hop16 is not None:
            if self._ctx.stream_resample_i16(self._hop_buf, self._hop16) != self.hop:
                raise ModelError(f"push: the resampler did not emit a hop of {self.hop} samples")
            self.model._native_stream_push(self._ctx, self._hop16, self._logits, self._labels, False)
        elif self._resample:
            self._ctx.stream_push_rate_i16(self._hop_buf, self._logits, self._labels)
        else:
            self.model._native_stream_push(self._ctx, self._hop_buf, self._logits, self._labels, self.use_graph)
        self._pushes += 1
        if self._host:
            lg, lb = self._ctx.stream_wait_host(self.n_streams)
            return lb.copy(), lg.copy()
        if self._vad is not None:
            self._ctx.stream_vad_f32(self.vad_log_energy, self.vad_windows[0], self.vad_windows[1], self._vad)
        if self.smooth_window > 0:
            self._ctx.stream_smooth_f32(self._logits, self.smooth_window, self._smoothed, self._labels)
            self._ctx.sync()
            self._fetch_vad()
            return self._labels.cpu().numpy(), self._smoothed.cpu().numpy()
        self._ctx.sync()
        self._fetch_vad()
        return self._labels.cpu().numpy(), self._logits.cpu().numpy()

    def reset(self, streams) -> int:
        """Start ``streams`` (an index or a sequence of indices; duplicates are fine) over between two pushes, in one call of
        ``kws_stream_reset``: nothing waits for the device and every other stream is untouched.  Returns the number of hops pushed
        so far, the reset's origin, and records it in ``stream_origin`` for the named streams.  The set's clock runs on, so for
        stream ``s`` a ``KeywordEvent.hop`` is hop ``hop - stream_origin[s]`` of the stream's own audio, and an ``Utterance`` or
        ``KeywordEvent`` time ``t`` (seconds) is ``t - stream_origin[s] * hop / config.sample_rate`` seconds after the stream's
        first sample.  An utterance open on a reset stream is returned by the next ``pop_utterances`` with reason
        ``"end_of_recording"``; events already queued stay.  With ``smooth_window`` > 0 the device refuses and this raises
        ``ModelError``."""
        idx = np.atleast_1d(np.asarray(streams))
        if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
            raise ModelError("reset expects a stream index or a sequence of stream indices")
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_streams):
            raise ModelError(f"reset: stream indices must be in [0, {self.n_streams})")
        idx = idx.astype(np.int64)
        if self.smooth_window > 0 and self._pushes == 0:  # the device refuses once the smoother's history is live: the same answer before it
            raise ModelError("kws_stream_reset: kws_stream_smooth_f32 (smooth_window > 0) keeps a running sum and one hop count for all "
                             "streams, which no single stream can leave; smooth with detect=DetectConfig(...) on spotters that reset streams")
        self._ctx.stream_reset(idx)
        self.stream_origin[idx[self._active[idx]]] = self._pushes  # (on an inactive stream the reset is a no-op)
        return self._pushes

    def _sparse_indices(self, streams, what: str) -> np.ndarray:
        """The checks ``activate`` and ``deactivate`` share: the indices, and what the spotter already knows the device refuses."""
        idx = np.atleast_1d(np.asarray(streams))
        if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
            raise ModelError(f"{what} expects a stream index or a sequence of stream indices")
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_streams):
            raise ModelError(f"{what}: stream indices must be in [0, {self.n_streams})")
        if not self.model._stream_zero_copy:
            raise ModelError(f"{what}: a {type(self.model).__name__} push is three launches over every slot of the set "
                             "(kws_stream_push_cnn_trad_i16); only the DS-CNN's one-launch push serves a set with inactive streams")
        if self.use_graph:
            raise ModelError(f"{what}: use_graph=True replays launches captured for every slot of the set; create the spotter without it")
        if self.smooth_window > 0:
            raise ModelError(f"kws_stream_{what}: kws_stream_smooth_f32 (smooth_window > 0) keeps a running sum and one hop count for all "
                             "streams, which no single stream can leave; smooth with detect=DetectConfig(...) on spotters whose streams come and go")
        if self._vad is not None:
            raise ModelError(f"{what}: vad_log_energy steps kws_stream_vad_f32 over every slot of the set; use utterances=UtteranceConfig(...)")
        return idx.astype(np.int64)

    def deactivate(self, streams) -> None:
        """Take ``streams`` (an index or a sequence; duplicates are fine) out of the set between two pushes
        (``kws_stream_deactivate``): an utterance open on one closes with ``"end_of_recording"``, and from the next push on nothing
        is launched, read or written for them -- their rows of ``push``'s input may hold anything and their result rows go stale.
        Naming an inactive stream does nothing.  Nothing waits for the device."""
        idx = self._sparse_indices(streams, "deactivate")
        self._ctx.stream_deactivate(idx)
        self._active[idx] = False

    def activate(self, streams) -> int:
        """(Re)join ``streams`` to the set between two pushes (``kws_stream_activate``): each gets the whole of ``reset`` -- it
        starts as a stream that has heard silence ever since the spotter was created -- and is served from the next push on.  On
        an active stream this is ``reset``.  Returns the number of hops pushed so far and records it in ``stream_origin``."""
        idx = self._sparse_indices(streams, "activate")
        self._ctx.stream_activate(idx)
        self._active[idx] = True
        self.stream_origin[idx] = self._pushes
        return self._pushes

    @property
    def active(self) -> np.ndarray:
        """``np.bool_[S]``: which streams the pushes serve (the device library's own record, ``kws_stream_active``)."""
        return self._ctx.stream_active(self.n_streams)[0]

    def _fetch_vad(self):
        if self._vad is not None:
            self.vad_state = self._vad.cpu().numpy()

    def features(self) -> np.ndarray:
        """The current windows, oldest frame first: float32 [S, 99, 10] (zeros where no frame exists yet)."""
        _, hops = self._ctx.stream_state()
        t, f = 99, 10
        tmp = torch.empty((self.n_streams, t, f), dtype=torch.float32, device=self.device)
        self._ctx.stream_copy_features(tmp)
        self._ctx.sync()
        host = tmp.cpu().numpy()
        frame_len = int(round(self.config.frame_length * self.config.sample_rate))
        k = -(-frame_len // self.hop)       # hops a frame spans (3 for 400 / 160): the newest frame is hops - k
        head = (hops - k + 1) % t
        return np.roll(host, -head, axis=1), hops

    def _drain(self, which: str, poll, read):
        """What a host-mirrored event queue (``"_utt"`` or ``"_det"``) holds beyond this spotter's sequence counter: ``(first,
        records)``, the counter advanced past them, or ``None`` with nothing new.  Records already overwritten are skipped."""
        total = poll()[0]
        first = max(getattr(self, which + "_seq"), total - getattr(self, which + "_max_events"))
        if total <= first:
            return None
        rec = read(first, total - first)
        setattr(self, which + "_seq", total)
        return first, rec

    def pop_utterances(self) -> List[Utterance]:
        """The utterances that closed since the last call, in the order they closed (ascending stream within a hop).  Waits for
        the newest push's step (``kws_stream_utt_poll``); with nothing new it returns ``[]`` and launches nothing.  Otherwise, on
        the device: the spans cut out of the history rings, normalised and padded or trimmed to a clip
        (``kws_stream_utt_cut_i16``), the model once per clip (``kws_infer_i16`` or the model's own fused entry), then ONE read of logits, labels and peaks.
        ``recording`` is the stream index; times are seconds of the stream since this spotter was armed, at ``config.sample_rate``
        (with ``input_rate`` that is the resampled timeline, ``delay_samples`` behind the input).  Records the queue has already
        overwritten (more than ``max_events`` closes between two calls) are skipped; an utterance cut more than ``slack_hops``
        hops after it closed has left the history and comes back with ``peak`` -1 and a silent clip's logits."""
        if self.utterances is None:
            raise ModelError("pop_utterances: this StreamingSpotter was created without utterances=UtteranceConfig(...)")
        if (new := self._drain("_utt", self._ctx.stream_utt_poll, self._ctx.stream_utt_read)) is None:
            return []
        first, rec = new
        return _classify_spans(self._ctx, self.model, self.device, self.words, self.model.num_classes, self.config.desired_samples,
                               float(self.config.sample_rate), self.hop, rec,
                               lambda clips, peaks: self._ctx.stream_utt_cut_i16(first, clips, int(self.utterances.normalize), peaks))

    def flush(self) -> List[Utterance]:
        """Close every utterance that is still open, at the newest frame and with reason ``"end_of_recording"``
        (``kws_stream_utt_flush``), then what ``pop_utterances`` does.  The streams go on afterwards."""
        if self.utterances is None:
            raise ModelError("flush: this StreamingSpotter was created without utterances=UtteranceConfig(...)")
        self._ctx.stream_utt_flush()
        return self.pop_utterances()

    def pop_events(self) -> List[KeywordEvent]:
        """The keyword events since the last call, in the order they fired (ascending stream within a hop).  Waits for the newest
        push's decision step (``kws_stream_detect_poll``); with nothing new it returns ``[]`` without a launch or a read.
        Otherwise one ``kws_stream_detect_read`` out of the queue's host mirror: no launch, no synchronise, no device copy.
        Records the queue has already overwritten (more than ``max_events`` events between two calls) are skipped."""
        if self.detect is None:
            raise ModelError("pop_events: this StreamingSpotter was created without detect=DetectConfig(...)")
        if (new := self._drain("_det", self._ctx.stream_detect_poll, self._ctx.stream_detect_read)) is None:
            return []
        rec = new[1]
        score = (rec[:, 4] & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
        rate = float(self.config.sample_rate)
        return [KeywordEvent(int(s), ((int(h) - self._det_lag) * self.hop + self._det_frame_len) / rate, int(k), self.words[int(k)],
                             float(score[i]), int(d), int(h)) for i, (s, d, h, k, _) in enumerate(rec)]

    def smoothed(self) -> Tuple[np.ndarray, np.ndarray]:
        """(labels int32 [S], posteriors float32 [S, C]) of the newest decision: the smoothed posteriors the events are decided
        on and their argmax (zeros before the first decision).  A synchronising read, for inspection."""
        if self.detect is None:
            raise ModelError("smoothed: this StreamingSpotter was created without detect=DetectConfig(...)")
        post = torch.empty((self.n_streams, self.model.num_classes), dtype=torch.float32, device=self.device)
        labels = torch.empty((self.n_streams,), dtype=torch.int32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()  # the context runs on its own stream
        self._ctx.stream_detect_smoothed(post, labels)
        self._ctx.sync()
        return labels.cpu().numpy(), post.cpu().numpy()

    def close(self):
        if self.detect is not None:
            self._ctx.stream_detect_close()
        if self.utterances is not None:
            self._ctx.stream_utt_close()
        self._ctx.stream_close()
        self._ctx.close()
