"""Keyword-spotting models whose forward runs in the fused gfx950 kernel.

Drop-in for the reference's ``kws/libs/models.py``: ``KeywordSpottingModel`` (``forward`` / ``save`` /
``load``, ``:13-72``), ``DepthwiseSeparableConvBlock`` (``:75-119``) and
``DepthwiseSeparableConv(num_classes=12, input_channels=1)`` (``:122-183``) with identical parameter
names, shapes and initialisation, so reference checkpoints (bare ``state_dict`` or the trainer's
``{"model_state_dict": ...}``) load unchanged.  The modules only *hold* parameters; the arithmetic of
``forward`` is ``kws_forward_f32`` (include/kws_hip.h): LDS-resident activations, depthwise 3x3 on the
VALU, pointwise 1x1 and conv1 on the matrix cores.  ``DepthwiseSeparableConv`` also trains: after ``model.train()`` (which
the reference trainers call every epoch), with grad mode on and a parameter that requires grad, its forward is a
``torch.autograd.Function`` (``_NativeTrainFunction``) whose backward is ``kws_dscnn_backward_f32``, so the trainer's ``loss.backward()`` /
``optimizer.step()`` work unchanged.  ``CnnTradFpool3`` trains the same way (``kws_cnn_trad_backward_f32``), and so does
``DepthwiseSeparableConvBN`` with batch statistics (``kws_dscnn_bn_train_forward_f32`` / ``kws_dscnn_bn_backward_f32``).
"""
from __future__ import annotations

import abc
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from kws.common.errors import ModelError

FEATURE_SHAPE = (1, 99, 10)  # [C, T, F] the fused kernel is built for (reference defaults)


class KeywordSpottingModel(nn.Module, abc.ABC):
    """Interface every KWS model implements."""

    def __init__(self, num_classes: int, **kwargs):
        super().__init__()
        self.num_classes = num_classes

    @abc.abstractmethod
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """``x [B,1,T,F]`` -> logits ``[B,num_classes]``."""

    def save(self, path: str) -> None:
        try:
            torch.save(self.state_dict(), path)
        except Exception as e:
            raise ModelError(f"Failed to save model to {path}: {str(e)}") from e

    def load(self, path: str, device: Optional[torch.device] = None) -> None:
        try:
            if device is None:
                device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
            state = torch.load(path, map_location=device, weights_only=True)
            if isinstance(state, dict) and "model_state_dict" in state:  # trainer checkpoints (training.py:199-216)
                state = state["model_state_dict"]
            self.load_state_dict(state)
            self.to(device)
        except Exception as e:
            raise ModelError(f"Failed to load model from {path}: {str(e)}") from e


class DepthwiseSeparableConvBlock(nn.Module):
    """One block: kxk depthwise + 1x1 pointwise + ReLU (the pointwise keeps the reference's ``padding=padding`` --
    the relu(bias) ring, ``models.py:104-106``).  Inside ``DepthwiseSeparableConv`` the four blocks run fused in the
    DS-CNN kernel and this module only holds their parameters; called on its own, ``forward`` is the general-shape
    operator ``kws_dsblock_forward_f32`` (any ``[B, C_in, H, W]``, kernel size, stride and padding).  Called on its own it is
    inference only: the output has no ``grad_fn`` (the block's gradients exist only through ``DepthwiseSeparableConv``)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, stride: int = 1, padding: int = 1):
        super().__init__()
        self.depthwise = nn.Conv2d(in_channels, in_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                                   groups=in_channels)
        self.pointwise = nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=padding)
        self.kernel_size, self.stride, self.padding = int(kernel_size), int(stride), int(padding)
        self._ctx = None
        self._dev_params = None  # (fingerprint, tensors on the device)

    def sync_weights(self) -> None:
        """Force a re-upload at the next forward (needed only after edits through ``p.data``)."""
        self._dev_params = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """``float32[B, C_in, H, W]`` on the GPU -> ``float32[B, C_out, Ho + 2p, Wo + 2p]`` (``models.py:108-119``)."""
        from kws import _native

        if not x.is_cuda:
            raise ModelError("DepthwiseSeparableConvBlock.forward needs a CUDA/ROCm tensor: the forward is a HIP kernel "
                             "and has no CPU fallback")
        c_in = self.depthwise.in_channels
        if x.dim() != 4 or x.shape[1] != c_in:
            raise ModelError(f"expected input [B,{c_in},H,W], got {tuple(x.shape)}")
        dev = x.device.index or 0
        if self._ctx is None or self._ctx.device != dev:
            self._ctx = _native.Context(dev, ModelError)
            self._dev_params = None
        params = (self.depthwise.weight, self.depthwise.bias, self.pointwise.weight, self.pointwise.bias)
        fp = tuple((p.data_ptr(), p._version) for p in params)
        if self._dev_params is None or self._dev_params[0] != fp:
            self._dev_params = (fp, tuple(p.detach().to(x.device, torch.float32).contiguous() for p in params))
        dw_w, dw_b, pw_w, pw_b = self._dev_params[1]
        k, s, p = self.kernel_size, self.stride, self.padding
        B, _, H, W = x.shape
        if H + 2 * p < k or W + 2 * p < k:
            raise ModelError(f"kernel size {k} exceeds the padded input {H + 2 * p} x {W + 2 * p}")
        ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self._ctx.use_torch_stream()
        x = x.detach().to(torch.float32).contiguous()
        out = torch.empty((B, self.pointwise.out_channels, ho + 2 * p, wo + 2 * p), dtype=torch.float32, device=x.device)
        self._ctx.dsblock_forward_f32(x, dw_w, dw_b, pw_w, pw_b, k, s, p, out)
        return out


def split_flat_grad(grad: torch.Tensor, params):
    """The flat gradient of a backward entry (``state_dict`` order) as one piece per parameter: shaped like the parameter, on its
    device and of its dtype.  ``grad`` is copied once per device."""
    on_dev = {}
    out, off = [], 0
    for p in params:
        if p.device not in on_dev:
            on_dev[p.device] = grad.to(p.device)
        out.append(on_dev[p.device][off:off + p.numel()].view(p.shape).to(p.dtype))
        off += p.numel()
    return out


class _NativeTrainFunction(torch.autograd.Function):
    """The forward of a ``_TrainableNative`` model with a HIP backward.  Forward: exactly the inference call; the input and
    the parameters are saved with ``save_for_backward``, so torch's version counter rejects a parameter modified in place between
    forward and backward.  Backward: the model's backward entry at the saved parameters -- the weights the forward saw, also when a
    module attribute was replaced by a new ``nn.Parameter`` in between (a new one bumps no version of the saved one; uploaded only
    if they are not the device copy, so no re-upload in a normal step), the flat gradient split by ``split_flat_grad``."""

    @staticmethod
    def forward(fctx, model, x, *params):
        logits, labels = model._forward_native(x)
        fctx.model = model
        fctx.save_for_backward(x, *params)
        fctx.mark_non_differentiable(labels)
        return logits, labels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, dlogits, _dlabels):
        x, *params = fctx.saved_tensors
        model = fctx.model
        if fctx.needs_input_grad[1]:
            raise ModelError(f"{model._name}: the gradient with respect to the input features is not provided "
                             f"({model._backward_entry} computes parameter gradients only); detach the input")
        ctx = model._train_context(x.device.index or 0, params)
        x = x.detach().to(torch.float32).contiguous()
        dl = dlogits.detach().to(x.device, torch.float32).contiguous()
        grad = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=x.device)
        model._native_backward(ctx, x, dl, grad)
        return (None, None, *split_flat_grad(grad, params))


class _TrainableNative(KeywordSpottingModel):
    """A model whose forward and backward are HIP entries of a ``_native.Context``: the context with its parameter refresh, the
    switch between the plain forward and ``_NativeTrainFunction``, the output tensors and the checks of ``infer_pcm16``.  A model
    supplies ``_name``, ``_backward_entry``, ``_pcm16_is`` and the hooks ``_check_features``, ``_load_host``, ``_load_device``,
    ``_native_forward``, ``_native_backward``, and what ``KeywordSpotter`` / ``StreamingSpotter`` run a model through:
    ``_native_infer_i16``, ``_native_infer_f32``, ``_native_scan``, ``_native_scan_ragged``, ``_native_stream_load``,
    ``_native_stream_push``."""

    _name = ""            # the class name in messages
    _backward_entry = ""  # the C entry behind loss.backward()
    _pcm16_is = "the forward is a HIP kernel"  # what infer_pcm16 tells a CPU tensor it is
    # the parameter refresh of ``_context`` for parameters on the GPU: True = on the device (``kws_load_*_device``), False =
    # through the host as for CPU-resident parameters (an instance of ``DepthwiseSeparableConv`` sets it to compare the routes)
    _device_refresh = True
    # what the spotters may use with this model: ``_family`` names the kernels (a StreamingSpotter swaps models within one
    # family only); the host-ingest pipeline, the captured-graph push and the zero-copy result delivery exist for the DS-CNN
    _family = ""
    _host_ingest = False
    _stream_graph = False
    _stream_zero_copy = False

    def __init__(self, num_classes: int):
        super().__init__(num_classes)
        self._ctx = None
        self._uploaded = None  # fingerprint of the parameters currently on the device
        self._autograd = False  # set by an explicit train(), cleared by eval() / train(False)

    def train(self, mode: bool = True):
        """``nn.Module.train``; an explicit ``train()`` also switches ``forward`` to the autograd path (see the class
        docstring), ``eval()`` / ``train(False)`` switches it back."""
        super().train(mode)
        self._autograd = bool(mode)
        return self

    def packed_weights(self) -> np.ndarray:
        """The ``state_dict`` tensors, in order, as one float32 vector (the layout of the model's host load): concatenated on
        the parameters' device and copied to the host once.  (The refresh after an optimizer step uses it only on the host route:
        parameters on the GPU are re-loaded there, see ``_context``.)"""
        return self._pack(self.state_dict().values())

    @staticmethod
    def _pack(tensors) -> np.ndarray:
        vals = [v.detach() for v in tensors]
        dev = vals[0].device
        flat = torch.cat([v.to(dev, torch.float32).reshape(-1) for v in vals])
        return flat.cpu().numpy()

    def sync_weights(self) -> None:
        """Force a re-upload of the parameters at the next forward.  The device copy is refreshed automatically when
        a parameter is replaced or modified through autograd-visible in-place operations (``p.copy_``, ``p.add_``,
        ``load_state_dict``: they bump ``p._version``); edits made behind torch's back through ``p.data`` (e.g.
        ``p.data.clamp_()``) do not, and need this call."""
        self._uploaded = None

    def _context(self, device_index: int, params=None):
        """The model's context on ``device_index`` holding ``params`` (default: the current parameters, in ``parameters()``
        order); uploaded only when they differ from the tensors (and versions) uploaded last.  Parameters that all live on
        that GPU are concatenated there and loaded by the model's device load (``_device_refresh``); otherwise through the
        host."""
        from kws import _native

        if self._ctx is None or self._ctx.device != device_index:
            self._ctx = _native.Context(device_index, ModelError)
            self._uploaded = None
        params = tuple(self.parameters()) if params is None else tuple(params)
        fp = tuple((p.data_ptr(), p._version) for p in params)
        if fp != self._uploaded:
            dev = torch.device("cuda", device_index)
            if self._device_refresh and all(p.device == dev for p in params):
                self._ctx.use_torch_stream()
                self._load_device(self._ctx, torch.cat([p.detach().to(torch.float32).reshape(-1) for p in params]))
            else:
                self._load_host(self._ctx, self._pack(params))
            self._uploaded = fp
        self._ctx.use_torch_stream()
        return self._ctx

    def _train_context(self, device_index: int, params):
        """What ``_NativeTrainFunction.backward`` hands to ``_native_backward``: the context holding the saved ``params``."""
        return self._context(device_index, params)

    def _outputs(self, like: torch.Tensor):
        return (torch.empty((like.shape[0], self.num_classes), dtype=torch.float32, device=like.device),
                torch.empty((like.shape[0],), dtype=torch.int32, device=like.device))

    def forward(self, x: torch.Tensor, return_labels: bool = False):
        """``float32[B,C,T,F]`` on the GPU -> logits ``float32[B,num_classes]`` (and argmax labels).  After ``train()``, under
        grad mode with trainable parameters, the logits carry a ``grad_fn`` (see the class docstring)."""
        if not x.is_cuda:
            raise ModelError(f"{self._name}.forward needs a CUDA/ROCm tensor: the forward is a HIP kernel and has no CPU fallback")
        self._check_features(x)
        params = tuple(self.parameters())
        if self._autograd and torch.is_grad_enabled() and any(p.requires_grad for p in params):
            logits, labels = _NativeTrainFunction.apply(self, x, *params)
        else:
            logits, labels = self._forward_native(x)
        return (logits, labels) if return_labels else logits

    def _forward_native(self, x: torch.Tensor):
        """The forward kernels on ``x`` (checked by the caller) -> (logits, labels); no autograd graph."""
        ctx = self._context(x.device.index or 0)
        x = x.detach().to(torch.float32).contiguous()
        logits, labels = self._outputs(x)
        self._native_forward(ctx, x, logits, labels)
        return logits, labels

    def _check_pcm16(self):
        pass

    def infer_pcm16(self, wav: torch.Tensor):
        """Fused path: ``int16[B,16000]`` PCM on the GPU -> (logits, labels); MFCC + the model back to back on one stream,
        features never leave the device (``kws_infer_i16`` / ``kws_infer_cnn_trad_i16``)."""
        if not wav.is_cuda:
            raise ModelError(f"{self._name}.infer_pcm16 needs a CUDA/ROCm tensor: {self._pcm16_is} and has no CPU fallback")
        self._check_pcm16()
        if wav.dtype != torch.int16 or wav.dim() != 2:
            raise ModelError("infer_pcm16 expects an int16 tensor [B, n_samples]")
        ctx = self._context(wav.device.index or 0)
        wav = wav.contiguous()
        logits, labels = self._outputs(wav)
        self._native_infer_i16(ctx, wav, logits, labels)
        return logits, labels


class DepthwiseSeparableConv(_TrainableNative):
    """DS-CNN: conv1 (1->64, 10x10, s2, p2) + 4 depthwise-separable blocks + global pool + Linear.  ``forward`` takes any
    ``T x F`` the reference's accepts (``models.py:160-183``: the pooling is adaptive): 99 x 10 runs the fused LDS-resident
    kernel, any other map the composed path (``kws_forward_map_f32``).

    Trainable: after an explicit ``model.train()`` (the reference trainers call it at the start of every epoch,
    ``kws/libs/training.py:275``, ``train.py:32``), when ``torch.is_grad_enabled()`` and some parameter requires grad,
    ``forward`` runs through ``_NativeTrainFunction`` -- the same forward kernels (logits and labels are bit-identical to a call under
    ``torch.no_grad()``) with a backward that recomputes the activations and computes all 20 parameter gradients in HIP
    (``kws_dscnn_backward_f32``, fp32, deterministic).  Each gradient lands on its parameter's device.  No gradient with
    respect to the input features is provided (an input that requires grad raises ``ModelError`` in backward), and
    ``input_channels > 1`` cannot be trained (backward raises ``ModelError``).  Otherwise -- a model never switched with
    ``train()``, or switched back with ``eval()``, ``torch.no_grad()``, frozen parameters -- no autograd graph is built and
    the logits are plain tensors, as for inference."""

    _name = "DepthwiseSeparableConv"
    _backward_entry = "kws_dscnn_backward_f32"
    _family = "dscnn"
    _host_ingest = True
    _stream_graph = True
    _stream_zero_copy = True

    def __init__(self, num_classes: int = 12, input_channels: int = 1):
        super().__init__(num_classes)
        if not 1 <= input_channels <= 64:
            raise ModelError("input_channels must be in [1, 64]")
        self.input_channels = int(input_channels)
        self.conv1 = nn.Conv2d(input_channels, 64, kernel_size=10, stride=2, padding=2)
        self.dsconv1 = DepthwiseSeparableConvBlock(64, 64)
        self.dsconv2 = DepthwiseSeparableConvBlock(64, 64)
        self.dsconv3 = DepthwiseSeparableConvBlock(64, 64)
        self.dsconv4 = DepthwiseSeparableConvBlock(64, 64)
        self.fc = nn.Linear(64, num_classes)
        self._initialize_weights()

    def _initialize_weights(self):
        # same scheme as the reference (:149-158)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)

    # ------------------------------------------------------------------ the hooks of _TrainableNative
    def _load_host(self, ctx, blob):
        ctx.load_dscnn(blob, self.num_classes, self.input_channels)

    def _load_device(self, ctx, blob):
        ctx.load_dscnn_device(blob, self.num_classes, self.input_channels)

    def _check_features(self, x):
        if x.dim() != 4 or x.shape[1] != self.input_channels:
            raise ModelError(f"expected input [B,{self.input_channels},T,F], got {tuple(x.shape)}")

    def _native_forward(self, ctx, x, logits, labels):
        if tuple(x.shape[2:]) == FEATURE_SHAPE[1:]:
            ctx.forward_f32(x, logits, labels)
        else:
            ctx.forward_map_f32(x, logits, labels)

    def _native_backward(self, ctx, x, dl, grad):
        ctx.dscnn_backward_f32(x, x.shape[2], x.shape[3], dl, grad)

    def _check_pcm16(self):
        if self.input_channels != 1:
            raise ModelError("infer_pcm16 needs input_channels=1: the MFCC front end yields one channel")

    def _native_infer_i16(self, ctx, wav, logits, labels):
        ctx.infer_i16(wav, logits, labels)

    def _native_infer_f32(self, ctx, wav, logits, labels):
        ctx.infer_f32(wav, logits, labels)

    def _native_scan(self, ctx, x, hop, logits, labels):
        (ctx.scan_f32 if x.dtype == torch.float32 else ctx.scan_i16)(x, hop, logits, labels)

    def _native_scan_ragged(self, ctx, buf, start, length, hop, logits, labels):
        (ctx.scan_ragged_f32 if buf.dtype == torch.float32 else ctx.scan_ragged_i16)(buf, start, length, hop, logits, labels)

    def _native_stream_load(self, ctx):
        ctx.load_dscnn(self.packed_weights(), self.num_classes)

    def _native_stream_push(self, ctx, hop, logits, labels, use_graph=False):
        ctx.stream_push_i16(hop, logits, labels, use_graph=use_graph)


class DepthwiseSeparableConvBN(KeywordSpottingModel):
    """Build-defined model-zoo member (the reference has no BatchNorm): the same DS-CNN
    with a BatchNorm2d after conv1, after every depthwise and after every pointwise convolution
    (conv -> BN -> ReLU where the plain model has conv -> ReLU; conv -> BN after a depthwise convolution).

    Inference -- a model never switched with ``train()``, or switched back with ``eval()`` / ``train(False)`` -- runs on the
    fold: ``fold()`` folds every BatchNorm, at its running statistics, into the convolution before it -- w' = w * g /
    sqrt(var + eps), b' = (b - mean) * g / sqrt(var + eps) + beta -- which yields an ordinary ``DepthwiseSeparableConv`` whose
    forward is the fused kernel.  The relu(bias) ring of the padded 1x1 convolutions stays exact: a BatchNorm acts per channel,
    ring included.  The fold is detached; ``KeywordSpotter`` / ``StreamingSpotter`` take the model through it.

    Training: after an explicit ``model.train()`` (as for ``_TrainableNative``: ``nn.Module.training`` alone, True by default,
    switches nothing), ``forward`` on a GPU tensor ``[B,1,T,F]`` is the train-mode forward in HIP
    (``kws_dscnn_bn_train_forward_f32``): every BatchNorm normalises with the statistics of the batch, with or without grad mode,
    as torch's does, and the ring of a pointwise convolution (equal to its bias) counts in them.  Each such forward updates the
    nine modules' ``running_mean`` / ``running_var`` (the unbiased batch variance, momentum as ``nn.BatchNorm2d``) and
    ``num_batches_tracked`` on the device without a host synchronisation; the in-place updates bump the buffers' versions, so the
    next ``eval()`` forward rebuilds the fold.  Under grad mode with a parameter that requires grad the forward runs through
    ``_NativeTrainFunction``, whose backward (``kws_dscnn_bn_backward_f32``: recompute, fp32 with float64 batch sums,
    deterministic) yields all 38 parameter gradients; a frozen parameter simply receives none.  No gradient with respect to the
    input (``ModelError`` in backward).  The batch is not chunked: ``B`` above ``_native.host_dscnn_bn_max_batch(T, F)`` (4747
    at 99 x 10) and ``B * H1 * W1 < 2`` raise ``ModelError``, as do ``momentum=None`` and ``track_running_stats=False``."""

    _name = "DepthwiseSeparableConvBN"
    _backward_entry = "kws_dscnn_bn_backward_f32"

    def __init__(self, num_classes: int = 12, eps: float = 1e-5):
        super().__init__(num_classes)
        self.plain = DepthwiseSeparableConv(num_classes)
        self.bn_conv1 = nn.BatchNorm2d(64, eps=eps)
        self.bn_dw = nn.ModuleList([nn.BatchNorm2d(64, eps=eps) for _ in range(4)])
        self.bn_pw = nn.ModuleList([nn.BatchNorm2d(64, eps=eps) for _ in range(4)])
        object.__setattr__(self, "_folded", None)  # kept out of nn.Module's child registry: not a parameter holder
        self._folded_key = None
        self._autograd = False  # set by an explicit train(), cleared by eval() / train(False)
        self._train_ctx = None  # the context of the training entries (the fold has its own)

    @staticmethod
    def _fold(conv: nn.Conv2d, bn: nn.BatchNorm2d):
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()
        w = conv.weight.detach() * scale.reshape(-1, 1, 1, 1)
        b = (conv.bias.detach() - bn.running_mean) * scale + bn.bias.detach()
        return w, b

    def fold(self) -> DepthwiseSeparableConv:
        """The equivalent plain model (cached until a parameter or running statistic changes)."""
        key = tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        if self._folded is not None and key == self._folded_key:
            return self._folded
        out = DepthwiseSeparableConv(self.num_classes)
        with torch.no_grad():
            w, b = self._fold(self.plain.conv1, self.bn_conv1)
            out.conv1.weight.copy_(w)
            out.conv1.bias.copy_(b)
            for i in range(4):
                src = getattr(self.plain, f"dsconv{i + 1}")
                dst = getattr(out, f"dsconv{i + 1}")
                w, b = self._fold(src.depthwise, self.bn_dw[i])
                dst.depthwise.weight.copy_(w)
                dst.depthwise.bias.copy_(b)
                w, b = self._fold(src.pointwise, self.bn_pw[i])
                dst.pointwise.weight.copy_(w)
                dst.pointwise.bias.copy_(b)
            out.fc.weight.copy_(self.plain.fc.weight)
            out.fc.bias.copy_(self.plain.fc.bias)
        object.__setattr__(self, "_folded", out)
        self._folded_key = key
        return out

    def sync_weights(self) -> None:
        """Drop the cached fold (needed only after edits through ``.data``, which do not bump ``_version``)."""
        self._folded_key = None

    def train(self, mode: bool = True):
        """``nn.Module.train``; an explicit ``train()`` also switches ``forward`` from the fold to the train-mode HIP forward (see
        the class docstring), ``eval()`` / ``train(False)`` switches it back."""
        super().train(mode)
        self._autograd = bool(mode)
        return self

    def bn_layers(self):
        """The nine BatchNorm modules in data-flow order (the layer order of ``kws_dscnn_bn_train_forward_f32``'s statistics):
        conv1, then depthwise and pointwise of block 1 .. 4."""
        return [self.bn_conv1] + [m for i in range(4) for m in (self.bn_dw[i], self.bn_pw[i])]

    def forward(self, x: torch.Tensor, return_labels: bool = False):
        if not self._autograd:
            return self.fold().forward(x, return_labels)
        if not x.is_cuda:
            raise ModelError(f"{self._name}.forward needs a CUDA/ROCm tensor: the train-mode forward is HIP kernels and has no CPU "
                             "fallback")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ModelError(f"expected input [B,1,T,F], got {tuple(x.shape)}")
        params = tuple(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            logits, labels = _NativeTrainFunction.apply(self, x, *params)
        else:
            logits, labels = self._forward_native(x)
        return (logits, labels) if return_labels else logits

    def _eps(self) -> float:
        layers = self.bn_layers()
        if any(m.eps != layers[0].eps for m in layers):
            raise ModelError(f"{self._name}: the nine BatchNorm modules must share one eps")
        for m in layers:
            if m.momentum is None or not m.track_running_stats or m.running_mean is None:
                raise ModelError(f"{self._name}: training needs running statistics with a fixed momentum "
                                 "(momentum=None and track_running_stats=False are not supported)")
        return float(layers[0].eps)

    def _train_context(self, device_index: int, params=None):
        """(context of the training entries on ``device_index``, ``params`` -- default: the current parameters -- as one float32
        blob on that device in ``parameters()`` order)."""
        from kws import _native

        if self._train_ctx is None or self._train_ctx.device != device_index:
            self._train_ctx = _native.Context(device_index, ModelError)
        self._train_ctx.use_torch_stream()
        dev = torch.device("cuda", device_index)
        params = tuple(self.parameters()) if params is None else tuple(params)
        return self._train_ctx, torch.cat([p.detach().to(dev, torch.float32).reshape(-1) for p in params])

    def _forward_native(self, x: torch.Tensor):
        """The train-mode forward on ``x`` (checked by the caller) -> (logits, labels), and the update of the running statistics;
        no autograd graph."""
        eps = self._eps()
        ctx, blob = self._train_context(x.device.index or 0)
        x = x.detach().to(torch.float32).contiguous()
        logits = torch.empty((x.shape[0], self.num_classes), dtype=torch.float32, device=x.device)
        labels = torch.empty((x.shape[0],), dtype=torch.int32, device=x.device)
        stats = torch.empty((9, 2, 64), dtype=torch.float32, device=x.device)
        ctx.dscnn_bn_train_forward_f32(blob, self.num_classes, x, eps, logits, labels, stats)
        self._update_running(stats)
        return logits, labels

    @torch.no_grad()
    def _update_running(self, stats: torch.Tensor) -> None:
        """running <- (1 - momentum) * running + momentum * batch for the 18 buffers, num_batches_tracked += 1: one fused launch
        per distinct momentum (one by default), no host synchronisation."""
        layers = self.bn_layers()
        by_momentum = {}
        for i, m in enumerate(layers):
            bufs, srcs = by_momentum.setdefault(float(m.momentum), ([], []))
            for j, buf in enumerate((m.running_mean, m.running_var)):
                bufs.append(buf)
                srcs.append(stats[i, j].to(buf.device, buf.dtype))
        for momentum, (bufs, srcs) in by_momentum.items():
            torch._foreach_lerp_(bufs, srcs, momentum)
        torch._foreach_add_([m.num_batches_tracked for m in layers], 1)

    def _native_backward(self, ctx, x, dl, grad):
        native, blob = ctx
        native.dscnn_bn_backward_f32(blob, self.num_classes, x, self._eps(), dl, grad)

    def infer_pcm16(self, wav: torch.Tensor):
        return self.fold().infer_pcm16(wav)

    # what the spotters run a model through: the fold is an ordinary DS-CNN, so its context, its packed weights and its hooks serve
    _family = DepthwiseSeparableConv._family
    _host_ingest = DepthwiseSeparableConv._host_ingest
    _stream_graph = DepthwiseSeparableConv._stream_graph
    _stream_zero_copy = DepthwiseSeparableConv._stream_zero_copy

    def _context(self, device_index: int, params=None):
        return self.fold()._context(device_index, params)

    def packed_weights(self) -> np.ndarray:
        return self.fold().packed_weights()

    def _native_infer_i16(self, ctx, wav, logits, labels):
        self.fold()._native_infer_i16(ctx, wav, logits, labels)

    def _native_infer_f32(self, ctx, wav, logits, labels):
        self.fold()._native_infer_f32(ctx, wav, logits, labels)

    def _native_scan(self, ctx, x, hop, logits, labels):
        self.fold()._native_scan(ctx, x, hop, logits, labels)

    def _native_scan_ragged(self, ctx, buf, start, length, hop, logits, labels):
        self.fold()._native_scan_ragged(ctx, buf, start, length, hop, logits, labels)

    def _native_stream_load(self, ctx):
        self.fold()._native_stream_load(ctx)

    def _native_stream_push(self, ctx, hop, logits, labels, use_graph=False):
        self.fold()._native_stream_push(ctx, hop, logits, labels, use_graph)


class CnnTradFpool3(_TrainableNative):
    """Build-defined model-zoo member: Sainath & Parada's cnn-trad-fpool3 on the reference's
    ``[1,99,10]`` MFCC map with SAME padding -- conv 64x(20x8)+ReLU, max-pool 1x3 over frequency, conv 64x(10x4)+ReLU,
    flatten, Linear 32, Linear 128+ReLU, Linear C.  The modules hold parameters; ``forward`` is
    ``kws_forward_cnn_trad_f32`` (both convolutions as implicit GEMMs on the bf16 matrix pipe with the exact
    three-way split, the dense tail batched on the VALU).

    Trainable like ``DepthwiseSeparableConv``: after an explicit ``model.train()``, when ``torch.is_grad_enabled()`` and some
    parameter requires grad, ``forward`` runs through ``_NativeTrainFunction`` -- the same inference call (logits and labels
    bit-identical to a call under ``torch.no_grad()``) with a backward that recomputes the activations in f32 and computes all
    ten parameter gradients in HIP (``kws_cnn_trad_backward_f32``, deterministic, independent of ``kws_set_cnn_trad_math``).
    Each gradient lands on its parameter's device.  No gradient with respect to the input features is provided (an input that
    requires grad raises ``ModelError`` in backward).  Otherwise -- no ``train()``, ``eval()``, ``torch.no_grad()``, frozen
    parameters -- no autograd graph is built.  Parameters on the GPU are re-uploaded after an optimizer step without leaving
    the device (``kws_load_cnn_trad_device``); CPU-resident parameters go through the host load.  ``infer_pcm16`` is
    BASELINE.json configs[2]."""

    _name = "CnnTradFpool3"
    _backward_entry = "kws_cnn_trad_backward_f32"
    _family = "cnn_trad"
    _pcm16_is = "the path is HIP kernels"

    def __init__(self, num_classes: int = 12):
        super().__init__(num_classes)
        self.conv1 = nn.Conv2d(1, 64, kernel_size=(20, 8))
        self.conv2 = nn.Conv2d(64, 64, kernel_size=(10, 4))
        self.lin = nn.Linear(64 * 99 * 3, 32)
        self.dnn = nn.Linear(32, 128)
        self.fc = nn.Linear(128, num_classes)

    def _load_host(self, ctx, blob):
        ctx.load_cnn_trad(blob, self.num_classes)

    def _load_device(self, ctx, blob):
        ctx.load_cnn_trad_device(blob, self.num_classes)

    def _check_features(self, x):
        if x.dim() != 4 or tuple(x.shape[1:]) != FEATURE_SHAPE:
            raise ModelError(f"expected input [B,1,99,10], got {tuple(x.shape)}")

    def _native_forward(self, ctx, x, logits, labels):
        ctx.forward_cnn_trad_f32(x, logits, labels)

    def _native_backward(self, ctx, x, dl, grad):
        ctx.cnn_trad_backward_f32(x, dl, grad)

    def _native_infer_i16(self, ctx, wav, logits, labels):
        ctx.infer_cnn_trad_i16(wav, logits, labels)

    def _native_infer_f32(self, ctx, wav, logits, labels):
        ctx.infer_cnn_trad_f32(wav, logits, labels)

    def _native_scan(self, ctx, x, hop, logits, labels):
        (ctx.scan_cnn_trad_f32 if x.dtype == torch.float32 else ctx.scan_cnn_trad_i16)(x, hop, logits, labels)

    def _native_scan_ragged(self, ctx, buf, start, length, hop, logits, labels):
        (ctx.scan_ragged_cnn_trad_f32 if buf.dtype == torch.float32 else ctx.scan_ragged_cnn_trad_i16)(buf, start, length, hop, logits,
                                                                                                     labels)

    def _native_stream_load(self, ctx):
        ctx.load_cnn_trad(self.packed_weights(), self.num_classes)

    def _native_stream_push(self, ctx, hop, logits, labels, use_graph=False):
        if use_graph:
            raise ModelError("CnnTradFpool3: the streaming push has no captured-graph variant (kws_stream_push_cnn_trad_i16)")
        ctx.stream_push_cnn_trad_i16(hop, logits, labels)
