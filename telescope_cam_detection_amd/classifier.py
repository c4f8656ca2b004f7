"""The Stage-2 species classifier network on the GPU: timm's EVA02 ViT behind `SpeciesClassifier.model`
(src/species_classifier.py: `logits = self.model(batch)`; config/config.yaml names timm/eva02_large_patch14_clip_336.merged2b_ft_inat21).

`Eva02Classifier` owns one rtd_eva handle (csrc/classifier.hip): every GEMM runs on the library's conv kernels in the fp16 hi + lo pair
format ("f16x3") or in fp32, attention on pair MFMAs, asynchronously on torch's current stream.  It is callable like the timm module -
[N, 3, S, S] fp32 in, [N, classes] fp32 logits out - so `install()` can put it where the reference keeps the timm model:

    install(pipeline.species_classifiers["bird"], "models/eva02_inat21/model.safetensors")
    BatchedStage2(pipeline)            # and the reference's own classify() / classify_batch() run unchanged, without timm

The arithmetic is restated in tests/eva_ref.py; the checkpoint conversion lives in eva_checkpoint.py.  Out of scope: other timm
families, head dims other than 64, pos_embed resampling, bf16 storage, softmax / top-k (BatchedStage2 keeps torch's).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Mapping, Optional

import numpy as np

from . import _capi
from .eva_checkpoint import POOLS, EvaArch, cached_blob, make_blob

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # timm's default_cfg of the eva02 clip-pretrained models
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def eva_config(arch: EvaArch, device: int = 0, precision="f16x3", max_batch: int = 16) -> _capi.RtdEvaConfig:
    c = _capi.RtdEvaConfig()
    c.struct_size = C.sizeof(_capi.RtdEvaConfig)
    c.device, c.precision, c.max_batch = int(device), _capi.precision_code(precision), int(max_batch)
    c.img, c.patch, c.dim, c.depth, c.heads, c.hidden = arch.img, arch.patch, arch.dim, arch.depth, arch.heads, arch.hidden
    c.classes, c.ref_feat = arch.classes, arch.ref_feat
    c.scale_attn_inner, c.scale_mlp, c.pool = int(arch.scale_attn_inner), int(arch.scale_mlp), POOLS[arch.pool]
    return c


class Eva02Classifier(_capi.Handle):
    """One rtd_eva handle.  checkpoint: a path (timm's model.safetensors, or a torch.save state dict, optionally under
    `model_state_dict`), a state dict, or a blob `eva_checkpoint.make_blob` returned together with `arch`.  Calls are asynchronous on
    torch's current stream; the handle's arena belongs to the call in flight, so use one classifier from one stream at a time."""

    _prefix, _what = "rtd_eva", "libmi355rtdetr"

    def __init__(self, checkpoint, precision="f16x3", device=0, max_batch: int = 16, arch: Optional[EvaArch] = None):
        if isinstance(checkpoint, (bytes, bytearray)):
            if arch is None:
                raise ValueError("a packed blob needs its EvaArch")
            blob = checkpoint
        elif isinstance(checkpoint, Mapping):
            arch, blob = make_blob(checkpoint, arch)
        elif arch is None:
            arch, blob = cached_blob(os.fspath(checkpoint))
        else:
            arch, blob = make_blob(os.fspath(checkpoint), arch)
        if isinstance(device, str):                  # 'cuda:1' (the reference's SpeciesClassifier.device is a string)
            device = int(device.split(":")[1]) if ":" in device else 0
        self.arch, self.device, self.max_batch = arch, _capi.device_index(device), int(max_batch)
        self.precision = _capi.precision_code(precision)
        cfg = eva_config(arch, self.device, precision, max_batch)
        self._open(C.byref(cfg), (C.c_char * len(blob)).from_buffer_copy(blob), len(blob))

    # ---- the parts of nn.Module the reference touches
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def __call__(self, x):
        """x: [N, 3, S, S] fp32 on the handle's device -> logits [N, classes] fp32, enqueued on torch's current stream.  Batches above
        max_batch are chunked."""
        import torch

        S = self.arch.img
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and tuple(x.shape[1:]) == (3, S, S)):
            raise ValueError(f"expected a device tensor [N, 3, {S}, {S}], got {tuple(getattr(x, 'shape', ()))}")
        x = x.to(torch.float32).contiguous()
        out = torch.empty((x.shape[0], self.arch.classes), dtype=torch.float32, device=x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        for i0 in range(0, x.shape[0], self.max_batch):
            n = min(self.max_batch, x.shape[0] - i0)
            self._check(self._L.rtd_eva_forward(self._h, C.c_void_p(x[i0:].data_ptr()), n, C.c_void_p(out[i0:].data_ptr()), stream))
        self._keep = x          # (rtd_debug_eva_tensor re-reads the last chunk's input)
        return out

    forward = __call__

    def self_check(self) -> int:
        """rtd_eva_self_check: values of the last call's residual stream and logits at (or beyond) fp16's range; 0 = healthy"""
        n = C.c_int64(-1)
        self._check(self._L.rtd_eva_self_check(self._h, C.byref(n)))
        return int(n.value)

    def arena_bytes(self) -> int:
        return int(self._L.rtd_eva_arena_bytes(self._h))

    def debug_tensor(self, name: str) -> np.ndarray:
        """rtd_debug_eva_tensor: a float stage output [N, rows, C] of the last call (its last chunk)"""
        shape = (C.c_int64 * 4)()
        self._check(self._L.rtd_debug_eva_tensor(self._h, name.encode(), None, 0, shape))
        out = np.zeros((shape[0], shape[2], shape[3]), np.float32)
        self._check(self._L.rtd_debug_eva_tensor(self._h, name.encode(), out.ctypes.data, out.size, shape))
        return out

    def wait_stream(self, producer_stream: int) -> None:
        """the handle owns no stream (every call runs on the caller's): there is nothing to order, and no rtd_eva_wait_stream"""
        raise _capi.RtdError(_capi.RTD_E_STATE, "rtd_eva owns no stream: enqueue the producer and the call on the same stream, or order them with torch events")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.rtd_eva_close(self._h)
            self._h = C.c_void_p()


def install(species_classifier, checkpoint, precision="f16x3", max_batch: int = 16, mean=None, std=None, arch: Optional[EvaArch] = None):
    """Put an `Eva02Classifier` where the reference's `SpeciesClassifier` keeps its timm model: sets `.model`, `.input_size`,
    `_mean_tensor` and `_std_tensor` (what `load_model()` would have set, src/species_classifier.py:258-275), so `classify()`,
    `classify_batch()` and `BatchedStage2` run unchanged and without timm.  mean / std: default the classifier's own `.mean` / `.std`,
    else the CLIP statistics of the eva02 clip models.  Returns the Eva02Classifier."""
    import torch

    if callable(checkpoint) and hasattr(checkpoint, "arch"):          # an Eva02Classifier built elsewhere (one handle for several categories)
        model = checkpoint
    else:
        dev = getattr(species_classifier, "device", None) or "cuda:0"
        model = Eva02Classifier(checkpoint, precision=precision, device=dev, max_batch=max_batch, arch=arch)
    tdev = torch.device(getattr(model, "torch_device", None) or f"cuda:{model.device}")
    mean = mean if mean is not None else getattr(species_classifier, "mean", None) or OPENAI_CLIP_MEAN
    std = std if std is not None else getattr(species_classifier, "std", None) or OPENAI_CLIP_STD
    species_classifier.model = model
    species_classifier.input_size = model.arch.img
    species_classifier.mean, species_classifier.std = tuple(mean), tuple(std)
    species_classifier._mean_tensor = torch.tensor(tuple(mean), device=tdev, dtype=torch.float32).view(3, 1, 1)
    species_classifier._std_tensor = torch.tensor(tuple(std), device=tdev, dtype=torch.float32).view(3, 1, 1)
    return model
