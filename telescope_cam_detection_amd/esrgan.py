"""Real-ESRGAN x4 upscaling of Stage-2 crops on the GPU: the reference's `ImageEnhancer` method "realesrgan"
(src/image_enhancement.py: `RealESRGANer.enhance(outscale=4)` around RRDBNet with 23 blocks, then CLAHE + bilateral on the 4x image).

`CropUpscaler` owns one rtd_esrgan handle (csrc/esrgan.hip): the network's 351 convolutions run on the library's conv kernels in the
fp16 hi + lo pair format ("f16x3") or in fp32, asynchronously on torch's current stream; the arithmetic is restated in
tests/esrgan_ref.py.  `UpscalingEnhancer` chains it with the existing `CropEnhancer`, and has the `enhance(frames, rects_per_frame)`
interface `CropBatcher.preprocess_batch(enhancer=...)` consumes:

    BatchedStage2(p, enhancer=UpscalingEnhancer.from_reference(p.enhancer, p.min_crop_size))

`enhancer="auto"` and `CropEnhancer.from_reference` keep returning None for "realesrgan": the upscaler is an opt-in.  Out of scope:
bf16 / plain-fp16 engines, scales other than 4, one-channel and alpha crops, and the reference's LRU cache of enhanced crops.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from .enhance import MIN_CROP_SIDE, CropEnhancer, within_limits

MAX_CROPS_PER_CALL = _capi.MAX_CROPS_PER_CALL
MIN_SIDE, MAX_SIDE, MAX_ONE_PASS_SIDE = 8, 4096, 576
NUM_FEAT, NUM_GROW_CH = 64, 32


def conv_table(num_block: int) -> List[Tuple[str, int, int]]:
    """(state-dict prefix, Cin, Cout) of every convolution of RRDBNet(3, 3, 64, num_block, 32, scale 4), in execution order"""
    t = [("conv_first", 3, NUM_FEAT)]
    for i in range(num_block):
        for j in (1, 2, 3):
            for k in (1, 2, 3, 4, 5):
                t.append((f"body.{i}.rdb{j}.conv{k}", NUM_FEAT + NUM_GROW_CH * (k - 1), NUM_FEAT if k == 5 else NUM_GROW_CH))
    t += [("conv_body", NUM_FEAT, NUM_FEAT), ("conv_up1", NUM_FEAT, NUM_FEAT), ("conv_up2", NUM_FEAT, NUM_FEAT), ("conv_hr", NUM_FEAT, NUM_FEAT),
          ("conv_last", NUM_FEAT, 3)]
    return t


def num_blocks_of(state: Dict[str, object]) -> int:
    n = 0
    while f"body.{n}.rdb1.conv1.weight" in state:
        n += 1
    return n


def state_dict_of(path_or_dict) -> Dict[str, object]:
    """the key rule of the upstream checkpoints: `params_ema` if the file has it, else `params`, else the dict itself"""
    import torch

    sd = path_or_dict
    if not isinstance(sd, dict):
        sd = torch.load(os.fspath(path_or_dict), map_location="cpu")
    if not isinstance(sd, dict):
        raise _capi.RtdError(_capi.RTD_E_WEIGHTS, "checkpoint is not a dict")
    for key in ("params_ema", "params"):
        if isinstance(sd.get(key), dict):
            return sd[key]
    return sd


def load_state(path_or_dict, num_block: Optional[int] = None) -> bytes:
    """The weight blob rtd_esrgan_create reads, from an upstream checkpoint (a path for torch.load, or the loaded dict).  A missing or
    mis-shaped tensor raises RtdError with RTD_E_WEIGHTS and the tensor's name.  num_block: default = the blocks the state dict holds."""
    import torch

    from .weights import pack_blob

    sd = state_dict_of(path_or_dict)
    nb = num_blocks_of(sd) if num_block is None else int(num_block)
    if nb < 1:
        raise _capi.RtdError(_capi.RTD_E_WEIGHTS, "missing tensor body.0.rdb1.conv1.weight")
    out = {}
    for name, cin, cout in conv_table(nb):
        for suffix, shape in ((".weight", (cout, cin, 3, 3)), (".bias", (cout,))):
            t = sd.get(name + suffix)
            if t is None:
                raise _capi.RtdError(_capi.RTD_E_WEIGHTS, f"missing tensor {name + suffix}")
            t = torch.as_tensor(t)
            if tuple(t.shape) != shape:
                raise _capi.RtdError(_capi.RTD_E_WEIGHTS, f"shape mismatch: {name + suffix} is {tuple(t.shape)}, not {shape}")
            out[name + suffix] = t.detach().to(torch.float32).cpu().contiguous()
    return pack_blob(out)


def layout(rects: Sequence[Sequence[int]]) -> List[int]:
    """rtd_esrgan_layout: byte offsets of the 4x crops (x1, y1, x2, y2) in the output buffer, plus its size.  Host arithmetic only."""
    return _capi.crop_layout("rtd_esrgan", rects)


class CropUpscaler(_capi.CropHandle):
    """One rtd_esrgan handle.  state: a checkpoint path, a state dict, or the blob `load_state` returned.  Calls are asynchronous on
    torch's current stream; the handle's arena belongs to the call in flight, so use one upscaler from one stream at a time."""

    _prefix, _what = "rtd_esrgan", "libmi355rtdetr"

    def __init__(self, state, num_block: int = 23, precision="f16x3", tile: int = 512, tile_pad: int = 10, device: int = 0):
        blob = state if isinstance(state, (bytes, bytearray)) else load_state(state, num_block)
        cfg = _capi.RtdEsrganConfig()
        cfg.struct_size = C.sizeof(_capi.RtdEsrganConfig)
        cfg.device = int(device)
        cfg.precision = _capi.precision_code(precision)
        cfg.num_feat, cfg.num_grow_ch = NUM_FEAT, NUM_GROW_CH
        cfg.num_block, cfg.tile, cfg.tile_pad = int(num_block), int(tile), int(tile_pad)
        self.device, self.num_block, self.tile, self.tile_pad, self.precision = int(device), int(num_block), int(tile), int(tile_pad), cfg.precision
        self._open(C.byref(cfg), (C.c_char * len(blob)).from_buffer_copy(blob), len(blob))

    def upscale(self, frames, rects_per_frame) -> Tuple["object", List[int], List[Tuple[int, int]]]:
        """frames: device uint8 HWC BGR tensors; rects_per_frame: per frame a list of (x1, y1, x2, y2).  Returns (buffer, offsets,
        shapes): one uint8 device tensor holding every 4x crop (frame-major order), crop i being buffer[offsets[i]:][:H * W * 3] viewed
        as (H, W, 3) with shapes[i] = (H, W) = (4h, 4w).  Enqueued on torch's current stream."""
        return self._crop_call("upscale", 4, frames, rects_per_frame)

    def arena_bytes(self) -> int:
        return int(self._L.rtd_esrgan_arena_bytes(self._h))

    def debug_tensor(self, name: str) -> np.ndarray:
        """rtd_debug_esrgan_tensor: a float stage output [h, w, c] of the last tile of the last call"""
        shape = (C.c_int64 * 4)()
        self._check(self._L.rtd_debug_esrgan_tensor(self._h, name.encode(), None, 0, shape))
        out = np.zeros(tuple(shape)[1:], np.float32)
        self._check(self._L.rtd_debug_esrgan_tensor(self._h, name.encode(), out.ctypes.data, out.size, shape))
        return out


class UpscalingEnhancer:
    """Real-ESRGAN x4, then CLAHE + bilateral on the 4x image: `ImageEnhancer.enhance_realesrgan`.  enhance() upscales every crop,
    hands each 4x image to `CropEnhancer.enhance` as a frame of its own with its full rectangle, and returns that call's result."""

    def __init__(self, upscaler: CropUpscaler, crop_enhancer: CropEnhancer):
        self.upscaler, self.crop_enhancer = upscaler, crop_enhancer
        self.last_upscaled = None

    @classmethod
    def from_reference(cls, image_enhancer, min_crop_size: int, device: int = 0, precision="f16x3") -> Optional["UpscalingEnhancer"]:
        """The device enhancer of a reference `ImageEnhancer` with method "realesrgan", or None when it cannot stand in: another method,
        a scale other than 4, no readable `realesrgan_model_path`, CLAHE / bilateral parameters beyond `CropEnhancer`'s limits, or a
        pipeline whose crops may be smaller than 16 pixels per side."""
        if image_enhancer is None or getattr(image_enhancer, "method", None) != "realesrgan":
            return None
        if int(getattr(image_enhancer, "realesrgan_scale", 4)) != 4 or int(min_crop_size) < MIN_CROP_SIDE:
            return None
        path = getattr(image_enhancer, "realesrgan_model_path", None)
        if not path or not os.path.isfile(path) or not os.access(path, os.R_OK):
            return None
        grid = getattr(image_enhancer, "clahe_tile_grid_size", (8, 8))
        d = getattr(image_enhancer, "bilateral_d", 9)
        ss = getattr(image_enhancer, "bilateral_sigma_space", 75)
        if not within_limits(grid, d, ss):
            return None
        tile, pad = int(getattr(image_enhancer, "realesrgan_tile", 512)), int(getattr(image_enhancer, "realesrgan_tile_pad", 10))
        if not (tile == 0 or 16 <= tile <= 512) or not 0 <= pad <= 32:
            return None
        sd = state_dict_of(path)
        up = CropUpscaler(sd, num_block=num_blocks_of(sd), precision=precision, tile=tile, tile_pad=pad, device=device)
        ce = CropEnhancer(clip_limit=getattr(image_enhancer, "clahe_clip_limit", 2.0), tile_grid_size=grid, bilateral_d=d,
                          sigma_color=getattr(image_enhancer, "bilateral_sigma_color", 75), sigma_space=ss, device=device)
        return cls(up, ce)

    def enhance(self, frames, rects_per_frame):
        buf, offsets, shapes = self.upscaler.upscale(frames, rects_per_frame)
        images = [buf[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offsets, shapes)]
        self.last_upscaled = (buf, offsets, shapes)
        return self.crop_enhancer.enhance(images, [[(0, 0, w, h)] for h, w in shapes])

    def last_call_ms(self) -> Optional[float]:
        a, b = self.upscaler.last_call_ms(), self.crop_enhancer.last_call_ms()
        return None if a is None or b is None else a + b

    def close(self):
        self.upscaler.close()
        self.crop_enhancer.close()
