"""Stage-2 crop enhancement on the GPU: the reference's `ImageEnhancer.enhance_clahe_bilateral`
(src/image_enhancement.py:146-183, enhancement method "clahe") for every crop of a frame batch.

BGR -> Lab, CLAHE on L, Lab -> BGR and the bilateral filter run on device-resident crops in three HIP launches per call
(`rtd_enhance_crops`, csrc/enhance.hip), asynchronously on torch's current stream; the arithmetic is restated in
tests/enhance_ref.py and matched bit for bit.  `CropBatcher.preprocess_batch(..., enhancer=e)` feeds the enhanced crops straight to
the unchanged crop-resize launch, `BatchedStage2(pipeline, enhancer="auto")` builds the enhancer from the pipeline's own
`ImageEnhancer` object.  Method "realesrgan" is served by esrgan.py (`UpscalingEnhancer`, an opt-in that chains the x4 network with this
enhancer): `from_reference` here and "auto" keep answering None for it.  Out of scope: one-channel crops and the
reference's LRU cache of enhanced crops.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _capi

# the limits of rtd_enhance_create / rtd_enhance_crops (include/rtdetr_mi355.h)
MAX_CROPS_PER_CALL = _capi.MAX_CROPS_PER_CALL
MAX_TILES = 16
MAX_RADIUS = 7
MIN_CROP_SIDE = 16


def bilateral_radius(d: int, sigma_space: float) -> int:
    """cv2.bilateralFilter's radius: d / 2 for d > 0, else rint(1.5 sigma_space); at least 1"""
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    return max(int(d) // 2 if d > 0 else int(np.rint(ss * 1.5)), 1)


def within_limits(tile_grid_size, bilateral_d, sigma_space) -> bool:
    try:
        tx, ty = (int(v) for v in tile_grid_size)
    except (TypeError, ValueError):
        return False
    return 1 <= tx <= MAX_TILES and 1 <= ty <= MAX_TILES and 1 <= bilateral_radius(int(bilateral_d), float(sigma_space)) <= MAX_RADIUS


def layout(rects: Sequence[Sequence[int]]) -> List[int]:
    """rtd_enhance_layout: byte offsets of the crops (x1, y1, x2, y2) in the output buffer, plus its size.  Host arithmetic only."""
    return _capi.crop_layout("rtd_enhance", rects)


class CropEnhancer(_capi.CropHandle):
    """One rtd_enhance handle.  The parameters are the reference's (`clahe_clip_limit`, `clahe_tile_grid_size` = (tilesX, tilesY),
    `bilateral_d`, `bilateral_sigma_color`, `bilateral_sigma_space`); the library takes the three real ones as float32, and `params`
    holds the values it actually uses.  Calls are asynchronous on torch's current stream; the handle's scratch belongs to the call in
    flight, so use one enhancer from one stream at a time."""

    _prefix, _what = "rtd_enhance", "libmi355rtdetr"

    def __init__(self, clip_limit: float = 2.0, tile_grid_size=(8, 8), bilateral_d: int = 9, sigma_color: float = 75, sigma_space: float = 75,
                 device: int = 0):
        p = _capi.RtdEnhanceParams()
        p.struct_size = C.sizeof(_capi.RtdEnhanceParams)
        p.clip_limit = float(clip_limit)
        p.tiles_x, p.tiles_y = int(tile_grid_size[0]), int(tile_grid_size[1])
        p.bilateral_d = int(bilateral_d)
        p.sigma_color, p.sigma_space = float(sigma_color), float(sigma_space)
        self.params = {"clip_limit": float(p.clip_limit), "tile_grid_size": (p.tiles_x, p.tiles_y), "bilateral_d": p.bilateral_d,
                       "sigma_color": float(p.sigma_color), "sigma_space": float(p.sigma_space)}
        self.device = int(device)
        self._open(self.device, C.byref(p))

    @classmethod
    def from_reference(cls, image_enhancer, min_crop_size: int, device: int = 0) -> Optional["CropEnhancer"]:
        """The device enhancer of a reference `ImageEnhancer` object (its `method`, `clahe_*` and `bilateral_*` attributes), or None
        when the batched path cannot stand in for it: any method but "clahe", parameters beyond the library's limits, or a pipeline
        whose crops may be smaller than 16 pixels per side."""
        if image_enhancer is None or getattr(image_enhancer, "method", None) != "clahe":
            return None
        if int(min_crop_size) < MIN_CROP_SIDE:
            return None
        grid = getattr(image_enhancer, "clahe_tile_grid_size", (8, 8))
        d = getattr(image_enhancer, "bilateral_d", 9)
        ss = getattr(image_enhancer, "bilateral_sigma_space", 75)
        if not within_limits(grid, d, ss):
            return None
        return cls(clip_limit=getattr(image_enhancer, "clahe_clip_limit", 2.0), tile_grid_size=grid, bilateral_d=d,
                   sigma_color=getattr(image_enhancer, "bilateral_sigma_color", 75), sigma_space=ss, device=device)

    def enhance(self, frames, rects_per_frame) -> Tuple["object", List[int], List[Tuple[int, int]]]:
        """frames: device uint8 HWC BGR tensors; rects_per_frame: per frame a list of (x1, y1, x2, y2).  Returns (buffer, offsets,
        shapes): one uint8 device tensor holding every enhanced crop (frame-major order), crop i being buffer[offsets[i]:][:h * w * 3]
        viewed as (h, w, 3) with shapes[i] = (h, w); offsets has one more entry, the buffer's size.  Enqueued on torch's current
        stream: the buffer is ready when that stream reaches it."""
        return self._crop_call("crops", 1, frames, rects_per_frame)

    def debug_stage(self, crop: int, stage: int, shape) -> np.ndarray:
        """rtd_debug_enhance_stage: 0 = Lab (h, w, 3), 1 = LUTs (tiles_y, tiles_x, 256), 2 = BGR before the bilateral filter; `crop`
        counts inside the LAST rtd_enhance_crops call (the last chunk of an enhance())."""
        out = np.zeros(shape, np.uint8)
        self._check(self._L.rtd_debug_enhance_stage(self._h, int(crop), int(stage), out.ctypes.data, out.nbytes))
        return out
