"""Empty-frame filter on the GPU: the reference's `EmptyFrameFilter` (src/empty_frame_filter.py, config key
`performance.empty_frame_filter`) as a batched motion gate ahead of detection.

The reference checks each frame on the CPU with cv2 (gray, Gaussian blur, absdiff, threshold, countNonZero) and only on the
non-coordinator path (src/inference_engine_yolox.py:588-593).  Here the check is one HIP launch per batch (csrc/motion.hip,
rtd_motion_* in include/rtdetr_mi355.h) that decides exactly as OpenCV does on 8-bit frames (restated in tests/motion_ref.py), for
numpy frames, host tensors and device-resident tensors alike.

* `EmptyFrameFilter(min_motion_area=200, threshold=25, blur_size=21, device=None)`: drop-in for the reference's class - `has_motion(frame)`,
  `reset()`, `get_stats()` with the same five keys and counting - plus `has_motion_batch(frames, keys)` (one library call per batch, one
  stored frame per camera key; a key of None is never gated) and per-camera `reset(key)` / `get_stats(key)`.
* `install(engine_module)`: the reference's InferenceEngine builds this filter for its non-coordinator path.
The coordinator path is batching.BatchCoordinator(empty_frame_filter=...), built from the config by batching.make_rtdetr_coordinator.

Deliberate deviation: a frame whose size differs from the camera's stored one counts as a first frame (True, state replaced) where the
reference would raise inside cv2.absdiff.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _capi

logger = logging.getLogger(__name__)

MAX_BLUR = 63
_SINGLE = object()           # the camera key of has_motion(frame): the reference's filter holds one stored frame


def odd_blur(blur_size: int) -> int:
    """upstream's `blur_size if blur_size % 2 == 1 else blur_size + 1`; 1..63 taps are supported"""
    k = int(blur_size)
    k = k if k % 2 == 1 else k + 1
    if not 1 <= k <= MAX_BLUR:
        raise ValueError(f"blur_size {blur_size} gives a {k}-tap kernel: 1..{MAX_BLUR} taps are supported")
    return k


class DeviceBackend(_capi.Handle):
    """One rtd_motion handle: the per-slot stored frames live on the device.  A test may hand EmptyFrameFilter another object with the
    same four methods (tests/motion_ref.py RefBackend)."""

    _prefix, _what = "rtd_motion", "the motion gate"

    def __init__(self, device: int, blur_size: int):
        self._open(int(device), int(blur_size))

    def check(self, frames: Sequence, on_device: bool, slots: Sequence[int], threshold: int) -> List[int]:
        """frames: HxWxC uint8 (C = 1 or 3) - C-contiguous numpy arrays, or contiguous device tensors when on_device."""
        n, ptrs, hwc = _capi.c_frames(*_capi.frame_ptrs(frames, on_device))
        sl = (C.c_int32 * max(n, 1))(*[int(s) for s in slots])
        area = (C.c_int64 * max(n, 1))()
        self._check(self._L.rtd_motion_check(self._h, n, ptrs, hwc, int(bool(on_device)), sl, int(threshold), area))
        return list(area)[:n]

    def reset(self, slot: int = -1) -> None:
        self._check(self._L.rtd_motion_reset(self._h, int(slot)))

    def state(self, slot: int, shape) -> np.ndarray:
        """the blurred frame the slot holds (rtd_debug_motion_state)"""
        out = np.zeros(tuple(shape), np.uint8)
        self._check(self._L.rtd_debug_motion_state(self._h, int(slot), out.ctypes.data, out.nbytes))
        return out


def _as_hwc(frame):
    """(HxWxC uint8 array or contiguous device tensor, on_device).  A 2-D frame is one-channel; C must be 1 or 3."""
    if hasattr(frame, "is_cuda"):
        import torch
        if frame.dtype != torch.uint8:
            raise ValueError(f"frames must be uint8, got {frame.dtype}")
        if frame.is_cuda:
            t = frame if frame.dim() != 2 else frame.unsqueeze(-1)
            if t.dim() != 3 or t.shape[2] not in (1, 3):
                raise ValueError(f"frames must be HxW or HxWxC with C = 1 or 3, got shape {tuple(frame.shape)}")
            return t.contiguous(), True
        frame = frame.numpy()
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise ValueError(f"frames must be uint8, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"frames must be HxW or HxWxC with C = 1 or 3, got shape {a.shape}")
    return np.ascontiguousarray(a), False


class EmptyFrameFilter:
    """Motion gate: True = run detection on the frame, False = nothing moved since the camera's previous frame (skip it).

    Same constructor, decisions and statistics as the reference's EmptyFrameFilter; the stored blurred frames live on the GPU (one per
    camera key).  `backend` is the only seam: an object with check / reset / wait_stream (DeviceBackend by default)."""

    def __init__(self, min_motion_area: int = 200, threshold: int = 25, blur_size: int = 21, device=None, backend=None):
        self.min_motion_area = min_motion_area
        self.threshold = threshold
        self.blur_size = odd_blur(blur_size)
        self.device = device = _capi.device_index(device)
        self._backend = backend if backend is not None else DeviceBackend(device, self.blur_size)
        self._slots: Dict[Any, int] = {}
        self._counts: Dict[Any, List[int]] = {}      # key -> [total, skipped, motion]
        logger.info(f"EmptyFrameFilter (GPU) initialized: min_motion_area={min_motion_area}px², threshold={threshold}, "
                    f"blur_size={self.blur_size}, device={device}")

    def _int_threshold(self) -> int:
        # cv2.threshold on 8-bit input compares with floor(threshold); anything < 0 counts every pixel, >= 255 none
        return int(min(max(math.floor(self.threshold), -1), 255))

    # ---- the reference's surface ------------------------------------------------------------------------------------------------
    def has_motion(self, frame) -> bool:
        return self.has_motion_batch([frame], [_SINGLE])[0]

    def reset(self, key=None) -> None:
        """Forget the stored frames (all cameras, or the camera `key`): the next frame is a first frame again."""
        if key is None:
            self._backend.reset(-1)
        elif key in self._slots:
            self._backend.reset(self._slots[key])

    def get_stats(self, key=None) -> dict:
        """The reference's five keys: totals over every camera, or the counts of camera `key`."""
        if key is None:
            c = [sum(v[i] for v in self._counts.values()) for i in range(3)]
        else:
            c = self._counts.get(key, [0, 0, 0])
        total, skipped, motion = c
        skip_rate = skipped / max(total, 1)
        return {"total_frames": total, "skipped_frames": skipped, "motion_frames": motion, "skip_rate": skip_rate,
                "skip_rate_percent": skip_rate * 100}

    # ---- batched ----------------------------------------------------------------------------------------------------------------
    def has_motion_batch(self, frames: Sequence, keys: Sequence) -> List[bool]:
        """One decision per frame, one library call for the batch.  keys[i] is the frame's camera (any hashable); a key of None is
        never gated (True, not counted).  Two frames of one camera in a batch are applied in order."""
        if len(frames) != len(keys):
            raise ValueError(f"{len(frames)} frames but {len(keys)} keys")
        out = [True] * len(frames)
        idx = [i for i, k in enumerate(keys) if k is not None]
        if not idx:
            return out
        conv = [_as_hwc(frames[i]) for i in idx]
        on_dev = [d for _, d in conv]
        arrs = [a for a, _ in conv]
        if any(on_dev) and not all(on_dev):            # one residency per call: mixed batches go through the host
            arrs = [a.cpu().numpy() if d else a for a, d in zip(arrs, on_dev)]
            on_dev = [False] * len(arrs)
        device = bool(on_dev[0])
        if device:
            import torch
            # the frames were written on torch's current stream; the gate's own stream waits for that work (an event of the library)
            self._backend.wait_stream(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        slots = []
        for i in idx:
            k = keys[i]
            if k not in self._slots:
                self._slots[k] = len(self._slots)
            slots.append(self._slots[k])
        areas = self._backend.check(arrs, device, slots, self._int_threshold())
        for i, a in zip(idx, areas):
            c = self._counts.setdefault(keys[i], [0, 0, 0])
            c[0] += 1
            moved = a < 0 or a >= self.min_motion_area        # a first frame (-1) runs detection and counts as motion
            c[2 if moved else 1] += 1
            out[i] = moved
        return out


def install(engine_module) -> None:
    """Let the reference's InferenceEngine build the GPU filter for its non-coordinator path, without editing it:

        import src.inference_engine_yolox as e, telescope_cam_detection_amd.motion as m
        m.install(e)
    """
    engine_module.EmptyFrameFilter = EmptyFrameFilter
