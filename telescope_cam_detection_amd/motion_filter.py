"""Motion filter on the GPU: the reference's `MotionFilter` / `AdaptiveMotionFilter` (src/motion_filter.py, config key `motion_filter`),
which `DetectionProcessor` runs on every frame that has detections.

The reference updates a cv2 MOG2 background subtractor with the frame once per detection, drops shadows from the foreground mask, blurs
it (21 x 21 Gaussian), thresholds it at 25 and keeps a detection when enough of its box moved.  Here one library call per frame does all
of a frame's detections (csrc/mog2.hip, rtd_mog2_* in include/rtdetr_mi355.h): one fused model pass per 32 updates and one launch for the
boxes, with the model resident on the device.  The arithmetic is OpenCV's, restated in tests/mog2_ref.py, for numpy frames, host tensors
and device-resident tensors alike.

* `MotionFilter(history=500, var_threshold=16, detect_shadows=True, min_motion_area=100, motion_required=True, motion_blur_size=21,
  min_motion_ratio=0.05, device=None, backend=None)`: the reference's constructor, `filter_detections`, `has_motion_in_bbox`,
  `reset_background`, `update_params`, `get_stats` and `cleanup`, with its annotations, statistics and recreate rules.
* `AdaptiveMotionFilter(day_var_threshold=16, night_var_threshold=32, day_start_hour=6, day_end_hour=20, **kw)`: the threshold follows
  `datetime.now().hour`; a change recreates the model.
* `install(detection_processor_module)`: INTEGRATION.md.

Deliberate deviations: a blur size that gives more than 63 taps (or fewer than 1) raises ValueError, and so does `history < 1`
(OpenCV divides by it; the reference's main.py refuses it too).
"""
from __future__ import annotations

import ctypes as C
import logging
import threading
from datetime import datetime
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

from . import _capi
from .motion import _as_hwc, odd_blur
from .stage2 import normalised_bbox

logger = logging.getLogger(__name__)

NMODES = 5


def _check_history(history) -> int:
    if int(history) != history or history < 1:
        raise ValueError(f"history must be an integer >= 1, got {history!r}")
    return int(history)


def roi(bbox: Dict[str, float], h: int, w: int) -> Tuple[int, int, int, int]:
    """has_motion_in_bbox's box: ensure_valid_bbox, int() truncation, clamp to [0, w] x [0, h] (may be empty)"""
    b = normalised_bbox(bbox)
    x1, y1, x2, y2 = int(b["x1"]), int(b["y1"]), int(b["x2"]), int(b["y2"])
    return max(0, x1), max(0, y1), min(w, x2), min(h, y2)


class DeviceBackend(_capi.Handle):
    """One rtd_mog2 handle: the background model lives on the device.  A test may hand MotionFilter another object with the same
    methods (tests/mog2_ref.py RefBackend)."""

    _prefix, _what = "rtd_mog2", "the motion filter"

    def __init__(self, device: int, history: int, var_threshold, detect_shadows: bool):
        self._open(int(device), int(history), float(var_threshold), int(bool(detect_shadows)))

    def configure(self, history: int, var_threshold, detect_shadows: bool) -> None:
        """a new subtractor: the model is forgotten"""
        self._check(self._L.rtd_mog2_configure(self._h, int(history), float(var_threshold), int(bool(detect_shadows))))

    def apply(self, frame, on_device: bool, rects: Sequence[Tuple[int, int, int, int]], blur_size: int) -> List[int]:
        """len(rects) model updates with `frame` (HxWxC uint8: a C-contiguous numpy array, or a contiguous device tensor when on_device);
        the motion count of each update's box"""
        n = len(rects)
        hwc = (C.c_int32 * 3)(int(frame.shape[0]), int(frame.shape[1]), int(frame.shape[2]))
        r = (C.c_int32 * max(4 * n, 1))(*[int(v) for b in rects for v in b])
        counts = (C.c_int64 * max(n, 1))()
        ptr = frame.data_ptr() if on_device else frame.ctypes.data
        self._check(self._L.rtd_mog2_apply(self._h, C.c_void_p(ptr), hwc, int(bool(on_device)), n, r, int(blur_size), counts))
        return list(counts)[:n]

    def model(self) -> Dict[str, Any]:
        """the model in a canonical layout (rtd_debug_mog2_model): weight / variance [H, W, 5], mean [H, W, 5, C], modes_used [H, W],
        nframes; None when the filter holds no model"""
        hwc = (C.c_int32 * 3)()
        nf = C.c_int64()
        self._check(self._L.rtd_debug_mog2_model(self._h, hwc, C.byref(nf), None, None, None, None, 0))
        H, W, Ch = hwc
        if H == 0:
            return None
        out = {"weight": np.zeros((H, W, NMODES), np.float32), "variance": np.zeros((H, W, NMODES), np.float32),
               "mean": np.zeros((H, W, NMODES, Ch), np.float32), "modes_used": np.zeros((H, W), np.uint8)}
        self._check(self._L.rtd_debug_mog2_model(self._h, hwc, C.byref(nf), out["weight"].ctypes.data, out["variance"].ctypes.data,
                                                 out["mean"].ctypes.data, out["modes_used"].ctypes.data, H * W))
        out["nframes"] = int(nf.value)
        return out

    def fg_bits(self, n: int, shape) -> np.ndarray:
        """the foreground words of the last apply of n updates: [ceil(n / 32), H, W] uint32"""
        out = np.zeros(((n + 31) // 32,) + tuple(shape), np.uint32)
        self._check(self._L.rtd_debug_mog2_fg_bits(self._h, out.ctypes.data, out.size))
        return out


class MotionFilter:
    """Keeps the detections whose box moved, as judged by a MOG2 background model of the camera's frames.

    Same constructor, decisions, annotations and statistics as the reference's MotionFilter; the model lives on the GPU.  `backend` is
    the only seam: an object with configure / apply / wait_stream / close (DeviceBackend by default)."""

    def __init__(self, history: int = 500, var_threshold: int = 16, detect_shadows: bool = True, min_motion_area: int = 100,
                 motion_required: bool = True, motion_blur_size: int = 21, min_motion_ratio: float = 0.05, device=None, backend=None):
        self.history = _check_history(history)
        self.var_threshold = var_threshold
        self.detect_shadows = detect_shadows
        self.min_motion_area = min_motion_area          # stored, as in the reference; it decides nothing
        self.motion_required = motion_required
        self.motion_blur_size = odd_blur(motion_blur_size)
        self.min_motion_ratio = min_motion_ratio
        self.device = _capi.device_index(device)
        self._lock = threading.RLock()                  # hot reload calls update_params from another thread
        self._new_backend = (lambda: backend) if backend is not None else (
            lambda: DeviceBackend(self.device, self.history, self.var_threshold, self.detect_shadows))
        self.bg_subtractor = self._new_backend()
        self.total_frames = 0
        self.total_detections_filtered = 0
        logger.info(f"MotionFilter (GPU) initialized (history={history}, var_threshold={var_threshold})")

    def _recreate(self) -> None:
        """the reference's `bg_subtractor = cv2.createBackgroundSubtractorMOG2(...)`: a fresh model"""
        if self.bg_subtractor is None:
            self.bg_subtractor = self._new_backend()
        self.bg_subtractor.configure(self.history, self.var_threshold, self.detect_shadows)

    def _counts(self, frame, rects) -> List[int]:
        arr, on_device = frame
        if on_device:
            import torch
            # the frame was written on torch's current stream: the filter's own stream waits for that work
            self.bg_subtractor.wait_stream(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        return self.bg_subtractor.apply(arr, on_device, rects, self.motion_blur_size)

    def _decide(self, rect, count: int, min_motion_pixels: int) -> Tuple[bool, float]:
        x1, y1, x2, y2 = rect
        if x2 <= x1 or y2 <= y1:
            return False, 0.0
        ratio = count / ((x2 - x1) * (y2 - y1))
        return count >= min_motion_pixels and ratio > self.min_motion_ratio, ratio

    # ---- the reference's surface ------------------------------------------------------------------------------------------------
    def has_motion_in_bbox(self, frame, bbox: Dict[str, float], min_motion_pixels: int = 10) -> Tuple[bool, float]:
        """One model update with `frame`, then (has_motion, motion_ratio) of `bbox`.  The update happens even when the box is empty."""
        with self._lock:
            f = _as_hwc(frame)
            rect = roi(bbox, int(f[0].shape[0]), int(f[0].shape[1]))
            return self._decide(rect, self._counts(f, [rect])[0], min_motion_pixels)

    def filter_detections(self, frame, detections: List[Dict[str, Any]]) -> List[Dict[str, Any]]:
        """The detections whose box moved, annotated with has_motion / motion_ratio.  One model update per detection, in order, all in
        one library call."""
        if not self.motion_required or len(detections) == 0:
            return detections
        with self._lock:
            self.total_frames += 1
            f = _as_hwc(frame)
            h, w = int(f[0].shape[0]), int(f[0].shape[1])
            rects = [roi(det["bbox"], h, w) for det in detections]
            counts = self._counts(f, rects)
            filtered = []
            for det, rect, count in zip(detections, rects, counts):
                has_motion, motion_ratio = self._decide(rect, count, 10)
                if has_motion:
                    det["has_motion"] = True
                    det["motion_ratio"] = motion_ratio
                    filtered.append(det)
                else:
                    self.total_detections_filtered += 1
        if len(detections) > len(filtered):
            logger.debug(f"Motion filter: {len(detections)} → {len(filtered)} detections ({len(detections) - len(filtered)} filtered)")
        return filtered

    def cleanup(self) -> None:
        """Free the model's device memory (DetectionProcessor.stop calls this)."""
        with self._lock:
            if self.bg_subtractor is not None:
                self.bg_subtractor.close()
                self.bg_subtractor = None
                logger.debug("Motion filter resources released")

    def reset_background(self) -> None:
        """Forget the background model (camera moved, lighting changed)."""
        with self._lock:
            self._recreate()
        logger.info("Background model reset")

    def update_params(self, config: Dict[str, Any]) -> None:
        """Hot reload.  A change of history, var_threshold or detect_shadows recreates the model; the other keys keep it."""
        with self._lock:
            if "history" in config:
                _check_history(config["history"])
            blur = odd_blur(config["motion_blur_size"]) if "motion_blur_size" in config else None
            updated = []
            for key in ("history", "var_threshold", "detect_shadows", "min_motion_area"):
                if key in config and config[key] != getattr(self, key):
                    setattr(self, key, config[key])
                    updated.append(f"{key}: {config[key]}")
            if blur is not None and blur != self.motion_blur_size:
                self.motion_blur_size = blur
                updated.append(f"motion_blur_size: {blur}")
            if "min_motion_ratio" in config and config["min_motion_ratio"] != self.min_motion_ratio:
                self.min_motion_ratio = config["min_motion_ratio"]
                updated.append(f"min_motion_ratio: {self.min_motion_ratio}")
            if any(p.startswith(("history:", "var_threshold:", "detect_shadows:")) for p in updated):
                self._recreate()
                logger.info("Motion filter background subtractor recreated with new parameters")
        if updated:
            logger.info(f"MotionFilter params updated: {', '.join(updated)}")

    def get_stats(self) -> Dict[str, Any]:
        return {"total_frames": self.total_frames, "total_detections_filtered": self.total_detections_filtered,
                "motion_required": self.motion_required}


class AdaptiveMotionFilter(MotionFilter):
    """MotionFilter whose var_threshold follows the time of day (day: day_var_threshold, night: night_var_threshold).  A change
    recreates the model."""

    def __init__(self, day_var_threshold: int = 16, night_var_threshold: int = 32, day_start_hour: int = 6, day_end_hour: int = 20,
                 **kwargs):
        super().__init__(var_threshold=day_var_threshold, **kwargs)
        self.day_var_threshold = day_var_threshold
        self.night_var_threshold = night_var_threshold
        self.day_start_hour = day_start_hour
        self.day_end_hour = day_end_hour

    def _is_daytime(self) -> bool:
        return self.day_start_hour <= datetime.now().hour < self.day_end_hour

    def filter_detections(self, frame, detections: List[Dict[str, Any]]) -> List[Dict[str, Any]]:
        current = self.day_var_threshold if self._is_daytime() else self.night_var_threshold
        with self._lock:
            if current != self.var_threshold:
                self.var_threshold = current
                self._recreate()
        return super().filter_detections(frame, detections)


def install(detection_processor_module) -> None:
    """Let the reference's DetectionProcessor build the GPU filter, without editing it:

        import src.detection_processor as dp, telescope_cam_detection_amd.motion_filter as mf
        mf.install(dp)

    src/motion_filter.py imports cv2 at module level; where cv2 is absent, alias the module before src.detection_processor is
    imported."""
    detection_processor_module.MotionFilter = MotionFilter
