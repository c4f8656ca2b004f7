"""JPEG encoder for device-resident frames: the reference's `cv2.imencode('.jpg', frame, [cv2.IMWRITE_JPEG_QUALITY, q])` of
src/snapshot_saver.py (`add_frame_to_buffer`, the pre-detection ring buffer) and of the MJPEG loop in src/web_server.py, without the
copy of the raw frame to the host.

The transform, the Huffman coding and the byte stuffing run on the GPU (csrc/jpeg.hip, rtd_jpeg_* in include/rtdetr_mi355.h); what
comes back is a complete baseline JFIF file, byte for byte the one libjpeg writes at its defaults (restated in tests/jpeg_ref.py), so
`cv2.imdecode` and every other reader take it.

* `JpegEncoder(device=None)`: `encode(frame, quality=95) -> bytes`, `encode_batch(frames, quality=95) -> List[bytes]` (one library
  call per batch) for numpy frames, host tensors and device tensors (HxW or HxWxC uint8, C = 1 or 3 = BGR).
* `imencode(ext, frame, params=None)`: the call shape of cv2.imencode for '.jpg' / '.jpeg' with IMWRITE_JPEG_QUALITY.
* `install(snapshot_saver_module)`: SnapshotSaver.add_frame_to_buffer keeps device frames on the device.
"""
from __future__ import annotations

import ctypes as C
import logging
import threading
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi
from ._capi import device_index as _device_index   # (overlay.py imports it from here)
from .motion import _as_hwc

logger = logging.getLogger(__name__)

IMWRITE_JPEG_QUALITY = 1     # cv2.IMWRITE_JPEG_QUALITY
DEFAULT_QUALITY = 95         # OpenCV's default
SNAPSHOT_BUFFER_QUALITY = 90   # src/snapshot_saver.py:160


class DeviceBackend(_capi.Handle):
    """One rtd_jpeg handle.  A test may hand JpegEncoder another object with encode / wait_stream / close (tests/jpeg_ref.py
    RefBackend).

    Safe to share between threads (one SnapshotSaver serves every camera's thread, and the MJPEG loop runs on another): the library
    serialises the calls on a handle, and `_lock` keeps a call and the copy out of the shared output array together, so that no other
    thread's call can overwrite or replace the array in between."""

    _prefix, _what = "rtd_jpeg", "the JPEG encoder"

    def __init__(self, device: int):
        self._out = np.empty(1 << 20, np.uint8)
        self._lock = threading.Lock()
        self._open(int(device))

    def encode_raw(self, ptrs: Sequence[Optional[int]], shapes: Sequence[Sequence[int]], on_device: bool, quality: int, out: Optional[np.ndarray]):
        """rtd_jpeg_encode as it is: (return code, offsets[n + 1])"""
        n, p, hwc = _capi.c_frames(ptrs, shapes)
        offs = (C.c_int64 * (n + 1))()
        rc = self._L.rtd_jpeg_encode(self._h, n, p, hwc, int(bool(on_device)), int(quality), out.ctypes.data if out is not None else None,
                                     out.nbytes if out is not None else 0, offs)
        return rc, list(offs)

    def encode(self, frames: Sequence, on_device: bool, quality: int) -> List[bytes]:
        """frames: HxWxC uint8 (C = 1 or 3) - C-contiguous numpy arrays, or contiguous device tensors when on_device."""
        ptrs, shapes = _capi.frame_ptrs(frames, on_device)
        with self._lock:                       # the call, a retry with a larger array and the copy out of it: one critical section
            rc, offs = self.encode_raw(ptrs, shapes, on_device, quality, self._out)
            if rc == _capi.RTD_E_INVALID and len(frames) and offs[-1] > self._out.nbytes:  # too small: the needed size came back
                self._out = np.empty(max(offs[-1], 2 * self._out.nbytes), np.uint8)
                rc, offs = self.encode_raw(ptrs, shapes, on_device, quality, self._out)
            if rc != _capi.RTD_OK:
                self._raise(rc)
            return [self._out[offs[i]:offs[i + 1]].tobytes() for i in range(len(frames))]

    def coefficients(self) -> np.ndarray:
        """int16 [blocks][64] of the last call (rtd_debug_jpeg_coefficients; a test aid: "the last call" is the caller's own only
        while no other thread encodes)"""
        count = C.c_int64()
        self._check(self._L.rtd_debug_jpeg_coefficients(self._h, None, 0, C.byref(count)))
        out = np.zeros(count.value, np.int16)
        self._check(self._L.rtd_debug_jpeg_coefficients(self._h, out.ctypes.data, out.size, C.byref(count)))
        return out.reshape(-1, 64)


class JpegEncoder:
    """Baseline JPEG files of uint8 frames, encoded on the GPU.  `backend` is the only seam: an object with encode / wait_stream
    (DeviceBackend by default)."""

    def __init__(self, device=None, backend=None):
        self.device = _device_index(device)
        self._backend = backend if backend is not None else DeviceBackend(self.device)

    def encode(self, frame, quality: int = DEFAULT_QUALITY) -> bytes:
        return self.encode_batch([frame], quality)[0]

    def encode_batch(self, frames: Sequence, quality: int = DEFAULT_QUALITY) -> List[bytes]:
        q = int(quality)
        if not 1 <= q <= 100:
            raise ValueError(f"quality must be in 1..100, got {quality}")
        if not len(frames):
            return []
        conv = [_as_hwc(f) for f in frames]
        on_dev = [d for _, d in conv]
        arrs = [a for a, _ in conv]
        if any(on_dev) and not all(on_dev):            # one residency per call: mixed batches go through the host
            arrs = [a.cpu().numpy() if d else a for a, d in zip(arrs, on_dev)]
            on_dev = [False] * len(arrs)
        device = bool(on_dev[0])
        if device:
            import torch
            # the frames were written on torch's current stream; the encoder's own stream waits for that work (an event of the library)
            self._backend.wait_stream(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        return self._backend.encode(arrs, device, q)

    def close(self) -> None:
        self._backend.close()


_encoders: Dict[int, JpegEncoder] = {}
_encoders_lock = threading.Lock()


def default_encoder(device=None) -> JpegEncoder:
    """the process-wide encoder of a device (imencode and install use it)"""
    idx = _device_index(device)
    with _encoders_lock:                       # camera threads and the MJPEG loop may ask at the same moment: one handle per device
        if idx not in _encoders:
            _encoders[idx] = JpegEncoder(idx)
        return _encoders[idx]


def _is_device_tensor(frame) -> bool:
    return bool(getattr(frame, "is_cuda", False))


def imencode(ext: str, frame, params=None, encoder: Optional[JpegEncoder] = None):
    """cv2.imencode for '.jpg' / '.jpeg': (True, 1-D uint8 array).  params: [IMWRITE_JPEG_QUALITY, q] (default 95).  Device tensors are
    encoded where they are.  Any other extension or parameter goes to cv2.imencode when cv2 is importable; ValueError otherwise."""
    plist = [int(p) for p in (params if params is not None else [])]
    ours = str(ext).lower() in (".jpg", ".jpeg") and len(plist) % 2 == 0 and all(k == IMWRITE_JPEG_QUALITY for k in plist[0::2])
    if not ours:
        try:
            import cv2
        except ImportError:
            raise ValueError(f"imencode({ext!r}, params={params!r}): only '.jpg' / '.jpeg' with IMWRITE_JPEG_QUALITY is encoded here "
                             "and cv2 is not importable") from None
        if _is_device_tensor(frame):
            frame = frame.cpu().numpy()
        return cv2.imencode(ext, frame, params if params is not None else [])
    quality = plist[-1] if plist else DEFAULT_QUALITY
    quality = min(max(quality, 0), 100) or 1          # OpenCV clamps to 0..100; libjpeg turns 0 into 1
    if encoder is None:
        encoder = default_encoder(frame.device if _is_device_tensor(frame) else None)
    return True, np.frombuffer(encoder.encode(frame, quality), np.uint8)


def install(snapshot_saver_module, encoder: Optional[JpegEncoder] = None) -> None:
    """Let the reference's SnapshotSaver keep device frames on the device, without editing it:

        import src.snapshot_saver as ss, telescope_cam_detection_amd.jpeg as j
        j.install(ss)

    add_frame_to_buffer then encodes a device tensor with the library (quality 90, as the reference) and applies the reference's
    ring-buffer bookkeeping to the bytes; numpy frames and use_compressed_buffer = False go to the original method.  One saver is
    shared by every camera's thread: the encode runs outside `buffer_lock` (the encoder serialises its own calls and hands each caller
    its own bytes), so a camera that appends does not wait for another camera's encode."""
    cls = snapshot_saver_module.SnapshotSaver
    original = getattr(cls, "_rtd_original_add_frame_to_buffer", None) or cls.add_frame_to_buffer
    max_mb = getattr(snapshot_saver_module, "MAX_BUFFER_MEMORY_MB", float("inf"))

    def add_frame_to_buffer(self, frame, timestamp):
        if frame is None:
            return
        if not _is_device_tensor(frame) or not self.use_compressed_buffer:
            return original(self, frame, timestamp)
        enc = encoder if encoder is not None else default_encoder(frame.device)
        encoded = np.frombuffer(enc.encode(frame, SNAPSHOT_BUFFER_QUALITY), np.uint8)
        with self.buffer_lock:
            if len(self.frame_buffer) == self.frame_buffer.maxlen:          # the oldest entry is about to be evicted
                self.buffer_memory_bytes -= self._estimate_frame_size(self.frame_buffer[0])
            entry = {"frame_compressed": encoded, "timestamp": timestamp}
            self.frame_buffer.append(entry)
            self.buffer_memory_bytes += self._estimate_frame_size(entry)
            self.estimated_buffer_memory_mb = self.buffer_memory_bytes / (1024 * 1024)
            if self.estimated_buffer_memory_mb > max_mb:
                logger.warning(f"Frame buffer using {self.estimated_buffer_memory_mb:.1f}MB (max recommended: {max_mb}MB). "
                               f"Consider reducing pre_buffer_seconds or fps.")

    cls._rtd_original_add_frame_to_buffer = original
    cls.add_frame_to_buffer = add_frame_to_buffer
