"""Privacy face masking for device-resident frames: the reference's `FaceMasker` / `FaceMaskingCache` (src/face_masker.py) and the live
feed's `WebServer._apply_face_masking_to_frame` (src/web_server.py), without the copy of the frame to the host.  With the overlay
renderer and the JPEG encoder an MJPEG tick of a masked camera is: device frame, mask, draw, encode - only a gray plane (every `ttl`
frames, for the face detector) and the compressed bytes cross PCIe.

* masks     csrc/facemask.hip (rtd_facemask_* in include/rtdetr_mi355.h): the four mask styles on the padded face rectangle, byte for
            byte what cv2 does to the numpy frame (restated in tests/face_ref.py).  numpy frames go through the same kernels.
* detection stays a host call: cv2's Haar cascade (or `detector=`, any callable gray ndarray -> [(x, y, w, h)]) on the gray plane the
            gray kernel writes into pinned host memory.  No face detector runs on the GPU.

`FaceMasker(...)` has the reference's constructor plus `device=None, detector=None`, and its methods `detect_faces`, `apply_mask`,
`detect_and_mask`; `apply_mask_batch` masks a tick's cameras in one library call.  `FaceMaskingCache` is the reference's.
`mask_frame(masker, cache, frame, camera_id)` is the decision flow of `_apply_face_masking_to_frame`, and `install(web_server)` puts it
behind that method for device frames.

Deliberate deviations: a face whose padded rectangle is empty is skipped (cv2 raises); frames are contiguous
[H, W, 3] uint8; k is at most 99 and blocks at least 1; without cv2 and without `detector` the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from .jpeg import _is_device_tensor

logger = logging.getLogger(__name__)

BLUR, PIXELATE, BLACK_BOX = 0, 1, 2                 # RTD_FACE_*
MAX_FRAMES, MAX_FACES, MAX_K = 64, 1024, 99         # RTD_FACEMASK_MAX_*
STYLES = ("gaussian_blur", "pixelate", "black_box", "adaptive_blur")
BACKENDS = ("opencv_haar", "mediapipe")
Face = Tuple[int, int, int, int]


def _cv2():
    try:
        import cv2
        return cv2
    except ImportError:
        return None


def gray_plane(frame: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(frame, COLOR_BGR2GRAY) of a host frame in integers, where cv2 is absent"""
    b, g, r = (frame[:, :, c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def check_frame(frame, what: str = "frame") -> None:
    """anything but a contiguous [H, W, 3] uint8 frame (numpy array or device tensor) raises ValueError"""
    if _is_device_tensor(frame):
        import torch
        ok = frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3 and frame.is_contiguous()
    else:
        ok = isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and frame.flags["C_CONTIGUOUS"]
    if not ok:
        raise ValueError(f"{what} must be a contiguous [H, W, 3] uint8 numpy array or device tensor")


class DeviceBackend(_capi.Handle):
    """One rtd_facemask handle.  Safe to share between threads: the library serialises the calls on a handle."""

    _prefix, _what = "rtd_facemask", "the face masker"

    def __init__(self, device: int):
        self.device = int(device)
        self._open(self.device)

    def apply_raw(self, ptrs: Sequence[Optional[int]], shapes: Sequence[Sequence[int]], on_device: bool, faces: Sequence[Sequence[int]],
                  n: Optional[int] = None, n_faces: Optional[int] = None) -> int:
        """rtd_facemask_apply as it is: the return code.  faces: rows of (frame, x, y, w, h, style, k_or_blocks)"""
        k = len(ptrs)
        p = (C.c_void_p * max(k, 1))(*ptrs)
        hw = (C.c_int32 * max(2 * k, 1))(*[int(v) for s in shapes for v in s[:2]])
        arr = (_capi.RtdFaceRect * max(len(faces), 1))(*[_capi.RtdFaceRect(*[int(v) for v in f], 0) for f in faces])
        return self._L.rtd_facemask_apply(self._h, k if n is None else int(n), p, hw, int(bool(on_device)),
                                          len(faces) if n_faces is None else int(n_faces), arr)

    def apply(self, frames: Sequence, on_device: bool, faces: Sequence[Sequence[int]]) -> None:
        """masks the frames IN PLACE: contiguous device tensors (ordered after torch's current stream), or C-contiguous numpy arrays"""
        if on_device:
            import torch
            self.wait_stream(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        ptrs, shapes = _capi.frame_ptrs(frames, on_device)
        self._check(self.apply_raw(ptrs, shapes, on_device, faces))

    def gray(self, frame) -> np.ndarray:
        """the gray plane of one device frame as a host array (rtd_facemask_gray), ordered after torch's current stream"""
        import torch
        h, w = int(frame.shape[0]), int(frame.shape[1])
        out = np.empty((h, w), np.uint8)
        self.wait_stream(torch.cuda.current_stream(frame.device).cuda_stream)
        self._check(self._L.rtd_facemask_gray(self._h, C.c_void_p(frame.data_ptr()), h, w, C.c_void_p(out.ctypes.data)))
        return out


def plan(shapes: Sequence[Sequence[int]], faces: Sequence[Sequence[int]]) -> Dict:
    """what the library would do with a call (rtd_debug_facemask_plan; no GPU needed): {'layers', 'layer_of', 'rects', 'tile', 'tiles'};
    raises RtdError for what rtd_facemask_apply would refuse"""
    L = _capi.lib()
    n, nf = len(shapes), len(faces)
    hw = (C.c_int32 * max(2 * n, 1))(*[int(v) for s in shapes for v in s[:2]])
    arr = (_capi.RtdFaceRect * max(nf, 1))(*[_capi.RtdFaceRect(*[int(v) for v in f], 0) for f in faces])
    layers, th, tw = C.c_int32(), C.c_int32(), C.c_int32()
    layer_of, rects, tiles = (C.c_int32 * max(nf, 1))(), (C.c_int32 * max(4 * nf, 1))(), (C.c_int64 * 5)()
    rc = L.rtd_debug_facemask_plan(n, hw, nf, arr, C.byref(layers), layer_of, rects, C.byref(th), C.byref(tw), tiles, 0, None)
    if rc != _capi.RTD_OK:
        raise _capi.RtdError(rc, (L.rtd_facemask_last_error(None) or b"").decode(errors="replace"))
    return {"layers": layers.value, "layer_of": list(layer_of)[:nf], "rects": [tuple(rects[4 * i:4 * i + 4]) for i in range(nf)],
            "tile": (th.value, tw.value), "tiles": dict(zip(("blur_rows", "blur_cols", "pix_small", "pix_nearest", "box"), tiles))}


def taps(k: int) -> List[int]:
    """the taps of a k-tap blur as the library makes them (the rule of csrc/gauss_taps.h; no GPU needed)"""
    L = _capi.lib()
    out = (C.c_uint16 * max(int(k), 1))()
    rc = L.rtd_debug_facemask_plan(0, None, 0, None, None, None, None, None, None, None, int(k), out)
    if rc != _capi.RTD_OK:
        raise _capi.RtdError(rc, (L.rtd_facemask_last_error(None) or b"").decode(errors="replace"))
    return list(out)


def adaptive_k(blur_strength: int, w: int, h: int, H: int, W: int) -> int:
    """the kernel size of adaptive_blur for a w x h face on an H x W frame, in Python's arithmetic as the reference works it out"""
    k = int(blur_strength * (1 + (w * h) / (H * W) * 10))
    k = k if k % 2 == 1 else k + 1
    return min(99, k)


class FaceMasker:
    """The reference's FaceMasker with its masks on the GPU.  `device`: where host frames are masked and the default for device frames
    (None: torch's current device); `detector`: gray ndarray -> [(x, y, w, h)], in place of cv2's Haar cascade."""

    FACE_PADDING_PERCENT = 0.2          # (the library pads by int(w * 0.2) itself)

    def __init__(self, detection_backend: str = "opencv_haar", mask_style: str = "gaussian_blur", min_face_size: int = 30, blur_strength: int = 25,
                 pixelate_blocks: int = 10, scale_factor: float = 1.1, min_neighbors: int = 5, device=None,
                 detector: Optional[Callable[[np.ndarray], Sequence[Face]]] = None):
        self.detection_backend = detection_backend
        self.mask_style = mask_style
        self.min_face_size = min_face_size
        if blur_strength <= 0:
            raise ValueError(f"blur_strength must be positive, got {blur_strength}")
        if blur_strength % 2 == 0:
            logger.warning("blur_strength must be odd, got %d; using %d", blur_strength, blur_strength + 1)
            blur_strength += 1
        self.blur_strength = blur_strength
        self.pixelate_blocks = pixelate_blocks
        self.scale_factor = scale_factor
        self.min_neighbors = min_neighbors
        self.device = device
        self.detector = detector
        self._backends: Dict[int, DeviceBackend] = {}
        if detection_backend == "mediapipe":
            self._init_mediapipe()
        else:
            if detection_backend == "yolox":
                logger.warning("the yolox face backend does not exist yet; using opencv_haar")
            elif detection_backend != "opencv_haar":
                logger.error("unknown detection backend %r; using opencv_haar", detection_backend)
            self.detection_backend = "opencv_haar"
            self._init_opencv_haar()
        logger.info("FaceMasker: backend=%s, style=%s, min_size=%s", self.detection_backend, self.mask_style, self.min_face_size)

    # ---- detection (host)
    def _init_opencv_haar(self) -> None:
        self.face_cascade = None
        if self.detector is not None:
            return
        cv2 = _cv2()
        if cv2 is None:
            raise RuntimeError("FaceMasker needs cv2 for its Haar cascade, or a `detector` callable (gray ndarray -> [(x, y, w, h)])")
        path = cv2.data.haarcascades + "haarcascade_frontalface_default.xml"
        self.face_cascade = cv2.CascadeClassifier(path)
        if self.face_cascade.empty():
            raise ValueError(f"could not load the Haar cascade {path}")

    def _init_mediapipe(self) -> None:
        try:
            import mediapipe as mp
            self.mp_face_detection = mp.solutions.face_detection
            self.face_detector = self.mp_face_detection.FaceDetection(model_selection=0, min_detection_confidence=0.5)
        except Exception as e:                     # not installed, or it would not start: the reference falls back as well
            logger.error("MediaPipe is not usable (%s); using opencv_haar", e)
            self.detection_backend = "opencv_haar"
            self._init_opencv_haar()

    def _backend(self, frame=None) -> DeviceBackend:
        idx = _capi.device_index(frame.device if frame is not None and _is_device_tensor(frame) else self.device)
        if idx not in self._backends:
            self._backends[idx] = DeviceBackend(idx)
        return self._backends[idx]

    def _faces_in_gray(self, gray: np.ndarray) -> List[Face]:
        if self.detector is not None:
            found = self.detector(gray)
        else:
            found = self.face_cascade.detectMultiScale(gray, scaleFactor=self.scale_factor, minNeighbors=self.min_neighbors,
                                                       minSize=(self.min_face_size, self.min_face_size))
        return [(int(x), int(y), int(w), int(h)) for (x, y, w, h) in found]

    def _detect_mediapipe(self, frame: np.ndarray) -> List[Face]:
        cv2 = _cv2()
        rgb = cv2.cvtColor(frame, cv2.COLOR_BGR2RGB) if cv2 is not None else np.ascontiguousarray(frame[:, :, ::-1])
        results = self.face_detector.process(rgb)
        faces: List[Face] = []
        H, W = frame.shape[:2]
        for det in results.detections or []:
            box = det.location_data.relative_bounding_box
            x, y, w, h = int(box.xmin * W), int(box.ymin * H), int(box.width * W), int(box.height * H)
            if w >= self.min_face_size and h >= self.min_face_size:
                faces.append((x, y, w, h))
        return faces

    def detect_faces(self, frame) -> List[Face]:
        """(x, y, w, h) of every face.  A device frame sends its gray plane to the host detector (a third of its bytes, no colour
        conversion on the CPU); mediapipe takes the downloaded frame."""
        check_frame(frame)
        on_device = _is_device_tensor(frame)
        if self.detection_backend == "mediapipe":
            return self._detect_mediapipe(frame.cpu().numpy() if on_device else frame)
        if on_device:
            gray = self._backend(frame).gray(frame)
        else:
            cv2 = _cv2()
            gray = cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY) if cv2 is not None else gray_plane(frame)
        return self._faces_in_gray(gray)

    # ---- masking (device)
    def _face_rows(self, index: int, shape, faces: Sequence[Face], style: str) -> List[Tuple[int, ...]]:
        if style not in STYLES:
            logger.warning("unknown mask style %r; using gaussian_blur", style)
            style = "gaussian_blur"
        H, W = int(shape[0]), int(shape[1])
        rows = []
        for (x, y, w, h) in faces:
            x, y, w, h = int(x), int(y), int(w), int(h)
            if style == "black_box":
                rows.append((index, x, y, w, h, BLACK_BOX, 0))
            elif style == "pixelate":
                rows.append((index, x, y, w, h, PIXELATE, int(self.pixelate_blocks)))
            elif style == "adaptive_blur":
                rows.append((index, x, y, w, h, BLUR, adaptive_k(self.blur_strength, w, h, H, W)))
            else:
                rows.append((index, x, y, w, h, BLUR, int(self.blur_strength)))
        return rows

    def apply_mask_batch(self, frames: Sequence, faces_per_frame: Sequence[Sequence[Face]], mask_style: Optional[str] = None) -> List:
        """apply_mask for a tick's cameras in ONE library call (more than 64 frames or 1024 faces: one call per such chunk).  The frames
        are all device tensors or all numpy arrays; a frame without faces comes back as the object it is."""
        if len(frames) != len(faces_per_frame):
            raise ValueError(f"{len(frames)} frames but {len(faces_per_frame)} face lists")
        for i, f in enumerate(frames):
            check_frame(f, f"frame {i}")
        on_dev = [_is_device_tensor(f) for f in frames]
        if any(on_dev) and not all(on_dev):
            raise ValueError("the frames of one call are all host memory or all device memory")
        style = mask_style or self.mask_style
        out = list(frames)
        todo = [i for i, faces in enumerate(faces_per_frame) if len(faces)]
        if not todo:
            return out
        device = bool(on_dev[todo[0]])
        for i in todo:                                         # the reference's frame.copy(): the input stays as it is
            out[i] = frames[i].clone() if device else frames[i].copy()
        chunk, rows = [], []

        def flush():
            if chunk:
                self._backend(out[chunk[0]]).apply([out[i] for i in chunk], device, rows)
            chunk.clear()
            rows.clear()

        for i in todo:
            faces = list(faces_per_frame[i])
            for at in range(0, len(faces), MAX_FACES):         # (a frame with more faces than a call takes: the calls follow each other)
                part = faces[at:at + MAX_FACES]
                same_device = not chunk or not device or out[chunk[0]].device == out[i].device
                if len(chunk) >= MAX_FRAMES or len(rows) + len(part) > MAX_FACES or not same_device:
                    flush()
                if not chunk or chunk[-1] != i:
                    chunk.append(i)
                rows.extend(self._face_rows(len(chunk) - 1, out[i].shape, part, style))
        flush()
        return out

    def apply_mask(self, frame, faces: Sequence[Face], mask_style: Optional[str] = None):
        """A masked copy of the frame: a new device tensor for a device tensor (the call is ordered after torch's current stream and
        complete on return), a numpy array for a numpy array (through the same kernels).  Without faces: the frame itself."""
        if not len(faces):
            return frame
        return self.apply_mask_batch([frame], [faces], mask_style)[0]

    def detect_and_mask(self, frame, mask_style: Optional[str] = None):
        faces = self.detect_faces(frame)
        return self.apply_mask(frame, faces, mask_style), faces

    def close(self) -> None:
        for b in self._backends.values():
            b.close()
        self._backends.clear()


class FaceMaskingCache:
    """Face positions per camera, reused for `ttl_frames` frames between two detections (the reference's class, call for call)."""

    def __init__(self, ttl_frames: int = 5):
        self.cache: Dict[str, Tuple[List[Face], int]] = {}
        self.ttl = ttl_frames

    def should_detect(self, camera_id: str) -> bool:
        return camera_id not in self.cache or self.cache[camera_id][1] >= self.ttl

    def get_cached_faces(self, camera_id: str) -> Optional[List[Face]]:
        return self.cache[camera_id][0] if camera_id in self.cache else None

    def update_cache(self, camera_id: str, faces: List[Face]) -> None:
        self.cache[camera_id] = (faces, 0)

    def increment_frame_count(self, camera_id: str) -> None:
        if camera_id in self.cache:
            faces, count = self.cache[camera_id]
            self.cache[camera_id] = (faces, count + 1)

    def clear_cache(self, camera_id: Optional[str] = None) -> None:
        if camera_id is None:
            self.cache.clear()
        else:
            self.cache.pop(camera_id, None)


def mask_frame(masker, cache, frame, camera_id: str):
    """The decision flow of WebServer._apply_face_masking_to_frame on any frame `masker` takes (a device tensor stays on the device):
    detect when the cache says so (or there is none), otherwise reuse the cached faces and count the frame; mask when there are faces.
    On ANY exception the unmasked frame comes back, as in the reference."""
    if not masker:
        return frame
    try:
        if cache and cache.should_detect(camera_id):
            faces = masker.detect_faces(frame)
            cache.update_cache(camera_id, faces)
        elif cache:
            faces = cache.get_cached_faces(camera_id)
            cache.increment_frame_count(camera_id)
        else:
            faces = masker.detect_faces(frame)
        return masker.apply_mask(frame, faces) if faces else frame
    except Exception as e:
        logger.error("face masking failed for camera %s: %s", camera_id, e)
        return frame


def from_reference(masker, device=None) -> FaceMasker:
    """a FaceMasker with the settings (and the loaded cascade) of a reference FaceMasker"""
    cascade = getattr(masker, "face_cascade", None)
    detector = None
    if cascade is not None:
        def detector(gray):
            return cascade.detectMultiScale(gray, scaleFactor=masker.scale_factor, minNeighbors=masker.min_neighbors,
                                            minSize=(masker.min_face_size, masker.min_face_size))
    return FaceMasker(masker.detection_backend, masker.mask_style, masker.min_face_size, masker.blur_strength, masker.pixelate_blocks,
                      masker.scale_factor, masker.min_neighbors, device=device, detector=detector)


def install(web_server) -> None:
    """Let the reference's WebServer mask device frames on the device, without editing it:

        import telescope_cam_detection_amd.face_masker as fm
        fm.install(web_server)            # an instance, or the WebServer class

    `_apply_face_masking_to_frame` is replaced: a device tensor goes through `mask_frame` (after the reference's own per-camera switch
    `_is_face_masking_enabled_for_camera`), with the server's masker if it is this module's FaceMasker and otherwise with one made
    from its settings; a numpy frame goes to the original method."""
    cls = web_server if isinstance(web_server, type) else type(web_server)
    original = getattr(cls, "_rtd_original_apply_face_masking", None) or cls._apply_face_masking_to_frame

    def _apply_face_masking_to_frame(self, frame, camera_id):
        if not _is_device_tensor(frame):
            return original(self, frame, camera_id)
        if not self._is_face_masking_enabled_for_camera(camera_id) or not self.face_masker:
            return frame
        masker = self.face_masker
        if not isinstance(masker, FaceMasker):
            if getattr(self, "_rtd_face_masker_of", None) is not masker:
                try:
                    self._rtd_face_masker, self._rtd_face_masker_of = from_reference(masker), masker
                except Exception as e:                         # as any failure inside the reference's method: the unmasked frame
                    logger.error("face masking failed for camera %s: %s", camera_id, e)
                    return frame
            masker = self._rtd_face_masker
        return mask_frame(masker, getattr(self, "face_masking_cache", None), frame, camera_id)

    cls._rtd_original_apply_face_masking = original
    cls._apply_face_masking_to_frame = _apply_face_masking_to_frame
