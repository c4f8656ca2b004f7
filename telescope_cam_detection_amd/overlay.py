"""Detection overlays for device-resident frames: the reference's `WebServer._draw_detections` (src/web_server.py, the MJPEG loop) and
`visualization_utils.draw_detections` (the annotated snapshot of src/detection_processor.py), without the copy of the raw frame to the
host.  With the JPEG encoder (jpeg.py) an MJPEG tick is: device frame, draw, encode - only the compressed bytes cross PCIe.

Three layers:

* plan      `plan_web` / `plan_snapshot`: pure Python, detections -> the reference's own cv2 call sequence as a list of events
            ('rect', (x1, y1), (x2, y2), bgr, thickness) and ('text', text, (x, y), scale, bgr, thickness, aa), event for event
            (tests/golden/overlay_calls.json holds the calls the reference makes, recorded by tools/make_overlay_golden.py).
* rasteriser the only place that knows a font: `size(text, scale, thickness) -> ((w, h), baseline)` as cv2.getTextSize, and
            `mask(text, scale, thickness, aa) -> (uint8 coverage HxW, dx, dy)` with dx, dy relative to cv2's text origin (the bottom-left
            of the text).  A few hundred bytes per distinct label, kept in a host LRU (`MaskCache`).  `Cv2Rasteriser` asks cv2 itself, so
            LINE_8 text (the web overlay) is cv2's own pixels by construction; `PillowRasteriser` uses Pillow's built-in FreeType font
            where cv2 is absent.
* renderer  csrc/overlay.hip (rtd_overlay_* in include/rtdetr_mi355.h): the primitives of a whole batch of frames in one launch,
            bit-identical to tests/overlay_ref.py.

Deliberate deviations from cv2's pixels: an outline of thickness t >= 2 has square corners (cv2 draws four thick lines
with round caps), and LINE_AA text is one coverage mask blended as out = (bg (255 - a) + colour a + 127) / 255, where cv2 blends stroke by
stroke.

`OverlayRenderer(device=None, rasteriser=None, backend=None)`: `draw_batch`, `draw_detections` (the reference's call shape), `web_draw`,
`mjpeg_tick` (one overlay call and one JpegEncoder.encode_batch call for all cameras), and `install(detection_processor_module)`.
"""
from __future__ import annotations

import ctypes as C
import threading
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from .jpeg import _device_index, _is_device_tensor
from .motion import _as_hwc

FILL, OUTLINE, MASK = 0, 1, 2                       # RTD_OVL_*
MAX_FRAMES, MAX_PRIMS = 64, 4096                    # RTD_OVERLAY_MAX_*
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("thickness", "<i4"),
                       ("bgr", "u1", 3), ("reserved0", "u1"), ("mask_offset", "<i8")], align=True)      # rtd_overlay_prim
assert PRIM_DTYPE.itemsize == 40

# src/web_server.py _draw_detections
WEB_PERSON, WEB_ANIMAL, WEB_OTHER = (0, 0, 255), (0, 165, 255), (0, 255, 0)
WEB_ANIMALS = ("cat", "dog", "bird")
# src/visualization_utils.py CLASS_COLORS / DEFAULT_COLOR (BGR)
CLASS_COLORS = {"person": (0, 102, 255), "bird": (0, 170, 255), "cat": (255, 68, 255), "dog": (255, 187, 68), "horse": (147, 20, 255),
                "sheep": (0, 215, 255), "cow": (114, 128, 250), "elephant": (170, 178, 32), "bear": (45, 82, 160), "zebra": (128, 128, 128),
                "giraffe": (0, 255, 255)}
DEFAULT_COLOR = (0, 255, 136)
WHITE = (255, 255, 255)


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def _corners(bbox) -> Tuple[int, int, int, int]:
    return int(bbox["x1"]), int(bbox["y1"]), int(bbox["x2"]), int(bbox["y2"])


def plan_web(detection_result: Dict[str, Any], rasteriser) -> List[tuple]:
    """WebServer._draw_detections: per detection an outline of thickness 2 in the class's colour, a filled bar sized by the label and the
    label in white (scale 0.5, thickness 2, LINE_8); then the latency line at (10, 30), scale 0.7, green."""
    plan: List[tuple] = []
    for det in detection_result.get("detections", []):
        x1, y1, x2, y2 = _corners(det["bbox"])
        name = det["class_name"]
        colour = WEB_PERSON if name == "person" else WEB_ANIMAL if name in WEB_ANIMALS else WEB_OTHER
        plan.append(("rect", (x1, y1), (x2, y2), colour, 2))
        label = f"{name}: {det['confidence']:.2f}"
        (w, h), _ = rasteriser.size(label, 0.5, 2)
        plan.append(("rect", (x1, y1 - h - 10), (x1 + w, y1), colour, -1))
        plan.append(("text", label, (x1, y1 - 5), 0.5, WHITE, 2, False))
    latency_ms = detection_result.get("total_latency_ms", 0)
    plan.append(("text", f"Latency: {latency_ms:.0f}ms", (10, 30), 0.7, (0, 255, 0), 2, False))
    return plan


def plan_snapshot(detections: Sequence[Dict[str, Any]], thickness: int = 3, font_scale: float = 0.7, draw_labels: bool = True,
                  rasteriser=None) -> List[tuple]:
    """visualization_utils.draw_detections: per detection an outline in the palette colour of the class; with labels, the species label
    (with its taxonomic level unless that is "species") or the class label, a bar that includes the baseline, above the box unless
    there is no room, and the label in white, anti-aliased, thickness 2."""
    plan: List[tuple] = []
    for det in detections:
        x1, y1, x2, y2 = _corners(det["bbox"])
        name = det["class_name"]
        colour = CLASS_COLORS.get(name.lower(), DEFAULT_COLOR)
        plan.append(("rect", (x1, y1), (x2, y2), colour, thickness))
        if not draw_labels:
            continue
        species, sconf, level = det.get("species"), det.get("species_confidence"), det.get("taxonomic_level")
        if species is not None and sconf is not None:
            label = f"{species} ({level}) {sconf:.2f}" if level and level != "species" else f"{species} {sconf:.2f}"
        else:
            label = f"{name} {det['confidence']:.2f}"
        (w, h), base = rasteriser.size(label, font_scale, 2)
        label_y = y1 - 10 if y1 - 10 > h else y1 + h + 10
        plan.append(("rect", (x1, label_y - h - base), (x1 + w, label_y + base), colour, -1))
        plan.append(("text", label, (x1, label_y - base), font_scale, WHITE, 2, True))
    return plan


# ---- rasterisers ----------------------------------------------------------------------------------------------------------------------
class Cv2Rasteriser:
    """cv2's own text: putText in white on a black one-channel canvas sized from getTextSize, cropped to what was drawn.  With LINE_8
    the coverage is 0 or 255, so text drawn through it is exactly cv2's.  `cv2` may be handed in (a test's stand-in)."""

    def __init__(self, cv2=None):
        if cv2 is None:
            import cv2
        self.cv2 = cv2

    def size(self, text: str, scale: float, thickness: int):
        (w, h), base = self.cv2.getTextSize(text, self.cv2.FONT_HERSHEY_SIMPLEX, scale, thickness)
        return (int(w), int(h)), int(base)

    def mask(self, text: str, scale: float, thickness: int, aa: bool):
        cv2 = self.cv2
        (w, h), base = self.size(text, scale, thickness)
        pad = thickness + 2                                     # strokes and the anti-aliasing fringe reach past the text box
        canvas = np.zeros((h + base + 2 * pad, w + 2 * pad), np.uint8)
        ox, oy = pad, pad + h                                   # the text origin: bottom-left of the text
        cv2.putText(canvas, text, (ox, oy), cv2.FONT_HERSHEY_SIMPLEX, scale, 255, thickness, cv2.LINE_AA if aa else cv2.LINE_8)
        ys, xs = np.nonzero(canvas)
        if not len(ys):
            return np.zeros((0, 0), np.uint8), 0, 0
        y0, y1, x0, x1 = int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())
        return np.ascontiguousarray(canvas[y0:y1 + 1, x0:x1 + 1]), x0 - ox, y0 - oy


class PillowRasteriser:
    """Pillow's built-in FreeType font where cv2 is absent: not Hershey's glyphs, but the same places and sizes.  The pixel size is
    32 x scale (Hershey Simplex is about 22 pixels from baseline to cap at scale 1, as this font at 32); a thickness above 2 widens
    the strokes.  The mask is the whole text box of `size`: w x (h + baseline), its top-left at (0, -h) from the text origin."""

    def __init__(self):
        from PIL import Image, ImageDraw, ImageFont
        self._Image, self._ImageDraw, self._ImageFont = Image, ImageDraw, ImageFont
        self._fonts: Dict[int, Any] = {}

    def _font(self, scale: float):
        px = max(int(round(32 * scale)), 6)
        if px not in self._fonts:
            self._fonts[px] = self._ImageFont.load_default(size=px)
        return self._fonts[px]

    @staticmethod
    def _stroke(thickness: int) -> int:
        return max((int(thickness) - 1) // 2, 0)

    def size(self, text: str, scale: float, thickness: int):
        font, s = self._font(scale), self._stroke(thickness)
        ascent, descent = font.getmetrics()
        return (int(np.ceil(font.getlength(text))) + 2 * s, ascent + s), descent + s

    def mask(self, text: str, scale: float, thickness: int, aa: bool):
        (w, h), base = self.size(text, scale, thickness)
        if w <= 0:
            return np.zeros((0, 0), np.uint8), 0, 0
        font, s = self._font(scale), self._stroke(thickness)
        im = self._Image.new("L", (w, h + base), 0)
        self._ImageDraw.Draw(im).text((s, h), text, fill=255, font=font, anchor="ls", stroke_width=s)
        m = np.asarray(im, np.uint8)
        if not aa:
            m = np.where(m >= 128, 255, 0).astype(np.uint8)
        return np.ascontiguousarray(m), 0, -h


def default_rasteriser():
    """cv2 where it is importable (the deployment: its text is then the reference's), Pillow otherwise"""
    try:
        import cv2  # noqa: F401
    except ImportError:
        return PillowRasteriser()
    return Cv2Rasteriser()


class MaskCache:
    """host LRU of rasterised labels, keyed by (text, scale, thickness, aa): a label's mask is made once while it stays in use"""

    def __init__(self, rasteriser, capacity: int = 512):
        self.rasteriser = rasteriser
        self.capacity = int(capacity)
        self.hits = self.misses = 0
        self._d: "OrderedDict[tuple, tuple]" = OrderedDict()
        self._lock = threading.Lock()

    def get(self, text: str, scale: float, thickness: int, aa: bool):
        key = (text, float(scale), int(thickness), bool(aa))
        with self._lock:
            if key in self._d:
                self._d.move_to_end(key)
                self.hits += 1
                return self._d[key]
        m, dx, dy = self.rasteriser.mask(text, scale, thickness, aa)
        val = (np.ascontiguousarray(m, np.uint8), int(dx), int(dy))
        with self._lock:
            self.misses += 1
            self._d[key] = val
            self._d.move_to_end(key)
            while len(self._d) > self.capacity:
                self._d.popitem(last=False)
        return val

    def __len__(self):
        return len(self._d)


def lower(plans: Sequence[Sequence[tuple]], cache: MaskCache):
    """plans (one event list per frame) -> (one rtd_overlay_prim array per frame, the mask bytes they index).  A label that occurs more
    than once in the call is stored once."""
    chunks: List[np.ndarray] = []
    where: Dict[int, int] = {}
    nbytes = 0
    out = []
    for plan in plans:
        prims = np.zeros(len(plan), PRIM_DTYPE)
        k = 0
        for ev in plan:
            p = prims[k]
            if ev[0] == "rect":
                _, (x1, y1), (x2, y2), bgr, t = ev
                if t == 0:
                    raise ValueError("a rectangle's thickness is >= 1, or negative for a filled one")
                p["kind"], p["thickness"] = (FILL, 0) if t < 0 else (OUTLINE, int(t))
                p["x1"], p["y1"], p["x2"], p["y2"] = int(x1), int(y1), int(x2), int(y2)
            elif ev[0] == "text":
                _, text, (x, y), scale, bgr, t, aa = ev
                m, dx, dy = cache.get(text, scale, t, aa)
                if m.size == 0:
                    continue
                if id(m) not in where:
                    where[id(m)] = nbytes
                    chunks.append(m.reshape(-1))
                    nbytes += m.size
                p["kind"], p["mask_offset"] = MASK, where[id(m)]
                p["x1"], p["y1"], p["x2"], p["y2"] = int(x) + dx, int(y) + dy, m.shape[1], m.shape[0]
            else:
                raise ValueError(f"unknown plan event {ev[0]!r}")
            p["bgr"] = [int(v) for v in (bgr if not np.isscalar(bgr) else (bgr, bgr, bgr))]
            k += 1
        out.append(prims[:k])
    masks = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    return out, np.ascontiguousarray(masks, np.uint8)


# ---- backends -------------------------------------------------------------------------------------------------------------------------
class DeviceBackend(_capi.Handle):
    """One rtd_overlay handle.  A test may hand OverlayRenderer another object with draw / wait_stream / close (tests/overlay_ref.py
    RefBackend).  Safe to share between threads: the library serialises the calls on a handle."""

    _prefix, _what = "rtd_overlay", "the overlay renderer"

    def __init__(self, device: int):
        self.device = int(device)
        self._open(self.device)

    def draw_raw(self, ptrs: Sequence[Optional[int]], shapes: Sequence[Sequence[int]], on_device: bool, prims: Sequence[np.ndarray],
                 masks: np.ndarray, out_ptrs: Sequence[Optional[int]]) -> int:
        """rtd_overlay_draw as it is: the return code"""
        n, p, hwc = _capi.c_frames(ptrs, shapes)
        o = (C.c_void_p * max(n, 1))(*out_ptrs)
        counts = (C.c_int32 * max(n, 1))(*[len(a) for a in prims])
        flat = np.ascontiguousarray(np.concatenate(list(prims)) if len(prims) else np.zeros(0, PRIM_DTYPE), PRIM_DTYPE)
        masks = np.ascontiguousarray(masks, np.uint8)
        return self._L.rtd_overlay_draw(self._h, n, p, hwc, int(bool(on_device)), counts, flat.ctypes.data if flat.size else None,
                                        masks.ctypes.data if masks.size else None, masks.size, o)

    def draw(self, frames: Sequence, on_device: bool, prims: Sequence[np.ndarray], masks: np.ndarray, inplace: bool) -> List:
        """frames: HxWxC uint8 - C-contiguous numpy arrays, or contiguous device tensors when on_device.  Returns device tensors: the
        frames themselves when inplace (device frames only), new ones otherwise."""
        import torch
        if inplace and not on_device:
            raise ValueError("only device frames are drawn in place")
        dev = torch.device("cuda", self.device)
        outs = list(frames) if inplace else [torch.empty(tuple(f.shape), dtype=torch.uint8, device=dev) for f in frames]
        # the frames were written, and the new tensors' memory was last used, on torch's current stream: the handle's stream waits for it
        self.wait_stream(torch.cuda.current_stream(dev).cuda_stream)
        ptrs, shapes = _capi.frame_ptrs(frames, on_device)
        self._check(self.draw_raw(ptrs, shapes, on_device, prims, masks, [o.data_ptr() for o in outs]))
        return outs

    def tiles(self) -> Tuple[int, int, int]:
        """(tile height, tile width, tiles the last draw launched): rtd_debug_overlay_tiles"""
        th, tw, n = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._L.rtd_debug_overlay_tiles(self._h, C.byref(th), C.byref(tw), C.byref(n)))
        return th.value, tw.value, n.value


# ---- the renderer ---------------------------------------------------------------------------------------------------------------------
class OverlayRenderer:
    """Overlays drawn on the GPU.  `rasteriser` is the font seam (default_rasteriser() by default), `backend` the device seam
    (DeviceBackend by default); `encoder` is the JpegEncoder of mjpeg_tick (the process-wide one of the device by default)."""

    def __init__(self, device=None, rasteriser=None, backend=None, encoder=None):
        self.device = _device_index(device)
        self.rasteriser = rasteriser if rasteriser is not None else default_rasteriser()
        self.cache = MaskCache(self.rasteriser)
        self._backend = backend if backend is not None else DeviceBackend(self.device)
        self._encoder = encoder

    def draw_batch(self, frames: Sequence, plans: Sequence[Sequence[tuple]], inplace: bool = False) -> List:
        """One overlay call for all frames (numpy arrays, host tensors or device tensors; HxW or HxWxC uint8, C = 1 or 3 = BGR) with one
        plan each.  Returns one HxWxC device tensor per frame: new tensors, or with `inplace` the device frames themselves (host frames
        are uploaded first and the uploaded copies are drawn on).  Device frames are ordered after torch's current stream."""
        if len(frames) != len(plans):
            raise ValueError(f"{len(frames)} frames but {len(plans)} plans")
        if not len(frames):
            return []
        if len(frames) > MAX_FRAMES:                             # the library's limit per call
            return [o for i in range(0, len(frames), MAX_FRAMES) for o in self.draw_batch(frames[i:i + MAX_FRAMES], plans[i:i + MAX_FRAMES], inplace)]
        conv = [_as_hwc(f) for f in frames]
        arrs, on_dev = [a for a, _ in conv], [d for _, d in conv]
        prims, masks = lower(plans, self.cache)
        if any(on_dev) and not all(on_dev):                      # one residency per call: the host frames of a mixed batch are uploaded
            import torch
            dev = torch.device("cuda", self.device)
            arrs = [a if d else torch.from_numpy(a).to(dev) for a, d in zip(arrs, on_dev)]
            on_dev = [True] * len(arrs)
        device = bool(on_dev[0])
        return self._backend.draw(arrs, device, prims, masks, bool(inplace) and device)

    def draw_detections(self, frame, detections, thickness: int = 3, font_scale: float = 0.7, draw_labels: bool = True):
        """visualization_utils.draw_detections: an annotated copy of the frame.  A device tensor comes back for a device frame (the
        reference's save_snapshot converts tensors; with jpeg.install they stay on the device), a numpy array for a host frame."""
        plan = plan_snapshot(detections, thickness, font_scale, draw_labels, rasteriser=self.rasteriser)
        out = self.draw_batch([frame], [plan])[0]
        if not _is_device_tensor(frame) and hasattr(out, "cpu"):
            out = out.cpu().numpy()
        return out.reshape(tuple(frame.shape))

    def web_draw(self, frame, detection_result: Dict[str, Any]):
        """WebServer._draw_detections of one frame: an annotated copy on the device"""
        return self.draw_batch([frame], [plan_web(detection_result, self.rasteriser)])[0]

    def mjpeg_tick(self, frames: Sequence, detection_results: Sequence[Optional[Dict[str, Any]]], quality: int) -> List[bytes]:
        """One MJPEG tick for all cameras: the web overlay of every frame in one overlay call (a camera without detections yet, None,
        is encoded as it is, as the reference does), then one JpegEncoder.encode_batch call.  Only the JPEG bytes reach the host."""
        if len(frames) != len(detection_results):
            raise ValueError(f"{len(frames)} frames but {len(detection_results)} detection results")
        plans = [plan_web(r, self.rasteriser) if r is not None else [] for r in detection_results]
        drawn = self.draw_batch(frames, plans)
        if self._encoder is None:
            from .jpeg import default_encoder
            self._encoder = default_encoder(self.device)
        return self._encoder.encode_batch(drawn, quality)

    def close(self) -> None:
        self._backend.close()


_renderers: Dict[int, OverlayRenderer] = {}
_renderers_lock = threading.Lock()


def default_renderer(device=None) -> OverlayRenderer:
    """the process-wide renderer of a device (install uses it)"""
    idx = _device_index(device)
    with _renderers_lock:
        if idx not in _renderers:
            _renderers[idx] = OverlayRenderer(idx)
        return _renderers[idx]


def install(detection_processor_module, renderer: Optional[OverlayRenderer] = None) -> None:
    """Let the reference's DetectionProcessor annotate device frames on the device, without editing it:

        import src.detection_processor as dp, telescope_cam_detection_amd.overlay as ov
        ov.install(dp)

    The module's `draw_detections` (bound by `from visualization_utils import draw_detections`) is replaced: a device tensor is
    annotated by the library and comes back as a device tensor; a numpy frame goes to the original function."""
    original = getattr(detection_processor_module, "_rtd_original_draw_detections", None) or detection_processor_module.draw_detections

    def draw_detections(frame, detections, thickness: int = 3, font_scale: float = 0.7, draw_labels: bool = True):
        if not _is_device_tensor(frame):
            return original(frame, detections, thickness, font_scale, draw_labels)
        r = renderer if renderer is not None else default_renderer(frame.device)
        return r.draw_detections(frame, detections, thickness, font_scale, draw_labels)

    detection_processor_module._rtd_original_draw_detections = original
    detection_processor_module.draw_detections = draw_detections
