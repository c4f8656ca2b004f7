"""Restatement of the overlay renderer (csrc/overlay.hip, rtd_overlay_draw) in numpy: what its bytes must equal, with the pieces the
overlay tests share.

Pixel rules (include/rtdetr_mi355.h), primitives in list order, clipped to the frame:
  FILL     every pixel of the inclusive rectangle between the two corners (any order)
  OUTLINE  o = t // 2, i = (t - 1) // 2: the pixels of [x1-o, x2+o] x [y1-o, y2+o] not strictly inside (x1+i, x2-i) x (y1+i, y2-i)
  MASK     out = (bg * (255 - a) + colour * a + 127) // 255 per channel; a = 0 keeps the pixel, a = 255 replaces it
One-channel frames take bgr[0].

Also here: `tiles_touched` (the tiles a call has to launch: an OUTLINE counts as its four strips), `RefBackend` (the compositor behind
overlay.OverlayRenderer's backend seam), `FakeRasteriser` (the metric rule of tests/golden/overlay_calls.json with seeded per-character
masks over 0..255) and `RecordingCv2` (a stand-in cv2 module that records rectangle / getTextSize / putText calls).
"""
from __future__ import annotations

import json
import os
import zlib
from typing import List, Sequence, Tuple

import numpy as np

from telescope_cam_detection_amd.overlay import FILL, MASK, OUTLINE, PRIM_DTYPE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay_calls.json")
METRIC = {"char_w": 18, "cap_h": 22, "base": 9}      # the declared fake metric rule (also written into the fixture)


def text_size(text: str, scale: float, thickness: int, metric=METRIC):
    """w = int(len * char_w * scale + 0.5), h = int(cap_h * scale + 0.5), baseline = int(base * scale + 0.5) + thickness // 2"""
    w = int(len(text) * metric["char_w"] * scale + 0.5)
    h = int(metric["cap_h"] * scale + 0.5)
    return (w, h), int(metric["base"] * scale + 0.5) + int(thickness) // 2


def prim(kind, x1, y1, x2, y2, bgr=(0, 0, 0), thickness=0, mask_offset=0) -> np.ndarray:
    p = np.zeros(1, PRIM_DTYPE)
    p["kind"], p["x1"], p["y1"], p["x2"], p["y2"], p["thickness"], p["mask_offset"] = kind, x1, y1, x2, y2, thickness, mask_offset
    p["bgr"] = bgr
    return p


def prims(*items) -> np.ndarray:
    return np.concatenate(items) if items else np.zeros(0, PRIM_DTYPE)


def _boxes(p):
    """(outer box, hole) of a FILL / OUTLINE, inclusive, unclipped; the hole is None when empty"""
    xl, xh = sorted((int(p["x1"]), int(p["x2"])))
    yl, yh = sorted((int(p["y1"]), int(p["y2"])))
    if int(p["kind"]) == FILL:
        return (xl, yl, xh, yh), None
    t = int(p["thickness"])
    o, i = t // 2, (t - 1) // 2
    hole = (xl + i + 1, yl + i + 1, xh - i - 1, yh - i - 1)
    return (xl - o, yl - o, xh + o, yh + o), (hole if hole[0] <= hole[2] and hole[1] <= hole[3] else None)


def _clip(box, H, W):
    x0, y0, x1, y1 = max(box[0], 0), max(box[1], 0), min(box[2], W - 1), min(box[3], H - 1)
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else None


def composite(frame: np.ndarray, prim_list: np.ndarray, masks: np.ndarray) -> np.ndarray:
    """a new HxWxC frame with the primitives applied"""
    a = np.array(frame, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    H, W, C = a.shape
    for p in prim_list:
        col = np.array(p["bgr"][:C], np.uint8)
        if int(p["kind"]) == MASK:
            w, h = int(p["x2"]), int(p["y2"])
            x0, y0 = int(p["x1"]), int(p["y1"])
            c = _clip((x0, y0, x0 + w - 1, y0 + h - 1), H, W)
            if w <= 0 or h <= 0 or c is None:
                continue
            m = masks[int(p["mask_offset"]):int(p["mask_offset"]) + w * h].reshape(h, w)
            cov = m[c[1] - y0:c[3] - y0 + 1, c[0] - x0:c[2] - x0 + 1].astype(np.uint32)[:, :, None]
            bg = a[c[1]:c[3] + 1, c[0]:c[2] + 1].astype(np.uint32)
            a[c[1]:c[3] + 1, c[0]:c[2] + 1] = ((bg * (255 - cov) + col.astype(np.uint32) * cov + 127) // 255).astype(np.uint8)
            continue
        outer, hole = _boxes(p)
        c = _clip(outer, H, W)
        if c is None:
            continue
        paint = np.ones((c[3] - c[1] + 1, c[2] - c[0] + 1), bool)
        hc = _clip(hole, H, W) if hole else None
        if hc:
            paint[hc[1] - c[1]:hc[3] - c[1] + 1, hc[0] - c[0]:hc[2] - c[0] + 1] = False
        a[c[1]:c[3] + 1, c[0]:c[2] + 1][paint] = col
    return a


def tiles_touched(prim_list: np.ndarray, hwc: Sequence[int], tile: Tuple[int, int]) -> int:
    """how many (tile_h, tile_w) tiles of an H x W frame some primitive paints: FILL its rectangle, MASK its whole box, OUTLINE its
    four strips (top, bottom, left, right), each clipped to the frame"""
    H, W = int(hwc[0]), int(hwc[1])
    th, tw = tile
    marks = np.zeros(((H + th - 1) // th, (W + tw - 1) // tw), bool)

    def mark(box):
        c = _clip(box, H, W)
        if c:
            marks[c[1] // th:c[3] // th + 1, c[0] // tw:c[2] // tw + 1] = True

    for p in prim_list:
        if int(p["kind"]) == MASK:
            mark((int(p["x1"]), int(p["y1"]), int(p["x1"]) + int(p["x2"]) - 1, int(p["y1"]) + int(p["y2"]) - 1))
            continue
        o, h = _boxes(p)
        if h is None:
            mark(o)
        else:
            mark((o[0], o[1], o[2], h[1] - 1))
            mark((o[0], h[3] + 1, o[2], o[3]))
            mark((o[0], h[1], h[0] - 1, h[3]))
            mark((h[2] + 1, h[1], o[2], h[3]))
    return int(marks.sum())


class RefBackend:
    """the compositor behind overlay.OverlayRenderer's backend seam: draw(frames, on_device, prims, masks, inplace) -> numpy frames"""

    def __init__(self):
        self.calls: List[Tuple[int, bool, bool]] = []
        self.waits = 0

    def draw(self, frames, on_device: bool, prim_lists, masks, inplace: bool):
        self.calls.append((len(frames), bool(on_device), bool(inplace)))
        outs = []
        for f, pl in zip(frames, prim_lists):
            r = composite(f, pl, masks)
            if inplace:
                f[...] = r
                r = f
            outs.append(r)
        return outs

    def wait_stream(self, producer_stream: int) -> None:
        self.waits += 1

    def close(self) -> None:
        pass


class FakeRasteriser:
    """no font: the fixture's metric rule for sizes, and for masks one seeded block of values over 0..255 per character (255 and 0 both
    occur), char_w * scale wide and h + baseline tall, with its top-left at (0, -h) from the text origin"""

    def __init__(self, metric=METRIC):
        self.metric = dict(metric)
        self.mask_calls = 0

    def size(self, text, scale, thickness):
        return text_size(text, scale, thickness, self.metric)

    def mask(self, text, scale, thickness, aa):
        self.mask_calls += 1
        (w, h), base = self.size(text, scale, thickness)
        m = np.zeros((h + base, w), np.uint8)
        for i, ch in enumerate(text):
            x0, x1 = int(i * self.metric["char_w"] * scale + 0.5), int((i + 1) * self.metric["char_w"] * scale + 0.5)
            rng = np.random.default_rng(zlib.crc32(f"{ch}|{scale}|{thickness}|{aa}".encode()))
            blk = rng.integers(0, 256, (h + base, x1 - x0), dtype=np.uint8)
            blk[rng.random(blk.shape) < 0.25] = 0
            blk[rng.random(blk.shape) < 0.25] = 255
            m[:, x0:x1] = blk if aa else np.where(blk >= 128, 255, 0)
        return m, 0, -h


class RecordingCv2:
    """a stand-in `cv2` module: records what is drawn as the events of overlay.plan_* ('rect' / 'text'; getTextSize answers by the
    metric rule and is listed in `size_calls`).  putText also leaves a deterministic mark on the canvas (a filled box of value
    color inside the text box, inset by 1) so that a rasteriser driven through it has something to crop."""
    FONT_HERSHEY_SIMPLEX, LINE_8, LINE_AA, IMWRITE_JPEG_QUALITY = 0, 8, 16, 1

    def __init__(self, metric=METRIC):
        self.metric = dict(metric)
        self.calls: list = []
        self.size_calls: list = []

    def rectangle(self, img, pt1, pt2, color, thickness=1, lineType=8, shift=0):
        self.calls.append(["rect", [int(pt1[0]), int(pt1[1])], [int(pt2[0]), int(pt2[1])], [int(c) for c in color], int(thickness)])
        return img

    def getTextSize(self, text, fontFace, fontScale, thickness):
        self.size_calls.append([text, fontFace, fontScale, thickness])
        return text_size(text, fontScale, thickness, self.metric)

    def putText(self, img, text, org, fontFace, fontScale, color, thickness=1, lineType=8, bottomLeftOrigin=False):
        col = [int(c) for c in color] if hasattr(color, "__len__") else [int(color)] * 3
        self.calls.append(["text", text, [int(org[0]), int(org[1])], fontScale, col, int(thickness), lineType == self.LINE_AA])
        (w, h), _ = text_size(text, fontScale, thickness, self.metric)
        if isinstance(img, np.ndarray) and img.ndim == 2 and w > 2 and h > 2:
            img[max(org[1] - h + 1, 0):org[1], org[0] + 1:org[0] + w - 1] = col[0]
        return img


def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def as_events(plan) -> list:
    """a plan of overlay.plan_* in the fixture's form (lists, as JSON stores them)"""
    return json.loads(json.dumps(plan))
