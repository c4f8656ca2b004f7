"""Numpy restatement of the reference's face masks (src/face_masker.py FaceMasker.apply_mask and its four _apply_* methods) on 8-bit BGR
frames, as OpenCV 4.x computes them.  cv2 is not a dependency of this project, so the arithmetic of `GaussianBlur(region, (k, k), 0)`,
`resize(..., INTER_LINEAR)`, `resize(..., INTER_NEAREST)` and `rectangle(..., -1)` is written out here in int64.  This file is the
definition: the device masks (csrc/facemask.hip) must equal it byte for byte.

* Padded rectangle: p = int(w * 0.2); x1 = max(0, x - p), y1 = max(0, y - p), x2 = min(W, x + w + p), y2 = min(H, y + h + p); the region is
  frame[y1:y2, x1:x2].  An empty one is skipped (cv2 would raise; a negative x2 or y2 would even index from the far edge).
* gaussian_blur: the fixed-point path of tests/motion_ref.py (taps in 1/256, 16-bit row sums, (sum + 32768) >> 16), per channel, with
  BORDER_REFLECT_101 at the REGION's edges: the slice reaches cv2 as a Mat of its own.  `taps` here has no 63-tap limit (k <= 99).
* adaptive_blur: the same with k = min(99, odd(int(blur_strength * (1 + w h / (H W) * 10)))).
* black_box: cv2.rectangle fills both corners: zero over x1..min(x2, W - 1), y1..min(y2, H - 1) inclusive.
* pixelate: small = resize(region, (max(1, rw // blocks), max(1, rh // blocks)), INTER_LINEAR); resize(small, (rw, rh), INTER_NEAREST).
  imgproc/src/resize.cpp, the portable 8-bit code, function by function in `resize_linear` and `resize_nearest` below.

Points that could not be checked against cv2 here (it is not installed; where it is, tests/test_face_masker_host.py compares): everything
tests/motion_ref.py lists for the blur; that the resize restatement (written from memory of resize.cpp) is cv2's; and whether a cv2
build with IPP or another HAL takes the portable resize path at all."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

from tests.motion_ref import FIXED_TABLES, _gauss, reflect101

MAX_K = 99
STYLES = ("gaussian_blur", "pixelate", "black_box", "adaptive_blur")
PADDING = 0.2


def taps(k: int, margins=None) -> np.ndarray:
    """motion_ref.taps without its 63-tap limit: the taps of a k x k GaussianBlur(sigma = 0) in units of 1/256, odd k in 1..99"""
    k = int(k)
    if not (1 <= k <= MAX_K and k % 2 == 1):
        raise ValueError(f"k must be odd and in 1..{MAX_K}, got {k}")
    if k in FIXED_TABLES:
        return np.array(FIXED_TABLES[k], np.int64)
    g = _gauss(k)
    c = [0] * k
    err = 0.0
    for i in range(k // 2):
        adj = 256.0 * g[i] + err
        v = int(round(adj))                     # half to even, like cvRound
        if margins is not None:
            margins.append(abs(adj - math.floor(adj) - 0.5))
        err = adj - v
        c[i] = c[k - 1 - i] = v
    c[k // 2] = 256 - 2 * sum(c[: k // 2])
    return np.array(c, np.int64)


def padded_rect(face, H: int, W: int) -> Tuple[int, int, int, int]:
    """x1, y1, x2, y2 of the padded face rectangle, ends exclusive (it may be empty)"""
    x, y, w, h = (int(v) for v in face)
    p = int(w * PADDING)
    return max(0, x - p), max(0, y - p), min(W, x + w + p), min(H, y + h + p)


def is_empty(rect) -> bool:
    return rect[2] <= rect[0] or rect[3] <= rect[1]


def adaptive_k(blur_strength: int, face, H: int, W: int) -> int:
    x, y, w, h = (int(v) for v in face)
    k = int(blur_strength * (1 + (w * h) / (H * W) * 10))
    k = k if k % 2 == 1 else k + 1
    return min(99, k)


def blur_region(region: np.ndarray, k: int) -> np.ndarray:
    """GaussianBlur(region, (k, k), 0) of an h x w x 3 uint8 region that is a Mat of its own"""
    c = taps(k)
    r = k // 2
    h, w = region.shape[:2]
    v = region.astype(np.int64)
    vp = v[:, reflect101(np.arange(-r, w + r), w)]
    R = np.zeros_like(v)
    for j in range(k):
        R += c[j] * vp[:, j:j + w]
    Rp = R[reflect101(np.arange(-r, h + r), h)]
    acc = np.zeros_like(v)
    for i in range(k):
        acc += c[i] * Rp[i:i + h]
    return ((acc + 32768) >> 16).astype(np.uint8)


# ---- resize ---------------------------------------------------------------------------------------------------------------------------
def _scale(ssize: int, dsize: int) -> float:
    """cv::resize: inv_scale = (double)dsize / ssize; hal::resize: scale = 1. / inv_scale"""
    return 1.0 / (dsize / ssize)


def _cv_round(v: float) -> int:
    return int(round(v))                        # half to even


def is_area2(rw: int, rh: int, sw: int, sh: int) -> bool:
    """hal::resize: INTER_LINEAR is INTER_AREA's 2 x 2 mean when is_area_fast && iscale_x == 2 && iscale_y == 2"""
    sx, sy = _scale(rw, sw), _scale(rh, sh)
    ix, iy = _cv_round(sx), _cv_round(sy)
    eps = np.finfo(np.float64).eps
    return abs(sx - ix) < eps and abs(sy - iy) < eps and ix == 2 and iy == 2


def linear_table(ssize: int, dsize: int, columns: bool):
    """resizeGeneric_'s table loop: per output sample (i0, i1, w0, w1).  fx = (float)((dx + 0.5) * scale - 0.5) from a double product,
    sx = cvFloor(fx), fx -= sx in float; columns: sx < 0 -> fx = 0, sx = 0; sx >= ssize - 1 -> fx = 0, sx = ssize - 1 (HResizeLinear's
    S[sx] * ONE beyond xmax is then S[i0] * 2048 + S[i1] * 0); rows keep fx, and resizeGeneric_Invoker clips both row indices.
    Weights: saturate_cast<short>((1.f - fx) * 2048) and (fx * 2048), cvRound in float."""
    scale = _scale(ssize, dsize)
    out = []
    for d in range(dsize):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if columns:
            if s < 0:
                f, s = np.float32(0), 0
            if s >= ssize - 1:
                f, s = np.float32(0), ssize - 1
            s1 = min(s + 1, ssize - 1)
        else:
            s1 = min(max(s + 1, 0), ssize - 1)
            s = min(max(s, 0), ssize - 1)
        w0 = int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048)))
        w1 = int(np.rint(f * np.float32(2048)))
        out.append((s, s1, w0, w1))
    return out


def resize_linear(region: np.ndarray, sw: int, sh: int) -> np.ndarray:
    rh, rw = region.shape[:2]
    v = region.astype(np.int64)
    if is_area2(rw, rh, sw, sh):
        # ResizeAreaFast_Invoker at scale 2: (a + b + c + d + 2) >> 2
        return ((v[0:2 * sh:2, 0:2 * sw:2] + v[0:2 * sh:2, 1:2 * sw:2] + v[1:2 * sh:2, 0:2 * sw:2] + v[1:2 * sh:2, 1:2 * sw:2] + 2) >> 2).astype(np.uint8)
    xs, ys = linear_table(rw, sw, True), linear_table(rh, sh, False)
    x0, x1, a0, a1 = (np.array(col, np.int64) for col in zip(*xs))
    # HResizeLinear<uchar, int, short, 2048>
    S = v[:, x0] * a0[None, :, None] + v[:, x1] * a1[None, :, None]
    out = np.zeros((sh, sw, v.shape[2]), np.int64)
    for dy, (y0, y1, b0, b1) in enumerate(ys):
        # VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>
        out[dy] = (((b0 * (S[y0] >> 4)) >> 16) + ((b1 * (S[y1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def nearest_table(ssize: int, dsize: int) -> np.ndarray:
    """resizeNN: x_ofs[x] = min(cvFloor(x * ifx), ssize - 1), ifx = 1. / ((double)dsize / ssize)"""
    ifx = 1.0 / (dsize / ssize)
    return np.array([min(int(math.floor(x * ifx)), ssize - 1) for x in range(dsize)], np.int64)


def resize_nearest(small: np.ndarray, rw: int, rh: int) -> np.ndarray:
    sh, sw = small.shape[:2]
    return small[nearest_table(sh, rh)][:, nearest_table(sw, rw)]


def pixelate_region(region: np.ndarray, blocks: int) -> np.ndarray:
    rh, rw = region.shape[:2]
    small = resize_linear(region, max(1, rw // blocks), max(1, rh // blocks))
    return resize_nearest(small, rw, rh)


# ---- the four styles, in place on `frame`, and the reference's loop ----------------------------------------------------------------------
def apply_face(frame: np.ndarray, face, style: str, blur_strength: int = 25, pixelate_blocks: int = 10) -> None:
    H, W = frame.shape[:2]
    x1, y1, x2, y2 = rect = padded_rect(face, H, W)
    if is_empty(rect):
        return
    if style == "black_box":
        frame[y1:min(y2, H - 1) + 1, x1:min(x2, W - 1) + 1] = 0
    elif style == "pixelate":
        frame[y1:y2, x1:x2] = pixelate_region(frame[y1:y2, x1:x2], pixelate_blocks)
    elif style == "adaptive_blur":
        frame[y1:y2, x1:x2] = blur_region(frame[y1:y2, x1:x2], adaptive_k(blur_strength, face, H, W))
    else:
        frame[y1:y2, x1:x2] = blur_region(frame[y1:y2, x1:x2], blur_strength)


def apply_mask(frame: np.ndarray, faces: Sequence, style: str = "gaussian_blur", blur_strength: int = 25, pixelate_blocks: int = 10) -> np.ndarray:
    """FaceMasker.apply_mask: a masked copy, the faces applied one after another; `style` one name, or one per face"""
    out = np.array(frame, np.uint8, copy=True)
    styles = [style] * len(faces) if isinstance(style, str) else list(style)
    for face, st in zip(faces, styles):
        apply_face(out, face, st, blur_strength, pixelate_blocks)
    return out


def layers(faces: Sequence, styles: Sequence[str], H: int, W: int) -> List[int]:
    """the layer of every face of ONE frame (-1: skipped): the first layer after every earlier face it meets"""
    out, rects = [], []
    for face, st in zip(faces, styles):
        x1, y1, x2, y2 = r = padded_rect(face, H, W)
        if is_empty(r):
            out.append(-1)
            rects.append(None)
            continue
        if st == "black_box":
            x2, y2 = min(x2 + 1, W), min(y2 + 1, H)
        layer = 0
        for o, l in zip(rects, out):
            if o is not None and x1 < o[2] and o[0] < x2 and y1 < o[3] and o[1] < y2:
                layer = max(layer, l + 1)
        out.append(layer)
        rects.append((x1, y1, x2, y2))
    return out


def noise(seed: int, h: int, w: int) -> np.ndarray:
    """a seeded noise frame (smooth content hides off-by-one taps)"""
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a
