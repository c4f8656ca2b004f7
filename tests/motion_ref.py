"""Numpy restatement of the reference's empty-frame filter (src/empty_frame_filter.py) on 8-bit frames, as OpenCV 4.x computes it.

cv2 is not a dependency of this project, so the arithmetic of `cvtColor(BGR2GRAY)`, `GaussianBlur(gray, (k, k), 0)`, `absdiff`,
`threshold(..., THRESH_BINARY)` and `countNonZero` is written out here in integers.  The device filter (csrc/motion.hip) must match it
bit for bit; the tests compare the stored blurred frames and the motion areas.

* Gray (imgproc/src/color_rgb: RGB2Gray<uchar>, yuv_shift = 14): Y = (1868 B + 9617 G + 4899 R + 8192) >> 14.  A 2-D frame, or one with
  C = 1, is already gray; any other channel count is refused.
* Blur (smooth.dispatch.cpp, the fixed-point path for CV_8U; smooth.simd.hpp hlineSmooth / vlineSmooth on ufixedpoint16 / ufixedpoint32):
  taps are ufixedpoint16 (8 fractional bits).  k = 1, 3, 5, 7 with sigma = 0 take the fixed tables of getGaussianKernelBitExact:
  [256], [64, 128, 64], [16, 64, 96, 64, 16], [8, 28, 56, 72, 56, 28, 8].  Larger k: sigma = 0.15 k + 0.35, g_i = exp(-x_i^2 / (2 sigma^2))
  normalised to sum 1 in double precision, then getGaussianKernelFixedPoint_ED: walking from the outermost tap towards the centre,
  v_i = round_half_even(256 g_i + e), e = 256 g_i + e - v_i (the rounding error is carried inwards), mirrored; the centre tap is
  256 - sum(off-centre), so the taps sum to exactly 256.  Row pass R = sum_j c_j Y[x + j] (exact, units of 1/256); column pass
  out = (sum_i c_i R[y + i] + 32768) >> 16, saturated to uint8.  Borders: BORDER_REFLECT_101 through borderInterpolate's index map.
* Difference: area = #{ |blur_t - blur_{t-1}| > floor(threshold) } (THRESH_BINARY is strict; a threshold < 0 counts every pixel, >= 255 none).

Points that could not be checked against cv2 here (it is not installed; where it is, tests/test_motion_host.py compares):
1. The error-diffusion step of the tap quantisation (getGaussianKernelFixedPoint_ED) is restated from memory; `taps(k, diffuse=False)`
   is plain per-tap rounding, and tests/test_motion_host.py pins for which k the two differ.
2. OpenCV computes the Gaussian in softdouble (its own IEEE emulation, with its own exp); Python's exp may differ in the last ulp.  A tap
   whose 256 g_i + e lay within ~1e-9 of a .5 boundary could round differently; the tests pin that none of the k <= 63 kernels is that close.
3. That the SIMD paths of hlineSmooth / vlineSmooth (symmetric-kernel specialisations, v_mul_expand / v_rshr_pack) equal the scalar
   formula above.  OpenCV's own tests assert that bit-exactness across dispatch modes; it was not re-derived here.
4. That no HAL (carotene on ARM, IPP) or OpenCL path takes over GaussianBlur on 8-bit input with sigma = 0 on the deployment host.
5. That k = 1 (a plain copy in OpenCV) equals the [256] table: it does arithmetically, (256 * 256 Y + 32768) >> 16 = Y.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

MAX_BLUR = 63
FIXED_TABLES = {1: [256], 3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [8, 28, 56, 72, 56, 28, 8]}


def odd_blur(blur_size: int) -> int:
    """upstream's `blur_size if blur_size % 2 == 1 else blur_size + 1`, limited to 1..63 taps"""
    k = int(blur_size)
    k = k if k % 2 == 1 else k + 1
    if not 1 <= k <= MAX_BLUR:
        raise ValueError(f"blur_size {blur_size} gives a {k}-tap kernel: 1..{MAX_BLUR} taps are supported")
    return k


def _gauss(k: int) -> List[float]:
    sigma = 0.15 * k + 0.35
    g = [math.exp(-((i - (k - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)) for i in range(k)]
    s = sum(g)
    return [v / s for v in g]


def taps(k: int, diffuse: bool = True, margins: Optional[list] = None) -> np.ndarray:
    """Gaussian taps of a k x k GaussianBlur(sigma = 0) on 8-bit input, in units of 1/256 (int64, symmetric, sum 256).
    `margins`, when given, receives |frac(256 g_i + e) - 0.5| of every rounding (how far each tap was from a rounding tie)."""
    k = odd_blur(k)
    if k in FIXED_TABLES:
        return np.array(FIXED_TABLES[k], np.int64)
    g = _gauss(k)
    c = [0] * k
    err = 0.0
    for i in range(k // 2):
        adj = 256.0 * g[i] + (err if diffuse else 0.0)
        v = int(round(adj))                     # Python rounds half to even, like cvRound
        if margins is not None:
            margins.append(abs(adj - math.floor(adj) - 0.5))
        err = adj - v
        c[i] = c[k - 1 - i] = v
    c[k // 2] = 256 - 2 * sum(c[: k // 2])
    return np.array(c, np.int64)


def reflect101(p, n: int) -> np.ndarray:
    """borderInterpolate(p, n, BORDER_REFLECT_101): reflects repeatedly while the index is outside [0, n); n = 1 maps everything to 0."""
    p = np.array(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p = np.where(lo, -p, np.where(hi, 2 * (n - 1) - p, p))


def as_gray(frame) -> np.ndarray:
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise ValueError(f"frames must be uint8, got {a.dtype}")
    if a.ndim == 2:
        return a
    if a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"frames must be HxW or HxWxC with C = 1 or 3, got shape {a.shape}")
    if a.shape[2] == 1:
        return a[:, :, 0]
    b, g, r = (a[:, :, c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def blur(gray: np.ndarray, k: int) -> np.ndarray:
    c = taps(k)
    r = len(c) // 2
    H, W = gray.shape
    y = gray.astype(np.int64)
    yp = y[:, reflect101(np.arange(-r, W + r), W)]
    R = np.zeros((H, W), np.int64)
    for j in range(2 * r + 1):
        R += c[j] * yp[:, j:j + W]
    Rp = R[reflect101(np.arange(-r, H + r), H), :]
    acc = np.zeros((H, W), np.int64)
    for i in range(2 * r + 1):
        acc += c[i] * Rp[i:i + H, :]
    return np.clip((acc + 32768) >> 16, 0, 255).astype(np.uint8)


def blurred(frame, k: int) -> np.ndarray:
    return blur(as_gray(frame), k)


def motion_area(prev: np.ndarray, cur: np.ndarray, threshold) -> int:
    d = np.abs(prev.astype(np.int16) - cur.astype(np.int16))
    return int((d > math.floor(threshold)).sum())


class RefBackend:
    """Numpy stand-in for telescope_cam_detection_amd.motion.DeviceBackend (same methods): one stored blurred frame per slot."""

    def __init__(self, blur_size: int):
        self.k = odd_blur(blur_size)
        self.state: Dict[int, np.ndarray] = {}
        self.calls = 0

    def check(self, frames: Sequence, on_device: bool, slots: Sequence[int], threshold: int) -> List[int]:
        self.calls += 1
        out = []
        for f, s in zip(frames, slots):
            if on_device:
                f = f.cpu().numpy()
            b = blurred(f, self.k)
            prev = self.state.get(int(s))
            out.append(-1 if prev is None or prev.shape != b.shape else motion_area(prev, b, threshold))
            self.state[int(s)] = b
        return out

    def reset(self, slot: int = -1) -> None:
        if slot < 0:
            self.state.clear()
        else:
            self.state.pop(int(slot), None)

    def wait_stream(self, stream) -> None:
        pass
