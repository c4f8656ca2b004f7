"""The restatement the ingest's resize stage (csrc/ingest.hip resize_kernel) must equal byte for byte: the conversion of tests/yuv_ref.py
followed by OpenCV's `resize(frame, (w, h))` with INTER_LINEAR on 8-bit data as tests/face_ref.py writes it out.

    out = resize_linear(to_bgr(frame), ow, oh)          (a BGR source: resize_linear(frame, ow, oh) alone)

* where `is_area2` holds (both scale factors exactly 2) the result is the 2 x 2 mean (a + b + c + d + 2) >> 2 of CONVERTED pixels: the
  conversion clamps per pixel, so averaging luma first is another function;
* otherwise the column and row tables of `linear_table` (weights in 1/2048), H = p[i0] w0 + p[i1] w1 and
  out = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2; a mixed case (one scale 2, the other not) is linear on both axes;
* the same size gives the frame back (weights 2048 / 0).

"As OpenCV" stays a restatement that cannot be checked where cv2 is not installed; tests/test_resize_host.py compares the BGR path with
cv2.resize where it is.  `forced_linear` ignores the area rule (what a kernel without it would compute), and `RefResizeIngest` is the
capture class's `ingest` seam with `out_sizes` / `native_out`, answering from this file with host tensors.
"""
import numpy as np

from tests import face_ref, yuv_ref
from tests.face_ref import is_area2, linear_table      # noqa: F401  (the two rules, for the tests that hold the library's tables to them)


def resize_bgr(frame, oh, ow):
    """[sh, sw, 3] uint8 -> [oh, ow, 3] uint8"""
    return face_ref.resize_linear(np.asarray(frame, np.uint8), int(ow), int(oh))


def to_bgr_resized(buf, h, w, oh, ow, layout="nv12", matrix="bt601", full_range=False):
    """a tightly packed 4:2:0 frame of h x w -> [oh, ow, 3] uint8 BGR"""
    return resize_bgr(yuv_ref.to_bgr(buf, h, w, layout, matrix, full_range), oh, ow)


def planes_resized(Y, U, V, oh, ow, matrix="bt601", full_range=False):
    return resize_bgr(yuv_ref.planes_to_bgr(Y, U, V, matrix, full_range), oh, ow)


def forced_linear(frame, oh, ow):
    """resize_linear's table path whatever is_area2 says"""
    v = np.asarray(frame, np.uint8).astype(np.int64)
    sh, sw = v.shape[:2]
    xs, ys = linear_table(sw, ow, True), linear_table(sh, oh, False)
    x0, x1, a0, a1 = (np.array(col, np.int64) for col in zip(*xs))
    S = v[:, x0] * a0[None, :, None] + v[:, x1] * a1[None, :, None]
    out = np.zeros((oh, ow, v.shape[2]), np.int64)
    for dy, (y0, y1, b0, b1) in enumerate(ys):
        out[dy] = (((b0 * (S[y0] >> 4)) >> 16) + ((b1 * (S[y1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def bgr(seed, h, w):
    """seeded noise [h, w, 3] (smooth content hides a wrong tap)"""
    return face_ref.noise(seed, h, w)


class RefResizeIngest(yuv_ref.RefIngest):
    """yuv_ref.RefIngest with FrameIngest's `out_sizes` and `native_out` (True only), from the restatement, with host tensors"""

    def __init__(self):
        super().__init__()
        self.kwargs = []

    def to_bgr(self, frames, sizes, layout="nv12", matrix="bt601", full_range=False, out=None, out_sizes=None, native_out=None):
        import torch
        self.kwargs.append({"sizes": list(sizes), "out_sizes": out_sizes, "native_out": native_out})
        native = super().to_bgr(frames, sizes, layout, matrix, full_range)
        if out_sizes is None:
            return native
        oh, ow = out_sizes
        resized = [torch.from_numpy(resize_bgr(f.numpy(), oh, ow)) for f in native]
        return (resized, native) if native_out else resized
