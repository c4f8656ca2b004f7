"""Frame ingest: 4:2:0 camera frames (NV12, NV21, I420: what a video decoder writes, 1.5 bytes per pixel) to the BGR device frames
every other part of this package takes - the conversion swscale does on a CPU core behind the reference's `cv2.VideoCapture`
(src/stream_capture.py) and behind `-pix_fmt bgr24` in src/stream_capture_gpu_ffmpeg.py.

The conversion runs on the GPU (csrc/ingest.hip, rtd_ingest_* in include/rtdetr_mi355.h), all frames of a call in one launch, and is
OpenCV's COLOR_YUV2BGR_NV12 / _NV21 / _I420 integer arithmetic bit for bit (restated in tests/yuv_ref.py), with two deliberate
deviations: odd widths and heights are accepted (the chroma plane then has ceil(H/2) x ceil(W/2) samples, as ffmpeg
writes it; OpenCV refuses such frames), and the matrix and range can be chosen per frame (OpenCV knows BT.601 limited only, which is
also swscale's choice for a stream without colour tags and the default here).

* `frame_bytes(h, w)`: the size of a tightly packed frame, what one read from an ffmpeg `-f rawvideo -pix_fmt nv12` pipe must return.
* `FrameIngest(device=None)`: `to_bgr(frames, sizes, layout="nv12", matrix="bt601", full_range=False, out=None)`.
* capture.py holds the camera class that feeds it.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _capi

LAYOUTS = {"nv12": 0, "nv21": 1, "i420": 2}          # RTD_YUV_*
MATRICES = {"bt601": 0, "bt709": 1}
MAX_FRAMES = 64                                      # RTD_INGEST_MAX_FRAMES


def chroma_hw(h: int, w: int) -> Tuple[int, int]:
    return (int(h) + 1) // 2, (int(w) + 1) // 2


def frame_bytes(h: int, w: int) -> int:
    """bytes of one tightly packed 4:2:0 frame of h x w pixels (any of the three layouts): h w of luma and two chroma planes of
    ceil(h/2) x ceil(w/2)"""
    ch, cw = chroma_hw(h, w)
    return int(h) * int(w) + 2 * ch * cw


def tight_frame(base: int, h: int, w: int, layout: int, matrix: int = 0, full_range: int = 0) -> _capi.RtdYuvFrame:
    """the rtd_yuv_frame of a tightly packed frame whose first byte is at address `base`"""
    ch, cw = chroma_hw(h, w)
    f = _capi.RtdYuvFrame()
    f.y, f.u = base, base + h * w
    f.v = None if layout != LAYOUTS["i420"] else base + h * w + ch * cw
    f.width, f.height, f.y_pitch = w, h, w
    f.c_pitch = cw if layout == LAYOUTS["i420"] else 2 * cw
    f.layout, f.matrix, f.full_range = layout, matrix, full_range
    return f


def _per_frame(value, n: int, table: Optional[dict], what: str) -> List[int]:
    vals = [value] * n if isinstance(value, (str, bool, int)) else list(value)
    if len(vals) != n:
        raise ValueError(f"{len(vals)} {what} values for {n} frames")
    if table is None:
        return [int(bool(v)) for v in vals]
    try:
        return [v if isinstance(v, int) else table[str(v).lower()] for v in vals]
    except KeyError as e:
        raise ValueError(f"unknown {what} {e.args[0]!r} ({' | '.join(table)})") from None


class FrameIngest(_capi.Handle):
    """One rtd_ingest handle.  Safe to share between camera threads: the library serialises the calls on a handle."""

    _prefix, _what = "rtd_ingest", "the frame ingest"

    def __init__(self, device=None):
        self.device = _capi.device_index(device)
        self._open(self.device)

    def convert_raw(self, descs: Sequence[_capi.RtdYuvFrame], on_device: bool, out_ptrs: Sequence[Optional[int]], n: Optional[int] = None) -> int:
        """rtd_ingest_convert as it is: the return code"""
        k = len(descs)
        arr = (_capi.RtdYuvFrame * max(k, 1))(*descs)
        outs = (C.c_void_p * max(len(out_ptrs), 1))(*out_ptrs)
        return self._L.rtd_ingest_convert(self._h, k if n is None else int(n), arr, int(bool(on_device)), outs)

    def to_bgr(self, frames: Sequence, sizes: Sequence[Tuple[int, int]], layout="nv12", matrix="bt601", full_range=False,
               out: Optional[Sequence] = None) -> List:
        """frames: one tightly packed 4:2:0 frame each, as flat `bytes`, a numpy array or a host tensor, or - all of them - as uint8
        device tensors; sizes: (h, w) per frame; layout, matrix, full_range: one value, or one per frame.  Returns one [h, w, 3] uint8
        BGR device tensor per frame: the tensors of `out` (device, uint8, contiguous, of that shape) where given, new ones otherwise.
        Device frames, and the memory of the outputs, are ordered after torch's current stream; the outputs are complete on return."""
        import torch

        n = len(frames)
        if len(sizes) != n:
            raise ValueError(f"{n} frames but {len(sizes)} sizes")
        if out is not None and len(out) != n:
            raise ValueError(f"{n} frames but {len(out)} outputs")
        if n == 0:
            return []
        if n > MAX_FRAMES:                                       # the library's limit per call
            sub = lambda v, i: v if isinstance(v, (str, bool, int)) else v[i:i + MAX_FRAMES]
            return [o for i in range(0, n, MAX_FRAMES)
                    for o in self.to_bgr(frames[i:i + MAX_FRAMES], sizes[i:i + MAX_FRAMES], sub(layout, i), sub(matrix, i), sub(full_range, i),
                                         None if out is None else out[i:i + MAX_FRAMES])]
        lay, mat, rng = _per_frame(layout, n, LAYOUTS, "layout"), _per_frame(matrix, n, MATRICES, "matrix"), _per_frame(full_range, n, None, "range")
        on_dev = [bool(getattr(f, "is_cuda", False)) for f in frames]
        if any(on_dev) and not all(on_dev):
            raise ValueError("the frames of one call are all host memory or all device memory")
        dev = torch.device("cuda", self.device)
        keep, descs = [], []
        for i, f in enumerate(frames):
            h, w = int(sizes[i][0]), int(sizes[i][1])
            if on_dev[i]:
                flat = f.reshape(-1)
                if flat.dtype != torch.uint8 or not flat.is_contiguous():
                    raise ValueError(f"frame {i}: device frames are contiguous uint8 tensors")
                nbytes, base = flat.numel(), flat.data_ptr()
            else:
                if hasattr(f, "numpy") and not isinstance(f, np.ndarray):     # a host tensor
                    f = f.numpy()
                flat = np.frombuffer(f, np.uint8) if isinstance(f, (bytes, bytearray, memoryview)) else np.ascontiguousarray(f, np.uint8).reshape(-1)
                nbytes, base = flat.size, flat.ctypes.data
            if nbytes != frame_bytes(h, w):
                raise ValueError(f"frame {i}: {nbytes} bytes, but a {h} x {w} frame has {frame_bytes(h, w)}")
            keep.append(flat)
            descs.append(tight_frame(base, h, w, lay[i], mat[i], rng[i]))
        if out is None:
            outs = [torch.empty((int(h), int(w), 3), dtype=torch.uint8, device=dev) for h, w in sizes]
        else:
            outs = list(out)
            for i, o in enumerate(outs):
                if not (o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and tuple(o.shape) == (int(sizes[i][0]), int(sizes[i][1]), 3)):
                    raise ValueError(f"out[{i}] must be a contiguous uint8 device tensor of shape ({sizes[i][0]}, {sizes[i][1]}, 3)")
        # device frames were written, and the outputs' memory was last used, on torch's current stream: the handle's stream waits for it
        self.wait_stream(torch.cuda.current_stream(dev).cuda_stream)
        self._check(self.convert_raw(descs, on_dev[0], [o.data_ptr() for o in outs]))
        return outs


def tables(matrix: int, full_range: int) -> List[int]:
    """the constants CY, CVR, CVG, CUG, CUB the kernel uses for a matrix and range (rtd_debug_ingest_info; no GPU needed)"""
    c = (C.c_int32 * 5)()
    rc = _capi.lib().rtd_debug_ingest_info(int(matrix), int(full_range), c, None, None, 0, None, None)
    if rc != _capi.RTD_OK:
        raise _capi.RtdError(rc, "unknown matrix or range")
    return list(c)


def tile_hw() -> Tuple[int, int]:
    """(height, width) in pixels of what one workgroup of the kernel converts (rtd_debug_ingest_info)"""
    th, tw = C.c_int32(), C.c_int32()
    rc = _capi.lib().rtd_debug_ingest_info(0, 0, None, C.byref(th), C.byref(tw), 0, None, None)
    assert rc == _capi.RTD_OK, rc
    return th.value, tw.value
