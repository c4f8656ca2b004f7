"""Frame ingest: 4:2:0 camera frames (NV12, NV21, I420: what a video decoder writes, 1.5 bytes per pixel) to the BGR device frames
every other part of this package takes - the conversion swscale does on a CPU core behind the reference's `cv2.VideoCapture`
(src/stream_capture.py) and behind `-pix_fmt bgr24` in src/stream_capture_gpu_ffmpeg.py.

The conversion runs on the GPU (csrc/ingest.hip, rtd_ingest_* in include/rtdetr_mi355.h), all frames of a call in one launch, and is
OpenCV's COLOR_YUV2BGR_NV12 / _NV21 / _I420 integer arithmetic bit for bit (restated in tests/yuv_ref.py), with two deliberate
deviations: odd widths and heights are accepted (the chroma plane then has ceil(H/2) x ceil(W/2) samples, as ffmpeg
writes it; OpenCV refuses such frames), and the matrix and range can be chosen per frame (OpenCV knows BT.601 limited only, which is
also swscale's choice for a stream without colour tags and the default here).

* `frame_bytes(h, w)`: the size of a tightly packed frame, what one read from an ffmpeg `-f rawvideo -pix_fmt nv12` pipe must return.
* `FrameIngest(device=None)`: `to_bgr(frames, sizes, layout="nv12", matrix="bt601", full_range=False, out=None)`; with
  `out_sizes=` the frames come back resized as `cv2.resize(frame, (w, h))` would make them (INTER_LINEAR on 8-bit data, restated in
  tests/resize_ref.py), with `native_out=` the native frame beside them; `resize(frames, out_sizes, out=None)` for BGR frames.
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

    def resize_raw(self, descs: Sequence, on_device: bool, out_hw: Sequence[int], out_ptrs: Sequence[Optional[int]],
                   native_ptrs: Optional[Sequence[Optional[int]]] = None, n: Optional[int] = None) -> int:
        """rtd_ingest_convert_resize (descs: RtdYuvFrame) or rtd_ingest_resize (descs: RtdBgrFrame) as it is: the return code"""
        k = len(descs)
        bgr = k > 0 and isinstance(descs[0], _capi.RtdBgrFrame)
        arr = ((_capi.RtdBgrFrame if bgr else _capi.RtdYuvFrame) * max(k, 1))(*descs)
        hw = (C.c_int32 * max(len(out_hw), 1))(*[int(v) for v in out_hw])
        outs = (C.c_void_p * max(len(out_ptrs), 1))(*out_ptrs)
        if bgr:
            return self._L.rtd_ingest_resize(self._h, k if n is None else int(n), arr, int(bool(on_device)), hw, outs)
        nat = None if native_ptrs is None else (C.c_void_p * max(len(native_ptrs), 1))(*native_ptrs)
        return self._L.rtd_ingest_convert_resize(self._h, k if n is None else int(n), arr, int(bool(on_device)), hw, outs, nat)

    def to_bgr(self, frames: Sequence, sizes: Sequence[Tuple[int, int]], layout="nv12", matrix="bt601", full_range=False,
               out: Optional[Sequence] = None, out_sizes=None, native_out=None):
        """frames: one tightly packed 4:2:0 frame each, as flat `bytes`, a numpy array or a host tensor, or - all of them - as uint8
        device tensors; sizes: (h, w) per frame; layout, matrix, full_range: one value, or one per frame.  Returns one [h, w, 3] uint8
        BGR device tensor per frame: the tensors of `out` (device, uint8, contiguous, of that shape) where given, new ones otherwise.
        Device frames, and the memory of the outputs, are ordered after torch's current stream; the outputs are complete on return.
        With out_sizes - one (h, w), or one per frame - frame i comes back resized to out_sizes[i] (and `out` holds tensors of those
        shapes); with native_out=True, or a list of [h, w, 3] device tensors of the native sizes, the call returns (resized, native)."""
        import torch

        if out_sizes is not None:
            return self._to_bgr_resized(frames, sizes, layout, matrix, full_range, out, out_sizes, native_out)
        if native_out is not None and native_out is not False:
            raise ValueError("native_out goes with out_sizes")
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

    @staticmethod
    def _out_sizes(out_sizes, n: int) -> List[Tuple[int, int]]:
        if len(out_sizes) == 2 and all(isinstance(v, (int, np.integer)) for v in out_sizes):
            return [(int(out_sizes[0]), int(out_sizes[1]))] * n
        if len(out_sizes) != n:
            raise ValueError(f"{n} frames but {len(out_sizes)} output sizes")
        return [(int(h), int(w)) for h, w in out_sizes]

    @staticmethod
    def _outputs(out, shapes, dev, what: str = "out") -> List:
        import torch
        if out is None:
            return [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for h, w in shapes]
        outs = list(out)
        if len(outs) != len(shapes):
            raise ValueError(f"{len(shapes)} frames but {len(outs)} tensors in {what}")
        for i, o in enumerate(outs):
            if not (o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and tuple(o.shape) == (shapes[i][0], shapes[i][1], 3)):
                raise ValueError(f"{what}[{i}] must be a contiguous uint8 device tensor of shape ({shapes[i][0]}, {shapes[i][1]}, 3)")
        return outs

    def _to_bgr_resized(self, frames, sizes, layout, matrix, full_range, out, out_sizes, native_out):
        import torch

        n = len(frames)
        if len(sizes) != n:
            raise ValueError(f"{n} frames but {len(sizes)} sizes")
        want_native = native_out is not None and native_out is not False
        osz = self._out_sizes(out_sizes, n)
        if n == 0:
            return ([], []) if want_native else []
        if n > MAX_FRAMES:                                       # the library's limit per call
            sub = lambda v, i: v if isinstance(v, (str, bool, int)) or v is None else v[i:i + MAX_FRAMES]
            parts = [self._to_bgr_resized(frames[i:i + MAX_FRAMES], sizes[i:i + MAX_FRAMES], sub(layout, i), sub(matrix, i), sub(full_range, i),
                                          sub(out, i), osz[i:i + MAX_FRAMES], sub(native_out, i)) for i in range(0, n, MAX_FRAMES)]
            if want_native:
                return [o for p in parts for o in p[0]], [o for p in parts for o in p[1]]
            return [o for p in parts for o in p]
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
        outs = self._outputs(out, osz, dev)
        native = None
        if want_native:
            native = self._outputs(None if native_out is True else native_out, [(int(h), int(w)) for h, w in sizes], dev, "native_out")
        self.wait_stream(torch.cuda.current_stream(dev).cuda_stream)
        self._check(self.resize_raw(descs, on_dev[0], [v for s in osz for v in s], [o.data_ptr() for o in outs],
                                    None if native is None else [o.data_ptr() for o in native]))
        return (outs, native) if want_native else outs

    def resize(self, frames: Sequence, out_sizes, out: Optional[Sequence] = None) -> List:
        """frames: [h, w, 3] uint8 BGR frames, as numpy arrays (a view whose rows are a stride apart is read where it lies; its pixels
        must be contiguous), host tensors or - all of them - device tensors; out_sizes: one (h, w), or one per frame.  Returns one
        [h, w, 3] uint8 device tensor per frame, `cv2.resize(frame, (w, h))` byte for byte: the tensors of `out` where given.  Ordered
        after torch's current stream like to_bgr; complete on return."""
        import torch

        n = len(frames)
        osz = self._out_sizes(out_sizes, n)
        if n == 0:
            return []
        if n > MAX_FRAMES:
            return [o for i in range(0, n, MAX_FRAMES)
                    for o in self.resize(frames[i:i + MAX_FRAMES], osz[i:i + MAX_FRAMES], None if out is None else out[i:i + MAX_FRAMES])]
        on_dev = [bool(getattr(f, "is_cuda", False)) for f in frames]
        if any(on_dev) and not all(on_dev):
            raise ValueError("the frames of one call are all host memory or all device memory")
        dev = torch.device("cuda", self.device)
        keep, descs = [], []
        for i, f in enumerate(frames):
            d = _capi.RtdBgrFrame()
            if on_dev[i]:
                if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.stride(2) != 1 or f.stride(1) != 3:
                    raise ValueError(f"frame {i}: device frames are [h, w, 3] uint8 tensors with contiguous pixels")
                d.data, d.pitch = f.data_ptr(), int(f.stride(0)) if f.shape[0] > 1 else 3 * int(f.shape[1])
            else:
                if hasattr(f, "numpy") and not isinstance(f, np.ndarray):     # a host tensor
                    f = f.numpy()
                f = np.asarray(f)
                if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise ValueError(f"frame {i}: frames are [h, w, 3] uint8")
                if f.strides[2] != 1 or f.strides[1] != 3 or (f.shape[0] > 1 and f.strides[0] < 3 * f.shape[1]):
                    f = np.ascontiguousarray(f)
                d.data, d.pitch = f.ctypes.data, int(f.strides[0]) if f.shape[0] > 1 else 3 * int(f.shape[1])
            d.height, d.width = int(f.shape[0]), int(f.shape[1])
            keep.append(f)
            descs.append(d)
        outs = self._outputs(out, osz, dev)
        self.wait_stream(torch.cuda.current_stream(dev).cuda_stream)
        self._check(self.resize_raw(descs, on_dev[0], [v for s in osz for v in s], [o.data_ptr() for o in outs]))
        return outs


def tables(matrix: int, full_range: int) -> List[int]:
    """the constants CY, CVR, CVG, CUG, CUB the kernel uses for a matrix and range (rtd_debug_ingest_info; no GPU needed)"""
    c = (C.c_int32 * 5)()
    rc = _capi.lib().rtd_debug_ingest_info(int(matrix), int(full_range), c, None, None, 0, None, None)
    if rc != _capi.RTD_OK:
        raise _capi.RtdError(rc, "unknown matrix or range")
    return list(c)


def resize_table(ssize: int, dsize: int, columns: bool) -> List[Tuple[int, int, int, int]]:
    """the (i0, i1, w0, w1) entries of the resize stage's pass from ssize to dsize samples (rtd_debug_resize_table; no GPU needed)"""
    out = (C.c_int32 * (4 * max(int(dsize), 1)))()
    rc = _capi.lib().rtd_debug_resize_table(int(ssize), int(dsize), int(bool(columns)), out, 0, 0, None, None)
    if rc != _capi.RTD_OK:
        raise _capi.RtdError(rc, "bad size (1..65535)")
    return [tuple(out[4 * d:4 * d + 4]) for d in range(int(dsize))]


def resize_is_area2(sw: int, sh: int, ow: int, oh: int) -> bool:
    """whether the resize stage takes sw x sh -> ow x oh (width x height) as the 2 x 2 mean (rtd_debug_resize_table)"""
    flag = C.c_int32(-1)
    rc = _capi.lib().rtd_debug_resize_table(int(sw), int(ow), 1, None, int(sh), int(oh), C.byref(flag), None)
    if rc != _capi.RTD_OK:
        raise _capi.RtdError(rc, "bad size (1..65535)")
    return bool(flag.value)


def resize_tile_hw() -> Tuple[int, int]:
    """(height, width) in OUTPUT pixels of what one workgroup of the resize kernel makes (rtd_debug_resize_table)"""
    t = (C.c_int32 * 2)()
    rc = _capi.lib().rtd_debug_resize_table(0, 0, 0, None, 0, 0, None, t)
    assert rc == _capi.RTD_OK, rc
    return t[0], t[1]


def tile_hw() -> Tuple[int, int]:
    """(height, width) in pixels of what one workgroup of the kernel converts (rtd_debug_ingest_info)"""
    th, tw = C.c_int32(), C.c_int32()
    rc = _capi.lib().rtd_debug_ingest_info(0, 0, None, C.byref(th), C.byref(tw), 0, None, None)
    assert rc == _capi.RTD_OK, rc
    return th.value, tw.value
