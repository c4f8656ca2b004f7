"""The frame ingest on the MI355X (csrc/ingest.hip): every comparison is exact equality with the numpy restatement (tests/yuv_ref.py).
Sizes are the smallest that reach each path of the kernel - one pixel, one block, odd in each direction, 3 W not a multiple of 4, whole
dword strips with and without a 4-pixel tail, one tile and one more in each direction, more than one tile both ways - each with all
three layouts and all four tables, from host frames and from device frames.  Every call writes into one buffer whose bytes between
the frames are guard bytes.  Then padded pitches, a mixed batch, 64 frames in a call, output reuse, stream ordering, the limits, the
handle scaffold, and the chain capture class -> motion gate and JPEG encoder."""
import ctypes as C
import queue

import numpy as np
import pytest
import torch

from tests import yuv_ref as ref
from tests.test_ingest_host import FakePopen
from telescope_cam_detection_amd import _capi, capture, ingest
from telescope_cam_detection_amd.jpeg import JpegEncoder
from telescope_cam_detection_amd.motion import EmptyFrameFilter

pytestmark = pytest.mark.gpu

GUARD = 0xA5
TH, TW = ingest.tile_hw()                                   # host arithmetic (rtd_debug_ingest_info): no GPU is touched at import
SIZES = [(1, 1), (2, 2), (3, 5), (5, 3), (2, 6), (6, 2), (6, 10), (10, 6), (4, 8), (8, 4), (5, 12), (TH, TW), (TH + 1, TW), (TH, TW + 1),
         (TH + 1, TW + 1), (37, 53), (130, 250), (2 * TH + 2, 2 * TW + 8)]
VARIANTS = [(layout, matrix, full) for layout in ref.LAYOUTS for matrix, full in ref.TABLES]          # 12 frames per size


@pytest.fixture(scope="module")
def be():
    b = ingest.FrameIngest(0)
    yield b
    b.close()


_CASES = {}


def case(h, w):
    """the 12 frames of a size, tightly packed, and what they convert to: made once, never changed"""
    if (h, w) not in _CASES:
        frames, want = [], []
        for k, (layout, matrix, full) in enumerate(VARIANTS):
            Y, U, V = ref.planes(1000 * h + w + 7 * k, h, w)
            buf = ref.pack(Y, U, V, layout)[0]
            buf.setflags(write=False)
            frames.append(buf)
            want.append(ref.planes_to_bgr(Y, U, V, matrix, full))
        _CASES[(h, w)] = (frames, want)
    return _CASES[(h, w)]


def desc(base, h, w, layout, matrix="bt601", full=False):
    return ingest.tight_frame(base, h, w, ingest.LAYOUTS[layout], ingest.MATRICES[matrix], int(full))


class Outputs:
    """one device buffer for the outputs of a call, every frame on a 4-byte boundary (plus `skew`), guard bytes everywhere else"""

    def __init__(self, shapes, skews=None):
        self.shapes, self.offs, at = shapes, [], 64
        for i, (h, w) in enumerate(shapes):
            at = (at + 3) // 4 * 4 + (skews[i] if skews else 0)
            self.offs.append(at)
            at += h * w * 3 + 32
        self.buf = torch.full((at + 64,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def ptrs(self):
        return [self.buf.data_ptr() + o for o in self.offs]

    def check(self, want):
        got = self.buf.cpu().numpy()
        rest = np.ones(got.size, bool)
        for i, ((h, w), o) in enumerate(zip(self.shapes, self.offs)):
            g = got[o:o + h * w * 3].reshape(h, w, 3)
            assert (g == want[i]).all(), (i, (h, w), np.argwhere(g != want[i])[:4].tolist())
            rest[o:o + h * w * 3] = False
        assert (got[rest] == GUARD).all(), "a byte outside the frames was written"

    def untouched(self):
        assert bool((self.buf == GUARD).all())


def convert(be, descs, on_device, outs):
    rc = be.convert_raw(descs, on_device, outs.ptrs())
    assert rc == _capi.RTD_OK, (rc, be._fn("last_error")(be._h))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_layout_and_table_at_this_size(be, hw, where):
    h, w = hw
    frames, want = case(h, w)
    on_device = where == "device"
    held = [torch.from_numpy(np.array(f)).cuda() for f in frames] if on_device else frames
    base = [f.data_ptr() if on_device else f.ctypes.data for f in held]
    outs = Outputs([(h, w)] * len(frames))
    convert(be, [desc(b, h, w, *v) for b, v in zip(base, VARIANTS)], on_device, outs)
    outs.check(want)


def test_the_sizes_reach_the_dword_path_and_the_byte_path():
    """what the cases above rest on: a tight frame moves as dwords exactly when W % 4 == 0 (and, I420, its V plane starts on a dword)"""
    wide = [(h, w) for h, w in SIZES if w % 4 == 0]
    assert (4, 8) in wide and (5, 12) in wide and (TH, TW) in wide and (TH + 1, TW) in wide and len(wide) < len(SIZES)
    assert any(w % 8 == 4 for _, w in wide) and any(h % 2 == 1 for h, _ in wide)                       # a 4-pixel tail; a single last row
    assert any((((h + 1) // 2) * ((w + 1) // 2)) % 4 != 0 for h, w in wide) and any((((h + 1) // 2) * ((w + 1) // 2)) % 4 == 0 for h, w in wide)


@pytest.mark.parametrize("pads", [(13, 5), (16, 8), (4, 0)], ids=lambda p: f"y{p[0]}c{p[1]}")
def test_padded_pitches_on_device_frames_and_the_padding_does_not_matter(be, pads):
    ypad, cpad = pads
    shapes = [(37, 53), (TH + 1, TW), (6, 12), (5, 3)]
    for fill in (0xFF, 0x00):
        held, descs, want = [], [], []
        for k, (h, w) in enumerate(shapes):
            for layout in ref.LAYOUTS:
                matrix, full = ref.TABLES[(k + len(descs)) % 4]
                Y, U, V = ref.planes(50 + k, h, w)
                buf, (oy, ou, ov), (yp, cp) = ref.pack(Y, U, V, layout, y_pitch=w + ypad, c_pitch=ref.chroma_row_bytes(layout, w) + cpad, fill=fill)
                t = torch.from_numpy(buf).cuda()
                held.append(t)
                d = desc(t.data_ptr(), h, w, layout, matrix, full)
                d.u, d.v, d.y_pitch, d.c_pitch = t.data_ptr() + ou, (t.data_ptr() + ov) if ov is not None else None, yp, cp
                descs.append(d)
                want.append(ref.planes_to_bgr(Y, U, V, matrix, full))
        outs = Outputs([s for s in shapes for _ in ref.LAYOUTS])
        convert(be, descs, True, outs)
        outs.check(want)


@pytest.mark.parametrize("where", ["host", "device"])
def test_one_batch_of_six_frames_of_mixed_sizes_layouts_and_tables(be, where):
    """sizes of every class in one call: a byte-path frame, dword-path frames with and without a tail, odd both ways, more than one
    tile, one pixel; two outputs off the dword boundary (a dword-path frame then moves byte by byte)"""
    spec = [((37, 53), "nv12", "bt601", False), ((TH, TW + 8), "i420", "bt709", True), ((5, 12), "nv21", "bt709", False),
            ((2 * TH + 1, 2 * TW + 3), "i420", "bt601", True), ((1, 1), "nv21", "bt601", False), ((4, 8), "nv12", "bt709", True)]
    on_device = where == "device"
    held, descs, want = [], [], []
    for k, ((h, w), layout, matrix, full) in enumerate(spec):
        Y, U, V = ref.planes(300 + k, h, w)
        buf = ref.pack(Y, U, V, layout)[0]
        held.append(torch.from_numpy(buf).cuda() if on_device else buf)
        descs.append(desc(held[-1].data_ptr() if on_device else buf.ctypes.data, h, w, layout, matrix, full))
        want.append(ref.planes_to_bgr(Y, U, V, matrix, full))
    outs = Outputs([s[0] for s in spec], skews=[0, 0, 1, 0, 3, 2])
    convert(be, descs, on_device, outs)
    outs.check(want)


def test_64_frames_of_2x2_in_one_call_and_65_through_the_class(be):
    raw = [ref.frame(400 + k, 2, 2, ref.LAYOUTS[k % 3]) for k in range(65)]
    want = [ref.to_bgr(raw[k], 2, 2, ref.LAYOUTS[k % 3], *ref.TABLES[k % 4]) for k in range(65)]
    outs = Outputs([(2, 2)] * 64)
    convert(be, [desc(raw[k].ctypes.data, 2, 2, ref.LAYOUTS[k % 3], *ref.TABLES[k % 4]) for k in range(64)], False, outs)
    outs.check(want[:64])
    got = be.to_bgr(raw, [(2, 2)] * 65, layout=[ref.LAYOUTS[k % 3] for k in range(65)], matrix=[ref.TABLES[k % 4][0] for k in range(65)],
                    full_range=[ref.TABLES[k % 4][1] for k in range(65)])
    assert len(got) == 65 and all((g.cpu().numpy() == w).all() for g, w in zip(got, want))


def test_to_bgr_takes_bytes_arrays_host_tensors_and_device_tensors(be):
    h, w = 37, 53
    buf = ref.frame(500, h, w, "nv12")
    want = ref.to_bgr(buf, h, w)
    for f in (buf.tobytes(), bytearray(buf.tobytes()), buf, torch.from_numpy(buf.copy()), torch.from_numpy(buf.copy()).cuda()):
        out = be.to_bgr([f], [(h, w)])[0]
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and out.is_contiguous()
        assert (out.cpu().numpy() == want).all(), type(f)
    i420 = ref.frame(500, h, w, "i420")
    assert (be.to_bgr([i420], [(h, w)], layout="i420", matrix="bt709", full_range=True)[0].cpu().numpy() == ref.to_bgr(i420, h, w, "i420", "bt709", True)).all()
    assert be.to_bgr([], []) == []
    with pytest.raises(ValueError):
        be.to_bgr([buf[:-1]], [(h, w)])
    with pytest.raises(ValueError):
        be.to_bgr([buf], [(h, w)], layout="yuy2")
    with pytest.raises(ValueError):
        be.to_bgr([buf, torch.from_numpy(buf.copy()).cuda()], [(h, w)] * 2)


def test_out_is_reused_across_two_calls_with_different_content(be):
    h, w = TH + 1, TW + 8
    out = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")]
    ptr = out[0].data_ptr()
    for seed in (600, 601):
        buf = ref.frame(seed, h, w, "nv12")
        got = be.to_bgr([buf], [(h, w)], out=out)
        assert got[0] is out[0] and got[0].data_ptr() == ptr
        assert (out[0].cpu().numpy() == ref.to_bgr(buf, h, w)).all()
    with pytest.raises(ValueError):
        be.to_bgr([buf], [(h, w)], out=[torch.zeros((h, w + 1, 3), dtype=torch.uint8, device="cuda")])


def test_a_device_frame_written_on_a_side_stream_just_before_the_call(be):
    h, w = 130, 250
    buf = ref.frame(700, h, w, "nv12")
    src = torch.from_numpy(buf).pin_memory()
    frame = torch.zeros(buf.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)                       # the write below is still pending when the call is made
        frame.copy_(src, non_blocking=True)
        got = be.to_bgr([frame], [(h, w)])[0]               # ordered after `side`, torch's current stream here
    assert (got.cpu().numpy() == ref.to_bgr(buf, h, w)).all()
    torch.cuda.synchronize()


def _two(h=6, w=10):
    raw = [ref.frame(800, h, w, "nv12"), ref.frame(801, h, w, "i420")]
    return raw, [desc(raw[0].ctypes.data, h, w, "nv12"), desc(raw[1].ctypes.data, h, w, "i420")]


BAD = {
    "width 0": lambda d: setattr(d, "width", 0),
    "height 65536": lambda d: setattr(d, "height", 65536),
    "width -1": lambda d: setattr(d, "width", -1),
    "y_pitch": lambda d: setattr(d, "y_pitch", 9),
    "c_pitch": lambda d: setattr(d, "c_pitch", 4),
    "null y": lambda d: setattr(d, "y", None),
    "null u": lambda d: setattr(d, "u", None),
    "null v": lambda d: setattr(d, "v", None),
    "layout": lambda d: setattr(d, "layout", 3),
    "matrix": lambda d: setattr(d, "matrix", 2),
    "range": lambda d: setattr(d, "full_range", 2),
    "range -1": lambda d: setattr(d, "full_range", -1),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_a_limit_or_bad_enum_is_refused_with_the_frames_index_and_nothing_is_written(be, what):
    raw, descs = _two()
    BAD[what](descs[1])                                     # frame 1 (I420) is the bad one: frame 0 must not be converted either
    outs = Outputs([(6, 10)] * 2)
    assert be.convert_raw(descs, False, outs.ptrs()) == _capi.RTD_E_INVALID
    assert b"frame 1" in be._fn("last_error")(be._h)
    outs.untouched()


def test_frame_counts_and_null_outputs_are_refused_and_the_handle_goes_on(be):
    raw, descs = _two()
    outs = Outputs([(6, 10)] * 2)
    assert be.convert_raw(descs, False, outs.ptrs(), n=0) == _capi.RTD_E_INVALID
    assert be.convert_raw(descs * 33, False, outs.ptrs() * 33) == _capi.RTD_E_INVALID and b"RTD_INGEST_MAX_FRAMES" in be._fn("last_error")(be._h)
    assert be.convert_raw(descs, False, [outs.ptrs()[0], None]) == _capi.RTD_E_INVALID and b"frame 1" in be._fn("last_error")(be._h)
    assert be._L.rtd_ingest_convert(be._h, 2, None, 0, (C.c_void_p * 2)(*outs.ptrs())) == _capi.RTD_E_INVALID
    assert be._L.rtd_ingest_convert(be._h, 2, (_capi.RtdYuvFrame * 2)(*descs), 0, None) == _capi.RTD_E_INVALID
    assert be._L.rtd_ingest_convert(None, 2, (_capi.RtdYuvFrame * 2)(*descs), 0, (C.c_void_p * 2)(*outs.ptrs())) == _capi.RTD_E_INVALID
    outs.untouched()
    convert(be, descs, False, outs)                         # and a good call after the refusals
    outs.check([ref.to_bgr(raw[0], 6, 10, "nv12"), ref.to_bgr(raw[1], 6, 10, "i420")])


def test_create_refused_create_wait_stream_and_close_as_the_scaffold_promises():
    L = _capi.lib()
    h = C.c_void_p(0xDEAD)
    assert L.rtd_ingest_create(torch.cuda.device_count(), C.byref(h)) == _capi.RTD_E_INVALID and h.value is None
    assert b"no such device" in L.rtd_ingest_last_error(None)
    assert L.rtd_ingest_create(0, None) == _capi.RTD_E_INVALID
    with pytest.raises(_capi.RtdError, match="no such device"):
        ingest.FrameIngest(torch.cuda.device_count())
    b = ingest.FrameIngest(0)
    try:
        assert b._h.value and (L.rtd_ingest_last_error(b._h) or b"") == b""
        b.wait_stream(0)
        raw, descs = _two()
        outs = Outputs([(6, 10)] * 2)
        convert(b, descs, False, outs)
        first = outs.buf.cpu().numpy().tobytes()
        descs[0].layout = 7
        assert b.convert_raw(descs, False, outs.ptrs()) == _capi.RTD_E_INVALID and b"frame 0" in L.rtd_ingest_last_error(b._h)
        descs[0].layout = 0
        convert(b, descs, False, outs)
        assert outs.buf.cpu().numpy().tobytes() == first
    finally:
        b.close()
    assert not b._h.value
    b.close()                                               # closing twice is harmless
    L.rtd_ingest_destroy(None)


def test_capture_feeds_the_motion_gate_and_the_jpeg_encoder_what_the_restatement_would(be):
    h, w = 160, 224
    planes = [ref.scene_planes(7, h, w), ref.scene_planes(8, h, w)]
    raw = [ref.pack(*p, layout="nv12")[0].tobytes() for p in planes]
    want = [ref.planes_to_bgr(*p) for p in planes]
    popen = FakePopen([b"".join(raw)])
    cap = capture.RTSPStreamCaptureGPU("rtsp://cam/1", queue.Queue(), target_width=w, target_height=h, camera_id="c1", popen=popen, ingest=be)
    cap.settle_delay = cap.reconnect_delay = cap.error_delay = 0
    popen.cap = cap
    cap._capture_loop()
    items = [cap.frame_queue.get_nowait() for _ in range(2)]
    assert cap.frame_queue.empty() and [it["frame_id"] for it in items] == [0, 1]
    gate_a, gate_b, enc = EmptyFrameFilter(device=0), EmptyFrameFilter(device=0), JpegEncoder(0)
    try:
        for it, bgr in zip(items, want):
            f = it["frame"]
            assert f.is_cuda and f.dtype == torch.uint8 and tuple(f.shape) == (h, w, 3) and it["is_gpu_tensor"] is True
            assert (f.cpu().numpy() == bgr).all()
            up = torch.from_numpy(bgr).cuda()
            assert gate_a.has_motion(f) == gate_b.has_motion(up)
            assert enc.encode(f, 90) == enc.encode(up, 90)
        assert gate_a.get_stats() == gate_b.get_stats() and gate_a.get_stats()["total_frames"] == 2
        assert (cap.get_latest_frame().cpu().numpy() == want[1]).all() and cap.get_latest_frame().data_ptr() != items[1]["frame"].data_ptr()
    finally:
        gate_a._backend.close()
        gate_b._backend.close()
        enc.close()
