"""The ingest's resize stage on the MI355X (csrc/ingest.hip resize_kernel): every comparison is exact equality with the restatement
(tests/resize_ref.py: the conversion of tests/yuv_ref.py, then OpenCV's 8-bit INTER_LINEAR resize of tests/face_ref.py).  Sizes are the
smallest that reach each path - one pixel, the 2 x 2 mean with byte and with dword rows, the linear tables down, up, by 3 and mixed,
odd output widths (3 W not a multiple of 4), more than one output tile each way, the same size - each with all three layouts, two
conversion tables, host and device frames, tight and padded.  Every call writes into one buffer whose bytes between the frames are
guard bytes.  Then BGR sources, the native output, a mixed batch, 64 frames in a call, output reuse, stream ordering, the limits and the
overlap check, and the chain capture class -> motion gate, JPEG encoder and Stage 2 from native pixels."""
import ctypes as C
import queue

import numpy as np
import pytest
import torch

from tests import resize_ref as ref
from tests import yuv_ref
from tests.standins import StandInPipeline
from tests.test_gpu_ingest import BAD, Outputs, desc
from tests.test_ingest_host import FakePopen
from telescope_cam_detection_amd import _capi, capture, ingest
from telescope_cam_detection_amd.jpeg import JpegEncoder
from telescope_cam_detection_amd.motion import EmptyFrameFilter
from telescope_cam_detection_amd.stage2 import BatchedStage2, CropBatcher, scaled_bbox

pytestmark = pytest.mark.gpu

RTH, RTW = ingest.resize_tile_hw()                          # host arithmetic (rtd_debug_resize_table): no GPU is touched at import
# (source h, w) -> (output h, w)
SIZES = [((1, 1), (1, 1)), ((2, 2), (1, 1)), ((3, 3), (2, 2)), ((6, 10), (3, 5)), ((7, 11), (4, 6)), ((6, 7), (3, 3)), ((9, 9), (3, 3)),
         ((5, 3), (8, 7)), ((17, 33), (9, 13)), ((34, 70), (17, 35)), ((36, 520), (18, 260)), ((40, 530), (23, 301)),
         ((2 * (RTH + 2), 2 * (RTW + 4)), (RTH + 2, RTW + 4)), ((RTH + 9, 3 * RTW // 2 + 9), (RTH + 3, RTW + 5)), ((90, 160), (36, 64)),
         ((17, 33), (17, 33)), ((16, 24), (16, 24))]
AREA = {((2, 2), (1, 1)), ((6, 10), (3, 5)), ((34, 70), (17, 35)), ((36, 520), (18, 260)), ((2 * (RTH + 2), 2 * (RTW + 4)), (RTH + 2, RTW + 4))}
VARIANTS = [(layout, matrix, full) for layout in yuv_ref.LAYOUTS for matrix, full in (("bt601", False), ("bt709", True))]
size_id = lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}"


@pytest.fixture(scope="module")
def be():
    b = ingest.FrameIngest(0)
    yield b
    b.close()


_CASES = {}


def case(size):
    """the 6 sets of planes of a size, what they convert to and what that resizes to: made once, never changed"""
    if size not in _CASES:
        (h, w), (oh, ow) = size
        planes, native, want = [], [], []
        for k, (layout, matrix, full) in enumerate(VARIANTS):
            p = yuv_ref.planes(2000 * h + 3 * w + 7 * k + ow, h, w)
            planes.append(p)
            native.append(yuv_ref.planes_to_bgr(*p, matrix, full))
            want.append(ref.resize_bgr(native[-1], oh, ow))
        _CASES[size] = (planes, native, want)
    return _CASES[size]


def test_the_sizes_reach_every_path():
    """what the cases rest on: which sizes take the 2 x 2 mean, which move dwords, which have more than one tile"""
    for (h, w), (oh, ow) in SIZES:
        assert bool(ref.is_area2(w, h, ow, oh)) == (((h, w), (oh, ow)) in AREA) == ingest.resize_is_area2(w, h, ow, oh)
    area = [o for s, o in SIZES if (s, o) in AREA]
    lin = [o for s, o in SIZES if (s, o) not in AREA]
    for group in (area, lin):
        assert any(ow % 4 == 0 for _, ow in group) and any(ow % 4 != 0 for _, ow in group)              # dword rows, byte rows
        assert any(ow > RTW and oh > RTH for oh, ow in group)                                          # more than one tile both ways
    assert any(oh > h and ow > w for (h, w), (oh, ow) in SIZES) and any(h == 3 * oh for (h, _), (oh, _) in SIZES)


def yuv_descs(planes, held, on_device, pads=None, fill=0xFF):
    """packs every set of planes in its variant's layout (tight, with the given (y, c) padding, or "dword": padded so that every row
    starts on a 4-byte boundary), uploads it for device frames and returns the descriptors; `held` keeps the buffers alive"""
    descs = []
    for (Y, U, V), (layout, matrix, full) in zip(planes, VARIANTS):
        h, w = Y.shape
        crow = yuv_ref.chroma_row_bytes(layout, w)
        if pads == "dword":
            yp, cp = w + (-w) % 4 + 4, crow + (-crow) % 4 + 8
        else:
            yp, cp = (None, None) if pads is None else (w + pads[0], crow + pads[1])
        buf, (oy, ou, ov), (yp, cp) = yuv_ref.pack(Y, U, V, layout, y_pitch=yp, c_pitch=cp, fill=fill)
        t = torch.from_numpy(buf).cuda() if on_device else buf
        held.append(t)
        base = t.data_ptr() if on_device else t.ctypes.data
        d = desc(base, h, w, layout, matrix, full)
        d.u, d.v, d.y_pitch, d.c_pitch = base + ou, (base + ov) if ov is not None else None, yp, cp
        descs.append(d)
    return descs


def resize(be, descs, on_device, hw, outs, native=None):
    rc = be.resize_raw(descs, on_device, [v for s in hw for v in s], outs.ptrs(), None if native is None else native)
    assert rc == _capi.RTD_OK, (rc, be._fn("last_error")(be._h))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_every_layout_and_two_tables_at_this_size(be, size, where):
    planes, _, want = case(size)
    held = []
    outs = Outputs([size[1]] * len(VARIANTS))
    resize(be, yuv_descs(planes, held, where == "device"), where == "device", [size[1]] * len(VARIANTS), outs)
    outs.check(want)


@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_padded_pitches_and_the_padding_does_not_matter(be, size):
    """device frames read where they lie: pitches that keep the rows on dwords and pitches that do not, two padding contents"""
    planes, _, want = case(size)
    for pads in ((13, 5), "dword"):
        for fill in (0xFF, 0x00):
            held = []
            outs = Outputs([size[1]] * len(VARIANTS))
            resize(be, yuv_descs(planes, held, True, pads, fill), True, [size[1]] * len(VARIANTS), outs)
            outs.check(want)


# ---- BGR sources ---------------------------------------------------------------------------------------------------------------------------
def bgr_desc(base, h, w, pitch):
    d = _capi.RtdBgrFrame()
    d.data, d.width, d.height, d.pitch = base, w, h, pitch
    return d


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_bgr_frames_at_this_size_tight_and_with_a_row_stride(be, size, where):
    (h, w), (oh, ow) = size
    _, native, want = case(size)
    src = [native[0], native[1]]
    wide = np.full((h, w + 5, 3), 0x5A, np.uint8)              # the second frame lies in a wider one: pitch 3 (w + 5), padding never read
    wide[:, :w] = src[1]
    held = [torch.from_numpy(np.ascontiguousarray(src[0])), torch.from_numpy(wide)]
    if where == "device":
        held = [t.cuda() for t in held]
    base = [t.data_ptr() for t in held]
    outs = Outputs([(oh, ow)] * 2, skews=[0, 1])
    resize(be, [bgr_desc(base[0], h, w, 3 * w), bgr_desc(base[1], h, w, 3 * (w + 5))], where == "device", [(oh, ow)] * 2, outs)
    outs.check(want[:2])


def test_resize_takes_numpy_views_host_tensors_and_device_tensors(be):
    h, w, oh, ow = 37, 53, 23, 31
    big = np.array(ref.bgr(40, h + 4, w + 6))
    view = big[2:2 + h, 3:3 + w]                                # rows a stride apart, pixels contiguous
    want = ref.resize_bgr(view, oh, ow)
    assert not view.flags["C_CONTIGUOUS"]
    mirrored = view[:, ::-1]                                    # pixels that run backwards: copied first
    for f, x in ((view, want), (np.ascontiguousarray(view), want), (torch.from_numpy(np.ascontiguousarray(view)), want),
                 (torch.from_numpy(big).cuda()[2:2 + h, 3:3 + w], want), (mirrored, ref.resize_bgr(mirrored, oh, ow))):
        got = be.resize([f], (oh, ow))[0]
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, 3) and got.is_contiguous()
        assert (got.cpu().numpy() == x).all(), type(f)
    two = be.resize([view, view[:20, :30]], [(oh, ow), (10, 15)])
    assert (two[1].cpu().numpy() == ref.resize_bgr(view[:20, :30], 10, 15)).all() and (two[0].cpu().numpy() == want).all()
    assert be.resize([], (4, 4)) == []
    with pytest.raises(ValueError):
        be.resize([view.astype(np.float32)], (oh, ow))
    with pytest.raises(ValueError):
        be.resize([view, torch.from_numpy(big).cuda()], (oh, ow))
    with pytest.raises(ValueError):
        be.resize([view], [(oh, ow), (oh, ow)])


# ---- the native output ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("size", [SIZES[3], SIZES[4], SIZES[9], SIZES[10], SIZES[11], SIZES[13]], ids=size_id)
def test_native_outputs_for_some_frames_of_a_call(be, size, where):
    """frames 0, 2, 3 and 5 also want their native frame (convert kernel, then the BGR kernel), 1 and 4 do not (the fused kernel)"""
    (h, w), (oh, ow) = size
    planes, native, want = case(size)
    held = []
    descs = yuv_descs(planes, held, where == "device")
    outs = Outputs([(oh, ow)] * 6 + [(h, w)] * 4, skews=[0, 0, 1, 0, 3, 0, 0, 2, 0, 0])
    ptrs = outs.ptrs()
    nat = [ptrs[6], None, ptrs[7], ptrs[8], None, ptrs[9]]
    rc = be.resize_raw(descs, where == "device", [oh, ow] * 6, ptrs[:6], nat)
    assert rc == _capi.RTD_OK, be._fn("last_error")(be._h)
    outs.check(want + [native[0], native[2], native[3], native[5]])
    # and the native output is what rtd_ingest_convert writes for the same frames
    conv = Outputs([(h, w)] * 6)
    assert be.convert_raw(descs, where == "device", conv.ptrs()) == _capi.RTD_OK
    conv.check(native)


def test_to_bgr_with_out_sizes_and_native_out_through_the_class(be):
    (h, w), (oh, ow) = (40, 530), (23, 301)
    bufs = [yuv_ref.frame(900 + k, h, w, "nv12") for k in range(3)]
    want = [ref.to_bgr_resized(b, h, w, oh, ow) for b in bufs]
    nat = [yuv_ref.to_bgr(b, h, w) for b in bufs]
    got = be.to_bgr(bufs, [(h, w)] * 3, out_sizes=(oh, ow))
    assert isinstance(got, list) and all((g.cpu().numpy() == x).all() for g, x in zip(got, want))
    got, native = be.to_bgr([torch.from_numpy(b).cuda() for b in bufs], [(h, w)] * 3, out_sizes=[(oh, ow), (h, w), (20, 265)], native_out=True)
    assert (got[0].cpu().numpy() == want[0]).all() and (got[1].cpu().numpy() == nat[1]).all() and (got[2].cpu().numpy() == ref.resize_bgr(nat[2], 20, 265)).all()
    assert all(tuple(n.shape) == (h, w, 3) and (n.cpu().numpy() == x).all() for n, x in zip(native, nat))
    mine = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
    got, native = be.to_bgr(bufs, [(h, w)] * 3, out_sizes=(oh, ow), native_out=mine)
    assert all(n is m for n, m in zip(native, mine)) and all((m.cpu().numpy() == x).all() for m, x in zip(mine, nat))
    assert be.to_bgr([], [], out_sizes=(4, 4)) == [] and be.to_bgr([], [], out_sizes=(4, 4), native_out=True) == ([], [])
    with pytest.raises(ValueError):
        be.to_bgr(bufs, [(h, w)] * 3, native_out=True)          # native_out goes with out_sizes
    with pytest.raises(ValueError):
        be.to_bgr(bufs, [(h, w)] * 3, out_sizes=[(oh, ow)] * 2)
    with pytest.raises(ValueError):
        be.to_bgr(bufs, [(h, w)] * 3, out_sizes=(oh, ow), native_out=[torch.zeros((h, w + 1, 3), dtype=torch.uint8, device="cuda")] * 3)


# ---- batches --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_one_batch_of_mixed_sizes_paths_layouts_and_tables(be, where):
    """different source and output sizes in one call: the 2 x 2 mean on dword and on byte rows, the tables down and up, one pixel, more
    than one tile; three outputs off the dword boundary (a dword-row frame then moves byte by byte)"""
    spec = [((36, 520), (18, 260), "nv12", "bt601", False), ((40, 530), (23, 301), "i420", "bt709", True), ((6, 10), (3, 5), "nv21", "bt709", False),
            ((5, 3), (8, 7), "i420", "bt601", True), ((1, 1), (1, 1), "nv21", "bt601", False), ((2 * RTH + 4, 2 * RTW + 8), (RTH + 2, RTW + 4), "i420", "bt601", False),
            ((90, 160), (36, 64), "nv12", "bt709", True), ((34, 72), (17, 36), "nv12", "bt601", False)]
    on_device = where == "device"
    held, descs, want = [], [], []
    for k, ((h, w), (oh, ow), layout, matrix, full) in enumerate(spec):
        Y, U, V = yuv_ref.planes(300 + k, h, w)
        buf = yuv_ref.pack(Y, U, V, layout)[0]
        held.append(torch.from_numpy(buf).cuda() if on_device else buf)
        descs.append(desc(held[-1].data_ptr() if on_device else buf.ctypes.data, h, w, layout, matrix, full))
        want.append(ref.planes_resized(Y, U, V, oh, ow, matrix, full))
    outs = Outputs([s[1] for s in spec], skews=[0, 0, 1, 0, 3, 0, 0, 2])
    resize(be, descs, on_device, [s[1] for s in spec], outs)
    outs.check(want)


def test_64_frames_in_one_call_and_65_through_the_class(be):
    sizes = [((4, 4), (2, 2)), ((3, 3), (2, 2)), ((2, 2), (3, 4))]
    raw = [yuv_ref.frame(400 + k, *sizes[k % 3][0], yuv_ref.LAYOUTS[k % 3]) for k in range(65)]
    want = [ref.to_bgr_resized(raw[k], *sizes[k % 3][0], *sizes[k % 3][1], yuv_ref.LAYOUTS[k % 3], *yuv_ref.TABLES[k % 4]) for k in range(65)]
    outs = Outputs([sizes[k % 3][1] for k in range(64)])
    resize(be, [desc(raw[k].ctypes.data, *sizes[k % 3][0], yuv_ref.LAYOUTS[k % 3], *yuv_ref.TABLES[k % 4]) for k in range(64)], False,
           [sizes[k % 3][1] for k in range(64)], outs)
    outs.check(want[:64])
    got, native = be.to_bgr(raw, [sizes[k % 3][0] for k in range(65)], layout=[yuv_ref.LAYOUTS[k % 3] for k in range(65)],
                            matrix=[yuv_ref.TABLES[k % 4][0] for k in range(65)], full_range=[yuv_ref.TABLES[k % 4][1] for k in range(65)],
                            out_sizes=[sizes[k % 3][1] for k in range(65)], native_out=True)
    assert len(got) == len(native) == 65 and all((g.cpu().numpy() == w).all() for g, w in zip(got, want))
    assert (native[64].cpu().numpy() == yuv_ref.to_bgr(raw[64], *sizes[64 % 3][0], yuv_ref.LAYOUTS[64 % 3], *yuv_ref.TABLES[0])).all()
    bgr = [np.array(ref.bgr(k, 5, 7)) for k in range(65)]
    got = be.resize(bgr, (3, 4))
    assert len(got) == 65 and all((g.cpu().numpy() == ref.resize_bgr(f, 3, 4)).all() for g, f in zip(got, bgr))


def test_out_is_reused_across_two_calls_with_different_content(be):
    (h, w), (oh, ow) = (2 * RTH + 6, 2 * RTW + 16), (RTH + 3, RTW + 8)
    out = [torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")]
    ptr = out[0].data_ptr()
    for seed in (600, 601):
        buf = yuv_ref.frame(seed, h, w, "nv12")
        got = be.to_bgr([buf], [(h, w)], out=out, out_sizes=(oh, ow))
        assert got[0] is out[0] and got[0].data_ptr() == ptr and (out[0].cpu().numpy() == ref.to_bgr_resized(buf, h, w, oh, ow)).all()
        got = be.resize([yuv_ref.to_bgr(buf, h, w)], (oh, ow), out=out)
        assert got[0] is out[0] and (out[0].cpu().numpy() == ref.to_bgr_resized(buf, h, w, oh, ow)).all()
    with pytest.raises(ValueError):
        be.to_bgr([buf], [(h, w)], out=[torch.zeros((oh, ow + 1, 3), dtype=torch.uint8, device="cuda")], out_sizes=(oh, ow))


def test_a_device_frame_written_on_a_side_stream_just_before_the_call(be):
    (h, w), (oh, ow) = (130, 250), (87, 167)
    buf = yuv_ref.frame(700, h, w, "nv12")
    src = torch.from_numpy(buf).pin_memory()
    frame = torch.zeros(buf.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)                       # the write below is still pending when the call is made
        frame.copy_(src, non_blocking=True)
        got, native = be.to_bgr([frame], [(h, w)], out_sizes=(oh, ow), native_out=True)      # ordered after `side`, torch's current stream here
    assert (got[0].cpu().numpy() == ref.to_bgr_resized(buf, h, w, oh, ow)).all() and (native[0].cpu().numpy() == yuv_ref.to_bgr(buf, h, w)).all()
    torch.cuda.synchronize()


# ---- the limits -----------------------------------------------------------------------------------------------------------------------------
def _two(h=6, w=10):
    raw = [yuv_ref.frame(800, h, w, "nv12"), yuv_ref.frame(801, h, w, "i420")]
    return raw, [desc(raw[0].ctypes.data, h, w, "nv12"), desc(raw[1].ctypes.data, h, w, "i420")]


def refused(be, rc, frame):
    assert rc == _capi.RTD_E_INVALID and (frame is None or f"frame {frame}".encode() in be._fn("last_error")(be._h)), (rc, be._fn("last_error")(be._h))


@pytest.mark.parametrize("what", sorted(BAD))
def test_a_bad_source_frame_is_refused_with_its_index_and_nothing_is_written(be, what):
    raw, descs = _two()
    BAD[what](descs[1])                                     # frame 1 (I420) is the bad one: frame 0 must not be resized either
    outs = Outputs([(3, 5)] * 2 + [(6, 10)] * 2)
    p = outs.ptrs()
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, p[:2], p[2:]), 1)
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, p[:2]), 1)
    outs.untouched()


def test_output_sizes_counts_null_pointers_and_shared_outputs_are_refused_and_the_handle_goes_on(be):
    raw, descs = _two()
    outs = Outputs([(3, 5)] * 2 + [(6, 10)] * 2)
    p = outs.ptrs()
    for hw, frame in (([3, 5, 0, 5], 1), ([3, 65536, 3, 5], 0), ([3, 5, 3, -1], 1)):
        refused(be, be.resize_raw(descs, False, hw, p[:2], p[2:]), frame)
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, p[:2], n=0), None)
    refused(be, be.resize_raw(descs * 33, False, [3, 5] * 66, p[:2] * 33), None)
    assert b"RTD_INGEST_MAX_FRAMES" in be._fn("last_error")(be._h)
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, [p[0], None]), 1)
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, [p[0], p[0] + 44]), 1)                  # one shared byte (3 x 5 x 3 = 45)
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, [p[0], p[0]]), 1)
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, p[:2], [p[2], p[2] + 179]), 1)          # two native outputs (6 x 10 x 3 = 180)
    refused(be, be.resize_raw(descs, False, [3, 5] * 2, p[:2], [None, p[1] + 44]), 1)           # a native output on an output
    L, arr, hw2, o2 = be._L, (_capi.RtdYuvFrame * 2)(*descs), (C.c_int32 * 4)(3, 5, 3, 5), (C.c_void_p * 2)(*p[:2])
    assert L.rtd_ingest_convert_resize(be._h, 2, None, 0, hw2, o2, None) == _capi.RTD_E_INVALID
    assert L.rtd_ingest_convert_resize(be._h, 2, arr, 0, None, o2, None) == _capi.RTD_E_INVALID
    assert L.rtd_ingest_convert_resize(be._h, 2, arr, 0, hw2, None, None) == _capi.RTD_E_INVALID
    assert L.rtd_ingest_convert_resize(None, 2, arr, 0, hw2, o2, None) == _capi.RTD_E_INVALID
    # the BGR call
    f = np.array(ref.bgr(1, 6, 10))
    good = lambda: [bgr_desc(f.ctypes.data, 6, 10, 30), bgr_desc(f.ctypes.data, 6, 10, 30)]
    for edit, frame in ((lambda d: setattr(d[1], "width", 0), 1), (lambda d: setattr(d[0], "height", 65536), 0), (lambda d: setattr(d[1], "pitch", 29), 1),
                        (lambda d: setattr(d[1], "data", None), 1)):
        d = good()
        edit(d)
        refused(be, be.resize_raw(d, False, [3, 5] * 2, p[:2]), frame)
    refused(be, be.resize_raw(good(), False, [3, 5, 3, 0], p[:2]), 1)
    refused(be, be.resize_raw(good(), False, [3, 5] * 2, [p[0], p[0] + 1]), 1)
    barr = (_capi.RtdBgrFrame * 2)(*good())
    assert L.rtd_ingest_resize(be._h, 2, None, 0, hw2, o2) == _capi.RTD_E_INVALID and L.rtd_ingest_resize(be._h, 0, barr, 0, hw2, o2) == _capi.RTD_E_INVALID
    assert L.rtd_ingest_resize(None, 2, barr, 0, hw2, o2) == _capi.RTD_E_INVALID
    outs.untouched()
    rc = be.resize_raw(descs, False, [3, 5] * 2, p[:2], p[2:])   # and a good call after the refusals
    assert rc == _capi.RTD_OK
    nat = [yuv_ref.to_bgr(raw[0], 6, 10, "nv12"), yuv_ref.to_bgr(raw[1], 6, 10, "i420")]
    outs.check([ref.resize_bgr(n, 3, 5) for n in nat] + nat)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def test_capture_at_native_size_feeds_the_gate_the_encoder_and_stage2_from_native_pixels(be):
    (h, w), (th, tw) = (160, 224), (80, 112)
    planes = [yuv_ref.scene_planes(7, h, w), yuv_ref.scene_planes(8, h, w)]
    raw = [yuv_ref.pack(*p, layout="nv12")[0].tobytes() for p in planes]
    native_want = [yuv_ref.planes_to_bgr(*p) for p in planes]
    want = [ref.resize_bgr(n, th, tw) for n in native_want]
    popen = FakePopen([b"".join(raw)])
    cap = capture.RTSPStreamCaptureGPU("rtsp://cam/1", queue.Queue(), target_width=tw, target_height=th, camera_id="c1", popen=popen, ingest=be,
                                       source_size=(w, h), keep_native=True)
    cap.settle_delay = cap.reconnect_delay = cap.error_delay = 0
    popen.cap = cap
    cap._capture_loop()
    items = [cap.frame_queue.get_nowait() for _ in range(2)]
    assert cap.frame_queue.empty() and [it["frame_id"] for it in items] == [0, 1] and "-s" not in popen.commands[0]
    gate_a, gate_b, enc = EmptyFrameFilter(device=0), EmptyFrameFilter(device=0), JpegEncoder(0)
    try:
        for it, bgr, nat in zip(items, want, native_want):
            f, nf = it["frame"], it["native_frame"]
            assert f.is_cuda and tuple(f.shape) == (th, tw, 3) and nf.is_cuda and tuple(nf.shape) == (h, w, 3) and it["is_gpu_tensor"] is True
            assert (f.cpu().numpy() == bgr).all() and (nf.cpu().numpy() == nat).all()
            up = torch.from_numpy(bgr).cuda()
            assert gate_a.has_motion(f) == gate_b.has_motion(up)
            assert enc.encode(f, 90) == enc.encode(up, 90)
        assert gate_a.get_stats() == gate_b.get_stats() and gate_a.get_stats()["total_frames"] == 2
        assert (cap.get_latest_native_frame().cpu().numpy() == native_want[1]).all()
        assert cap.get_latest_native_frame().data_ptr() != items[1]["native_frame"].data_ptr()
    finally:
        gate_a._backend.close()
        gate_b._backend.close()
        enc.close()
    # Stage 2: a 24 x 20 bird at the detector's size is skipped (min_crop_size 32) and classified from the native frame, where it is 48 x 40
    p = StandInPipeline(categories=("bird",), min_crop_size=32)
    batcher = CropBatcher(input_size=64, min_crop_size=32)
    seen = []
    p.species_classifiers["bird"].model.register_forward_pre_hook(lambda m, args: seen.append(args[0].clone()))
    dets = lambda: [[{"class_id": 14, "confidence": 0.9, "bbox": {"x1": 10.0, "y1": 8.0, "x2": 34.0, "y2": 28.0}},
                     {"class_id": 14, "confidence": 0.8, "bbox": {"x1": 60.5, "y1": 30.25, "x2": 112.0, "y2": 80.0}}], []]
    s2 = BatchedStage2(p, batcher=batcher)
    frames, natives = [it["frame"] for it in items], [it["native_frame"] for it in items]
    plain = s2.process_batch(frames, dets())
    assert len(seen) == 1 and seen[0].shape[0] == 1 and plain[0][0]["species"] is None          # only the large box at the detector's size
    seen.clear()
    got = s2.process_batch(frames, dets(), native_frames=natives)
    rects = [batcher.rects_for(dets()[0], (th, tw), source_hw=(h, w))[1], []]
    assert len(rects[0]) == 2 and rects[0][0] == (11, 8, 77, 64)       # (20, 16, 68, 56) padded by int(48 * 0.2) = 9 and int(40 * 0.2) = 8
    assert len(seen) == 1 and torch.equal(seen[0], batcher.preprocess_batch(natives, rects))
    assert [got[0][0]["bbox"][k] for k in ("x1", "y1", "x2", "y2")] == [10.0, 8.0, 34.0, 28.0]       # detector-frame coordinates stay
    assert "species" in got[0][0] and got[0][0].get("stage2_category") == "bird"
    seen.clear()
    s2.process_batch(frames, dets(), native_frames=[None, natives[1]])                           # no native frame for camera 0: the detector frame
    assert len(seen) == 1 and torch.equal(seen[0], batcher.preprocess_batch(frames, [batcher.rects_for(dets()[0], (th, tw))[1], []]))
    assert scaled_bbox(dets()[0][0]["bbox"], (th, tw), (h, w)) == {"x1": 20.0, "y1": 16.0, "x2": 68.0, "y2": 56.0}
