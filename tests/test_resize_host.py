"""The host side of the ingest's resize stage, without a GPU: the library's tap tables and its area rule against the restatement
(tests/face_ref.py through tests/resize_ref.py), hand-worked pixels against literal values, that the area rule and the linear tables give the same
bytes at an exact 2x (and what does tell two functions apart), Stage 2's rectangles in native pixels, and the capture loop with `source_size` (a stand-in for
ffmpeg and an ingest that answers from the restatement)."""
import queue
import types

import numpy as np
import pytest

from telescope_cam_detection_amd import _capi, capture, ingest
from telescope_cam_detection_amd.stage2 import CropBatcher, scaled_bbox
from tests import resize_ref as ref
from tests import yuv_ref
from tests.test_ingest_host import FakePopen, drain

BIG = [(2560, 1280), (3840, 1280), (1920, 640), (65535, 1), (1, 65535), (1080, 720)]


@pytest.mark.parametrize("columns", [True, False], ids=["columns", "rows"])
def test_the_librarys_tables_are_the_restatements(columns):
    for s in range(1, 41):
        for d in range(1, 41):
            assert ingest.resize_table(s, d, columns) == ref.linear_table(s, d, columns), (s, d)
    for s, d in BIG:
        assert ingest.resize_table(s, d, columns) == ref.linear_table(s, d, columns), (s, d)


def test_the_table_call_refuses_sizes_outside_the_limits():
    for s, d in ((0, 4), (4, 0), (65536, 4), (4, 65536), (-1, 1)):
        with pytest.raises(_capi.RtdError):
            ingest.resize_table(s, d, True)
        with pytest.raises(_capi.RtdError):
            ingest.resize_is_area2(s, 4, d, 2)
    th, tw = ingest.resize_tile_hw()
    assert th >= 1 and tw >= 4 and tw % 4 == 0


@pytest.mark.parametrize("case", [((2, 2), (1, 1), True), ((10, 6), (5, 3), True), ((6, 7), (3, 3), False), ((7, 7), (3, 3), False),
                                  ((2560, 1440), (1280, 720), True), ((3840, 2160), (1280, 720), False), ((4, 4), (4, 4), False),
                                  ((4, 4), (8, 8), False), ((5, 4), (2, 2), False)], ids=str)
def test_the_area_rule_of_the_library_and_of_the_restatement(case):
    (sw, sh), (ow, oh), want = case
    assert bool(ref.is_area2(sw, sh, ow, oh)) is want
    assert ingest.resize_is_area2(sw, sh, ow, oh) is want


def test_a_hand_worked_2x2_block_and_a_3x1_row():
    block = np.array([[(10, 20, 30), (11, 22, 33)], [(12, 24, 36), (14, 27, 39)]], np.uint8)
    assert ref.resize_bgr(block, 1, 1).tolist() == [[[12, 23, 35]]]                    # (47 + 2) >> 2, (93 + 2) >> 2, (138 + 2) >> 2
    # scale 1.5: output 0 sits at 0.25 (weights 1536, 512 on pixels 0, 1), output 1 at 1.75 (512, 1536 on pixels 1, 2); the one row
    # has the weights 2048, 0.  Blue of output 0: H = 40 * 512 = 20480, ((2048 * (20480 >> 4)) >> 16) = 40, (40 + 2) >> 2 = 10
    row = np.array([[(0, 100, 255), (40, 100, 0), (200, 100, 255)]], np.uint8)
    assert ref.linear_table(3, 2, True) == [(0, 1, 1536, 512), (1, 2, 512, 1536)] and ref.linear_table(1, 1, False) == [(0, 0, 2048, 0)]
    assert ref.resize_bgr(row, 1, 2).tolist() == [[[10, 100, 191], [160, 100, 191]]]
    assert ref.forced_linear(row, 1, 2).tolist() == [[[10, 100, 191], [160, 100, 191]]]


def test_the_area_rule_and_the_linear_tables_agree_at_an_exact_2x_and_converting_first_is_not_averaging_first():
    """The issue asked for a scene on which the area result DIFFERS from the forced-linear one, so that a kernel without the area rule
    could not pass.  No such scene exists, in this restatement or in cv2: at a scale of exactly 2 every column entry is (2 d, 2 d + 1,
    1024, 1024) and every row entry likewise, so H = (a + b) * 1024, (1024 * (H >> 4)) >> 16 = a + b without a remainder, and the
    result is ((a + b) + (c + d) + 2) >> 2: the area mean, bit for bit.  The two paths are one function at these sizes; this test
    holds that (the kernel's area path is a faster way to the same bytes, and the GPU tests reach both), and keeps the check that
    does tell two functions apart: the mean of converted pixels against the conversion of mean luma."""
    assert ref.linear_table(24, 12, True) == [(2 * d, 2 * d + 1, 1024, 1024) for d in range(12)]
    assert ref.linear_table(16, 8, False) == [(2 * d, 2 * d + 1, 1024, 1024) for d in range(8)]
    planes = yuv_ref.scene_planes(7, 16, 24)
    frame = yuv_ref.planes_to_bgr(*planes)
    assert ref.is_area2(24, 16, 12, 8) and frame.std() > 10
    for f in (frame, ref.bgr(3, 16, 24), ref.bgr(4, 34, 70), np.full((2, 2, 3), 255, np.uint8)):
        h, w = f.shape[:2]
        assert ref.is_area2(w, h, w // 2, h // 2) and (ref.resize_bgr(f, h // 2, w // 2) == ref.forced_linear(f, h // 2, w // 2)).all()
    # a mixed case is linear on both axes, and there the 2 x 2 mean would be wrong
    noise = ref.bgr(5, 6, 7)
    mean = ((noise[0::2, 0:6:2].astype(int) + noise[0::2, 1:6:2] + noise[1::2, 0:6:2] + noise[1::2, 1:6:2] + 2) >> 2).astype(np.uint8)
    assert not ref.is_area2(7, 6, 3, 3) and (ref.resize_bgr(noise, 3, 3) != mean).any()
    # and converting first is not averaging first: the conversion clamps per pixel
    Y, U, V = yuv_ref.planes(5, 16, 24)
    Ym = ((Y[0::2, 0::2].astype(int) + Y[0::2, 1::2] + Y[1::2, 0::2] + Y[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    averaged_first = yuv_ref.planes_to_bgr(np.repeat(np.repeat(Ym, 2, 0), 2, 1), U, V)[0::2, 0::2]
    assert (ref.planes_resized(Y, U, V, 8, 12) != averaged_first).any()


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (16, 24), (37, 53)], ids=str)
def test_the_same_size_gives_the_frame_back(hw):
    h, w = hw
    f = ref.bgr(11, h, w)
    assert (ref.resize_bgr(f, h, w) == f).all()
    assert all(e == (d, min(d + 1, w - 1), 2048, 0) for d, e in enumerate(ingest.resize_table(w, w, True)))
    buf = yuv_ref.frame(12, h, w, "i420")
    assert (ref.to_bgr_resized(buf, h, w, h, w, "i420", "bt709", True) == yuv_ref.to_bgr(buf, h, w, "i420", "bt709", True)).all()


def test_matches_cv2_resize_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    for (h, w), (oh, ow) in (((6, 10), (3, 5)), ((7, 11), (4, 6)), ((36, 52), (18, 26)), ((37, 53), (23, 31)), ((5, 3), (8, 7)), ((9, 9), (3, 3)),
                             ((6, 7), (3, 3))):
        f = np.array(ref.bgr(21, h, w))
        assert (cv2.resize(f, (ow, oh)) == ref.resize_bgr(f, oh, ow)).all(), ((h, w), (oh, ow))


# ---- Stage 2's rectangles in native pixels ----------------------------------------------------------------------------------------------
def det(x1, y1, x2, y2):
    return {"bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}}


def test_rects_for_with_source_hw_against_hand_worked_rectangles():
    b = CropBatcher()                                          # min_crop_size 64, 20 % padding
    dets = [det(100, 100, 140, 150), det(1200, 650, 1280, 720), det(300, 300, 400, 400)]
    # at the detector's size the 40 x 50 box is skipped; the second is 80 x 70: pads 16, 14, clamped at the frame's corner
    assert b.rects_for(dets, (720, 1280)) == ([1, 2], [(1184, 636, 1280, 720), (280, 280, 420, 420)])
    assert b.rects_for(dets, (720, 1280), source_hw=None) == b.rects_for(dets, (720, 1280))
    # at twice the size it is 80 x 100 at (200, 200): pads 16 and 20; the second is 160 x 140 at (2400, 1300): pads 32 and 28, clamped
    # at the NATIVE border; the third 200 x 200 at (600, 600): pads 40
    assert b.rects_for(dets, (720, 1280), source_hw=(1440, 2560)) == ([0, 1, 2], [(184, 180, 296, 320), (2368, 1272, 2560, 1440), (560, 560, 840, 840)])
    # x times 2, y times 3: (10.5, 10.4, 60.5, 40.4) -> (21.0, 31.2.., 121.0, 121.19..) -> ints 21, 31, 121, 121: 100 x 90, pads 20 and 18
    assert b.rects_for([det(10.5, 10.4, 60.5, 40.4)], (100, 200), source_hw=(300, 400)) == ([0], [(1, 13, 141, 139)])
    assert scaled_bbox({"x1": 1, "y1": 2, "x2": 3, "y2": 4}, (100, 200), (300, 400)) == {"x1": 2.0, "y1": 6.0, "x2": 6.0, "y2": 12.0}
    assert dets[0]["bbox"] == {"x1": 100, "y1": 100, "x2": 140, "y2": 150}                 # the detections keep their coordinates


# ---- the capture loop with source_size ----------------------------------------------------------------------------------------------------
SH, SW, TH_, TW_ = 12, 20, 6, 10


def make_capture(streams, **kw):
    popen = FakePopen(streams)
    cap = capture.RTSPStreamCaptureGPU("rtsp://cam/1", queue.Queue(maxsize=100), target_width=TW_, target_height=TH_, camera_id="c1", camera_name="Cam 1",
                                       popen=popen, ingest=ref.RefResizeIngest(), **kw)
    cap.settle_delay = cap.reconnect_delay = cap.error_delay = 0       # no test waits
    popen.cap = cap
    return cap, popen


def test_the_command_has_no_s_with_source_size_and_is_todays_without():
    cap, _ = make_capture([b""], source_size=(SW, SH), use_tcp=True, decoder_args=("-hwaccel", "vaapi"))
    assert cap._build_ffmpeg_command() == ["ffmpeg", "-hwaccel", "vaapi", "-rtsp_transport", "tcp", "-i", "rtsp://cam/1", "-f", "rawvideo", "-pix_fmt", "nv12", "pipe:1"]
    plain, _ = make_capture([b""], use_tcp=True)
    assert plain._build_ffmpeg_command() == ["ffmpeg", "-rtsp_transport", "tcp", "-i", "rtsp://cam/1", "-f", "rawvideo", "-pix_fmt", "nv12", "-s", f"{TW_}x{TH_}", "pipe:1"]
    with pytest.raises(ValueError):
        make_capture([b""], keep_native=True)


@pytest.mark.parametrize("keep_native", [False, True])
def test_native_frames_are_read_and_resized_and_the_native_key_comes_with_keep_native(keep_native):
    import torch
    raw = [yuv_ref.frame(s, SH, SW, "nv12").tobytes() for s in range(3)]
    cap, popen = make_capture([b"".join(raw)], source_size=(SW, SH), keep_native=keep_native)
    cap._capture_loop()
    items = drain(cap.frame_queue)
    assert len(items) == 3 and len(popen.commands) == 1 and "-s" not in popen.commands[0]     # three reads of frame_bytes(SH, SW) each
    assert all(k["sizes"] == [(SH, SW)] and k["out_sizes"] == (TH_, TW_) and bool(k["native_out"]) is keep_native for k in cap._ingest.kwargs)
    for k, it in enumerate(items):
        assert tuple(it) == capture.ITEM_KEYS + (("native_frame",) if keep_native else ())
        assert isinstance(it["frame"], torch.Tensor) and tuple(it["frame"].shape) == (TH_, TW_, 3) and it["frame_id"] == k
        assert (it["frame"].numpy() == ref.to_bgr_resized(raw[k], SH, SW, TH_, TW_)).all()
        if keep_native:
            assert tuple(it["native_frame"].shape) == (SH, SW, 3) and (it["native_frame"].numpy() == yuv_ref.to_bgr(raw[k], SH, SW)).all()
    assert (cap.get_latest_frame().numpy() == ref.to_bgr_resized(raw[2], SH, SW, TH_, TW_)).all()
    if keep_native:
        latest = cap.get_latest_native_frame()
        assert (latest.numpy() == yuv_ref.to_bgr(raw[2], SH, SW)).all() and latest.data_ptr() != items[2]["native_frame"].data_ptr()
    else:
        assert cap.get_latest_native_frame() is None


def test_numpy_copies_of_both_with_keep_frames_on_gpu_off_and_a_short_native_read_is_a_failure():
    raw = [yuv_ref.frame(s, SH, SW, "nv12").tobytes() for s in (5, 6)]
    cap, _ = make_capture([[raw[0], raw[1][:yuv_ref.frame_bytes(TH_, TW_)], raw[1]]], source_size=(SW, SH), keep_native=True, keep_frames_on_gpu=False)
    cap._capture_loop()
    items = drain(cap.frame_queue)
    assert [it["frame_id"] for it in items] == [0, 1] and items[0]["is_gpu_tensor"] is False      # a target-size read is short now
    assert all(type(it["frame"]) is np.ndarray and type(it["native_frame"]) is np.ndarray for it in items)
    assert (items[1]["frame"] == ref.to_bgr_resized(raw[1], SH, SW, TH_, TW_)).all() and (items[1]["native_frame"] == yuv_ref.to_bgr(raw[1], SH, SW)).all()
    assert isinstance(cap.get_latest_native_frame(), np.ndarray)


def test_install_takes_one_source_size_or_one_per_camera():
    main = types.SimpleNamespace(RTSPStreamCapture=object)
    kw = dict(frame_queue=queue.Queue(), target_width=1280, target_height=720, camera_name="Cam", use_tcp=False, buffer_size=None, max_failures=30, retry_delay=5.0)
    capture.install(main, source_size={"c1": (2560, 1440)}, keep_native=True, ingest=ref.RefResizeIngest(), popen=FakePopen([b""]))
    a = main.RTSPStreamCapture(rtsp_url="rtsp://cam/1", camera_id="c1", **kw)
    b = main.RTSPStreamCapture(rtsp_url="rtsp://cam/2", camera_id="c2", **kw)
    assert a.source_size == (2560, 1440) and a.keep_native and "-s" not in a._build_ffmpeg_command()
    assert b.source_size is None and not b.keep_native and b._build_ffmpeg_command()[-3:] == ["-s", "1280x720", "pipe:1"]
    capture.install(main, source_size=(3840, 2160), ingest=ref.RefResizeIngest(), popen=FakePopen([b""]))
    c = main.RTSPStreamCapture(rtsp_url="rtsp://cam/3", camera_id="c3", **kw)
    assert c.source_size == (3840, 2160) and not c.keep_native and "-s" not in c._build_ffmpeg_command() and main._rtd_original_RTSPStreamCapture is object
