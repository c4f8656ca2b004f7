"""The host side of the frame ingest and the capture class, without a GPU: the conversion constants (the restatement's and the
library's own), frame sizes, hand-worked frames against literal BGR values, the relations between the three layouts, what the content
generator promises, and the capture loop of capture.RTSPStreamCaptureGPU with a stand-in for ffmpeg and an ingest that answers from
tests/yuv_ref.py."""
import ctypes as C
import queue
import types

import numpy as np
import pytest

from telescope_cam_detection_amd import _capi, capture, ingest
from tests import yuv_ref as ref

# order CY, CVR, CVG, CUG, CUB
TABLE_LITERALS = {
    ("bt601", False): (1220542, 1673527, -852492, -409993, 2116026),
    ("bt709", False): (1220542, 1880097, -558891, -223347, 2214593),
    ("bt601", True): (1048576, 1470104, -748683, -360710, 1858077),
    ("bt709", True): (1048576, 1651507, -490734, -196084, 1946157),
}


@pytest.mark.parametrize("key", sorted(TABLE_LITERALS))
def test_the_four_tables_are_these_integers_in_the_restatement_and_in_the_library(key):
    matrix, full = key
    assert ref.table(matrix, full) == TABLE_LITERALS[key]
    assert tuple(ingest.tables(ingest.MATRICES[matrix], int(full))) == TABLE_LITERALS[key]


def test_unknown_matrix_or_range_has_no_table():
    L = _capi.lib()
    c = (C.c_int32 * 5)()
    assert L.rtd_debug_ingest_info(2, 0, c, None, None, 0, None, None) == _capi.RTD_E_INVALID
    assert L.rtd_debug_ingest_info(0, 2, c, None, None, 0, None, None) == _capi.RTD_E_INVALID
    assert L.rtd_debug_ingest_info(-1, 0, c, None, None, 0, None, None) == _capi.RTD_E_INVALID


def test_frame_bytes_for_even_and_odd_sizes():
    for h, w, want in ((2, 2, 6), (1, 1, 3), (3, 5, 15 + 2 * 2 * 3), (5, 3, 15 + 2 * 3 * 2), (720, 1280, 1382400), (1080, 1920, 3110400),
                       (1081, 1921, 1081 * 1921 + 2 * 541 * 961)):
        assert ingest.frame_bytes(h, w) == want == ref.frame_bytes(h, w)
        for layout in ref.LAYOUTS:
            assert ref.frame(0, h, w, layout).size == want
    f = ingest.tight_frame(4096, 3, 5, ingest.LAYOUTS["i420"])
    assert (f.y, f.u, f.v, f.y_pitch, f.c_pitch) == (4096, 4096 + 15, 4096 + 15 + 6, 5, 3)
    f = ingest.tight_frame(4096, 3, 5, ingest.LAYOUTS["nv12"])
    assert (f.y, f.u, f.v, f.y_pitch, f.c_pitch) == (4096, 4096 + 15, None, 5, 6)


def test_the_tile_count_of_a_call_is_host_arithmetic():
    th, tw = ingest.tile_hw()
    assert th >= 2 and tw >= 2 and th % 2 == 0 and tw % 2 == 0
    frames = (_capi.RtdYuvFrame * 3)(ingest.tight_frame(256, th, tw, 0), ingest.tight_frame(256, th + 1, tw + 1, 2), ingest.tight_frame(256, 1, 1, 1))
    tiles = C.c_int64()
    assert _capi.lib().rtd_debug_ingest_info(0, 0, None, None, None, 3, frames, C.byref(tiles)) == _capi.RTD_OK
    assert tiles.value == 1 + 4 + 1
    frames[1].width = 65536
    assert _capi.lib().rtd_debug_ingest_info(0, 0, None, None, None, 3, frames, C.byref(tiles)) == _capi.RTD_E_INVALID


# ---- hand-worked frames, BT.601 limited ---------------------------------------------------------------------------------------------------
def test_the_four_spot_colours():
    for yuv, bgr in (((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)),
                     ((41, 240, 110), (255, 0, 0))):
        a = lambda v: np.array([[v]], np.uint8)
        assert tuple(ref.planes_to_bgr(a(yuv[0]), a(yuv[1]), a(yuv[2]))[0, 0]) == bgr


Y2 = np.array([[16, 235], [81, 145]], np.uint8)
WANT2 = np.array([[(0, 0, 179), (178, 179, 255)], [(0, 0, 254), (73, 74, 255)]], np.uint8)       # one block: U = 90, V = 240
Y3 = np.array([[81, 82, 145], [80, 83, 144], [41, 40, 128]], np.uint8)
U3 = np.array([[90, 54], [240, 128]], np.uint8)
V3 = np.array([[240, 34], [110, 128]], np.uint8)
WANT3 = np.array([[(0, 0, 254), (0, 1, 255), (1, 255, 0)], [(0, 0, 253), (1, 2, 255), (0, 254, 0)], [(255, 0, 0), (254, 0, 0), (130, 130, 130)]], np.uint8)
PACKED2 = {"nv12": [16, 235, 81, 145, 90, 240], "nv21": [16, 235, 81, 145, 240, 90], "i420": [16, 235, 81, 145, 90, 240]}
PACKED3 = {"nv12": [81, 82, 145, 80, 83, 144, 41, 40, 128, 90, 240, 54, 34, 240, 110, 128, 128],
           "nv21": [81, 82, 145, 80, 83, 144, 41, 40, 128, 240, 90, 34, 54, 110, 240, 128, 128],
           "i420": [81, 82, 145, 80, 83, 144, 41, 40, 128, 90, 54, 240, 128, 240, 34, 110, 128]}


@pytest.mark.parametrize("layout", ref.LAYOUTS)
def test_a_hand_worked_2x2_and_an_odd_3x3_frame(layout):
    u, v = np.array([[90]], np.uint8), np.array([[240]], np.uint8)
    assert ref.pack(Y2, u, v, layout)[0].tolist() == PACKED2[layout]
    assert (ref.to_bgr(bytes(PACKED2[layout]), 2, 2, layout) == WANT2).all()
    assert ref.pack(Y3, U3, V3, layout)[0].tolist() == PACKED3[layout]
    assert (ref.to_bgr(bytes(PACKED3[layout]), 3, 3, layout) == WANT3).all()


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 5), (5, 3), (6, 10), (37, 53)])
def test_nv21_is_nv12_with_u_and_v_swapped_and_i420_is_nv12_of_the_same_planes(hw):
    h, w = hw
    Y, U, V = ref.planes(11, h, w)
    for key in ref.TABLES:
        want = ref.planes_to_bgr(Y, U, V, *key)
        nv12, i420 = ref.pack(Y, U, V, "nv12")[0], ref.pack(Y, U, V, "i420")[0]
        assert (ref.to_bgr(nv12, h, w, "nv12", *key) == want).all()
        assert (ref.to_bgr(i420, h, w, "i420", *key) == want).all()
        assert (ref.to_bgr(nv12, h, w, "nv21", *key) == ref.planes_to_bgr(Y, V, U, *key)).all()      # the same bytes read as NV21
        assert (ref.to_bgr(ref.pack(Y, U, V, "nv21")[0], h, w, "nv21", *key) == want).all()


def test_padded_pitches_hold_the_same_planes():
    Y, U, V = ref.planes(5, 5, 7)
    for layout in ref.LAYOUTS:
        buf, (oy, ou, ov), (yp, cp) = ref.pack(Y, U, V, layout, y_pitch=7 + 13, c_pitch=8 + 5, fill=0xFF)
        assert (buf[oy:oy + 5 * yp].reshape(5, yp)[:, :7] == Y).all() and (buf[oy:oy + 5 * yp].reshape(5, yp)[:, 7:] == 0xFF).all()
        assert (ov is None) == (layout != "i420")
        assert buf.size == 5 * yp + (3 * cp) * (2 if layout == "i420" else 1)


def test_the_content_meets_both_clamps_in_every_channel_and_tells_the_tables_apart():
    """a frame with at least as many 2 x 2 blocks as the generator has extreme triples; on grey content a comparison proves nothing"""
    for seed, (h, w) in enumerate([(6, 10), (16, 256), (17, 257), (37, 53), (130, 250)]):
        Y, U, V = ref.planes(seed, h, w)
        assert ((h + 1) // 2) * ((w + 1) // 2) >= len(ref._EXTREMES)
        for key in ref.TABLES:
            un = ref.unclamped(Y, U, V, *key)
            for c in range(3):
                assert (un[..., c] < 0).any() and (un[..., c] > 255).any(), (key, c, (h, w))
        imgs = [ref.planes_to_bgr(Y, U, V, *key) for key in ref.TABLES]
        for i in range(4):
            for j in range(i):
                assert (imgs[i] != imgs[j]).any(), (ref.TABLES[i], ref.TABLES[j])
    Ys, Us, Vs = ref.scene_planes(7, 160, 224)
    scene = ref.planes_to_bgr(Ys, Us, Vs)
    assert Ys.shape == (160, 224) and Us.shape == (80, 112) and scene.std() > 10           # a picture, not a flat field


def test_matches_cv2_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    for h, w in ((2, 2), (6, 10), (36, 52)):
        Y, U, V = ref.planes(3, h, w)
        for layout, code in (("nv12", cv2.COLOR_YUV2BGR_NV12), ("nv21", cv2.COLOR_YUV2BGR_NV21), ("i420", cv2.COLOR_YUV2BGR_I420)):
            buf = ref.pack(Y, U, V, layout)[0]
            assert (cv2.cvtColor(buf.reshape(h * 3 // 2, w), code) == ref.to_bgr(buf, h, w, layout)).all()


# ---- the capture loop -----------------------------------------------------------------------------------------------------------------------
H, W = 6, 10
NEED = ref.frame_bytes(H, W)


class FakePipe:
    """reads as a pipe does: up to n bytes of what is left - or, given a list of chunks, one chunk per read (a frame cut short);
    when nothing is left it calls on_empty (the last process of a test stops the loop there) and returns b"" """

    def __init__(self, data, on_empty):
        self.data, self.at, self.on_empty = data, 0, on_empty

    def read(self, n=-1):
        if self.at >= len(self.data):
            self.on_empty()
            return b""
        if isinstance(self.data, list):
            out = self.data[self.at]
            self.at += 1
            return out
        out = self.data[self.at:self.at + n]
        self.at += len(out)
        return out


class FakePopen:
    """subprocess.Popen's call shape; process k serves streams[k]"""

    def __init__(self, streams):
        self.streams, self.commands, self.kwargs, self.procs, self.cap = list(streams), [], [], [], None

    def __call__(self, cmd, **kwargs):
        k = len(self.commands)
        self.commands.append(list(cmd))
        self.kwargs.append(kwargs)
        last = k + 1 >= len(self.streams)
        proc = types.SimpleNamespace(stdout=FakePipe(self.streams[min(k, len(self.streams) - 1)], self.cap.stop_event.set if last else (lambda: None)),
                                     stderr=FakePipe(b"", lambda: None), terminated=0, killed=0)
        proc.poll = lambda: None
        proc.terminate = lambda: setattr(proc, "terminated", proc.terminated + 1)
        proc.kill = lambda: setattr(proc, "killed", proc.killed + 1)
        proc.wait = lambda timeout=None: 0
        self.procs.append(proc)
        return proc


def frames_of(seeds):
    return [ref.frame(s, H, W, "nv12").tobytes() for s in seeds]


def make_capture(streams, qsize=100, **kw):
    popen = FakePopen(streams)
    cap = capture.RTSPStreamCaptureGPU("rtsp://cam/1", queue.Queue(maxsize=qsize), target_width=W, target_height=H, camera_id="c1", camera_name="Cam 1",
                                       popen=popen, ingest=ref.RefIngest(), **kw)
    cap.settle_delay = cap.reconnect_delay = cap.error_delay = 0       # no test waits
    popen.cap = cap
    return cap, popen


def drain(q):
    out = []
    while not q.empty():
        out.append(q.get_nowait())
    return out


def test_good_frames_reach_the_queue_as_the_reference_items():
    import torch
    raw = frames_of(range(4))
    cap, popen = make_capture([b"".join(raw)])
    cap._capture_loop()                                         # (on this thread: it ends when the stand-in's pipe is empty)
    items = drain(cap.frame_queue)
    assert len(items) == 4 and len(popen.commands) == 1 and cap.reconnects == 0 and cap.dropped_frames == 0
    for k, it in enumerate(items):
        assert tuple(it) == capture.ITEM_KEYS
        assert isinstance(it["frame"], torch.Tensor) and it["frame"].dtype == torch.uint8 and tuple(it["frame"].shape) == (H, W, 3)
        assert (it["frame"].numpy() == ref.to_bgr(raw[k], H, W)).all()
        assert it["frame_id"] == k and isinstance(it["timestamp"], float) and it["camera_id"] == "c1" and it["camera_name"] == "Cam 1"
        assert it["is_gpu_tensor"] is True
    latest = cap.get_latest_frame()
    assert (latest.numpy() == ref.to_bgr(raw[3], H, W)).all()
    assert latest.data_ptr() != items[3]["frame"].data_ptr()    # the queued frame is a tensor of its own
    assert (cap.get_latest_frame_as_numpy() == latest.numpy()).all()
    assert cap.frame_id_counter == 4 and set(cap.get_stats()) == {"is_connected", "fps", "total_frames", "dropped_frames", "queue_size"}
    assert popen.kwargs[0]["bufsize"] == 10 ** 8


def test_numpy_frames_with_keep_frames_on_gpu_off():
    raw = frames_of([5, 6])
    cap, _ = make_capture([b"".join(raw)], keep_frames_on_gpu=False)
    cap._capture_loop()
    items = drain(cap.frame_queue)
    assert [type(it["frame"]) for it in items] == [np.ndarray, np.ndarray] and items[0]["is_gpu_tensor"] is False
    assert (items[1]["frame"] == ref.to_bgr(raw[1], H, W)).all() and isinstance(cap.get_latest_frame(), np.ndarray)


def test_a_short_read_in_the_middle_counts_one_failure_and_the_stream_goes_on():
    raw = frames_of(range(3))
    cap, popen = make_capture([[raw[0], raw[1][:-5], raw[1], raw[2]]], max_failures=3)      # a read that comes back 5 bytes short
    cap._capture_loop()
    items = drain(cap.frame_queue)
    assert [it["frame_id"] for it in items] == [0, 1, 2] and cap.reconnects == 0 and len(popen.commands) == 1
    assert (items[1]["frame"].numpy() == ref.to_bgr(raw[1], H, W)).all()


def test_max_failures_short_reads_reconnect_exactly_once_and_frame_ids_go_on():
    raw = frames_of(range(4))
    first = b"".join(raw[:2])                                   # two frames, then the pipe is dry: every read after that is short
    cap, popen = make_capture([first, b"".join(raw[2:])], max_failures=3)
    cap._capture_loop()
    items = drain(cap.frame_queue)
    assert cap.reconnects == 1 and len(popen.commands) == 2
    assert popen.procs[0].terminated == 1 and popen.procs[0].killed == 0
    assert [it["frame_id"] for it in items] == [0, 1, 2, 3]     # monotone across the reconnect
    assert (items[2]["frame"].numpy() == ref.to_bgr(raw[2], H, W)).all()
    assert cap.is_connected and cap.ffmpeg_process is popen.procs[1]
    cap.stop()
    assert cap.ffmpeg_process is None and not cap.is_connected and popen.procs[1].terminated == 1


def test_fewer_short_reads_than_max_failures_do_not_reconnect():
    cap, popen = make_capture([b"\x00" * (NEED - 1)], max_failures=30)
    cap._capture_loop()
    assert cap.reconnects == 0 and len(popen.commands) == 1 and cap.frame_queue.empty() and cap.latest_frame is None


def test_a_full_queue_counts_dropped_frames_and_keeps_the_frame_id():
    raw = frames_of(range(5))
    cap, _ = make_capture([b"".join(raw)], qsize=2)
    cap._capture_loop()
    items = drain(cap.frame_queue)
    assert [it["frame_id"] for it in items] == [0, 1] and cap.dropped_frames == 3 and cap.frame_id_counter == 2
    assert (cap.get_latest_frame().numpy() == ref.to_bgr(raw[4], H, W)).all()     # latest_frame still follows the camera


def test_the_command_has_no_nvidia_flag_and_puts_decoder_args_before_the_input():
    cap, _ = make_capture([b""], decoder_args=("-hwaccel", "vaapi"), use_tcp=True)
    cmd = cap._build_ffmpeg_command()
    assert cmd[0] == "ffmpeg" and not any("cuda" in t or "cuvid" in t for t in cmd)
    i = cmd.index("-i")
    assert cmd[i + 1] == "rtsp://cam/1" and cmd[1:3] == ["-hwaccel", "vaapi"] and cmd.index("-rtsp_transport") < i
    assert cmd[cmd.index("-pix_fmt") + 1] == "nv12" and cmd[cmd.index("-s") + 1] == f"{W}x{H}" and cmd[cmd.index("-f") + 1] == "rawvideo"
    assert cmd[-1] == "pipe:1" and cmd.index("-pix_fmt") > i
    plain, _ = make_capture([b""])
    assert plain._build_ffmpeg_command()[:2] == ["ffmpeg", "-i"]


def test_install_rebinds_the_name_main_builds_with_the_shared_keywords():
    main = types.SimpleNamespace(RTSPStreamCapture=object)
    capture.install(main, decoder_args=("-hwaccel", "vaapi"), ingest=ref.RefIngest(), popen=FakePopen([b""]))
    cap = main.RTSPStreamCapture(rtsp_url="rtsp://cam/2", frame_queue=queue.Queue(), target_width=1280, target_height=720, camera_id="c2",
                                 camera_name="Cam 2", use_tcp=False, buffer_size=None, max_failures=30, retry_delay=5.0)
    assert isinstance(cap, capture.RTSPStreamCaptureGPU) and main._rtd_original_RTSPStreamCapture is object
    assert cap._build_ffmpeg_command()[1:4] == ["-hwaccel", "vaapi", "-i"] and cap.keep_frames_on_gpu and (cap.target_height, cap.target_width) == (720, 1280)
