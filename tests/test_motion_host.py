"""Host side of the empty-frame filter (no GPU): the numpy restatement of OpenCV's arithmetic (tests/motion_ref.py), EmptyFrameFilter on
that restatement, BatchCoordinator's motion gate with a stand-in detector, and the config wiring of make_rtdetr_coordinator."""
import threading
import time

import numpy as np
import pytest

from tests import motion_ref as ref
from telescope_cam_detection_amd import batching
from telescope_cam_detection_amd.batching import BatchCoordinator, make_rtdetr_coordinator
from telescope_cam_detection_amd.motion import EmptyFrameFilter


# ---- the restatement's pinned facts -------------------------------------------------------------------------------------------------
def test_gray_of_pure_colours():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], np.uint8)   # B, G, R, white, black
    assert ref.as_gray(px).tolist() == [[29, 150, 76, 255, 0]]          # (1868|9617|4899 * 255 + 8192) >> 14
    assert ref.as_gray(px[:, :, :1]).tolist() == [[255, 0, 0, 255, 0]]   # C = 1 is already gray
    with pytest.raises(ValueError):
        ref.as_gray(np.zeros((2, 2, 4), np.uint8))


def test_fixed_tables_and_every_kernel_is_symmetric_and_sums_to_256():
    assert ref.taps(1).tolist() == [256]
    assert ref.taps(3).tolist() == [64, 128, 64]
    assert ref.taps(5).tolist() == [16, 64, 96, 64, 16]
    assert ref.taps(7).tolist() == [8, 28, 56, 72, 56, 28, 8]
    for k in range(1, 64, 2):
        c = ref.taps(k)
        assert len(c) == k and c.sum() == 256 and (c == c[::-1]).all() and (c >= 0).all(), k
    # k = 21 (upstream's default), sigma = 3.5
    assert ref.taps(21).tolist() == [0, 2, 2, 4, 6, 11, 15, 20, 25, 28, 30, 28, 25, 20, 15, 11, 6, 4, 2, 2, 0]


def test_tap_rounding_is_far_from_ties_and_where_error_diffusion_matters():
    """motion_ref's docstring, points 1 and 2: which kernels the error-diffused rounding changes, and that no tap of any kernel lies
    close enough to a rounding tie for a last-ulp difference of exp() to flip it"""
    differ = []
    for k in range(9, 64, 2):
        margins = []
        a = ref.taps(k, margins=margins)
        assert min(margins) > 1e-4, k
        if (a != ref.taps(k, diffuse=False)).any():
            differ.append(k)
    assert differ == list(range(13, 64, 2))


def test_constant_frame_stays_constant():
    for k in range(1, 64, 2):
        for v in (0, 1, 128, 255):
            g = np.full((7, 9), v, np.uint8)
            assert (ref.blur(g, k) == v).all(), (k, v)


def test_reflect101_index_maps():
    p = np.arange(-10, 11)
    assert ref.reflect101(p, 1).tolist() == [0] * 21
    assert ref.reflect101(p, 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert ref.reflect101(p, 5).tolist() == [2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2]


def test_matches_cv2_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(0)
    for (h, w), k in (((48, 64), 21), ((31, 17), 5), ((5, 8), 63), ((1, 37), 9), ((40, 40), 13)):
        f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        g = cv2.cvtColor(f, cv2.COLOR_BGR2GRAY)
        assert (ref.as_gray(f) == g).all()
        assert (ref.blur(g, k) == cv2.GaussianBlur(g, (k, k), 0)).all(), (h, w, k)


# ---- EmptyFrameFilter on the numpy backend ------------------------------------------------------------------------------------------
def _filt(**kw):
    kw.setdefault("device", 0)
    be = ref.RefBackend(kw.get("blur_size", 21))
    return EmptyFrameFilter(backend=be, **kw), be


def _frame(seed, h=40, w=48):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_first_frame_stats_and_counting():
    f, _ = _filt(min_motion_area=1, threshold=5, blur_size=3)
    a = _frame(1)
    assert f.has_motion(a) is True                                      # first frame: motion, counted
    assert f.has_motion(a) is False                                     # identical: skipped
    assert f.has_motion(_frame(2)) is True
    s = f.get_stats()
    assert s == {"total_frames": 3, "skipped_frames": 1, "motion_frames": 2, "skip_rate": 1 / 3, "skip_rate_percent": 1 / 3 * 100}
    assert EmptyFrameFilter(device=0, backend=ref.RefBackend(21)).get_stats()["skip_rate"] == 0.0


def test_even_blur_size_is_bumped_and_limits():
    f, _ = _filt(blur_size=20)
    assert f.blur_size == 21
    assert _filt(blur_size=0)[0].blur_size == 1
    with pytest.raises(ValueError):
        EmptyFrameFilter(blur_size=64, device=0, backend=ref.RefBackend(63))


def test_threshold_floor_clamp_and_min_area_is_inclusive():
    a = np.full((10, 10), 100, np.uint8)
    b = a.copy()
    b[:4, :] = 110                                                       # blur k = 1: exact diff of 10 on 40 pixels
    cases = [(9.9, 40), (10, 0), (10.5, 0), (-0.5, 100), (-7, 100), (255, 0), (300, 0)]
    for thr, want in cases:
        be = ref.RefBackend(1)
        f = EmptyFrameFilter(min_motion_area=want if want else 1, threshold=thr, blur_size=1, device=0, backend=be)
        f.has_motion(a)
        got = f.has_motion(b)
        area = ref.motion_area(ref.blur(a, 1), ref.blur(b, 1), thr)
        assert area == want, (thr, area)
        assert got is (want > 0), thr                                    # area >= min_motion_area (= area itself) -> True
    f = EmptyFrameFilter(min_motion_area=41, threshold=9, blur_size=1, device=0, backend=ref.RefBackend(1))
    f.has_motion(a)
    assert f.has_motion(b) is False                                      # 40 < 41


def test_reset_and_size_change_are_first_frames():
    f, be = _filt(min_motion_area=10 ** 9, blur_size=5)
    f.has_motion(_frame(1))
    assert f.has_motion(_frame(2)) is False
    f.reset()
    assert f.has_motion(_frame(3)) is True
    assert f.has_motion(_frame(4, 30, 30)) is True                      # new size: first frame, state replaced
    assert f.has_motion(_frame(5, 30, 30)) is False
    assert f.get_stats()["motion_frames"] == 3


def test_batch_keys_and_per_camera_stats():
    f, be = _filt(min_motion_area=1, threshold=0, blur_size=3)
    a, b = _frame(1), _frame(2)
    assert f.has_motion_batch([a, b, a], ["c0", "c1", None]) == [True, True, True]
    assert be.calls == 1
    assert f.has_motion_batch([a, a, b], ["c0", "c0", "c1"]) == [False, False, False]   # a repeated key: applied in order
    assert f.has_motion_batch([b], [None]) == [True]
    assert f.get_stats("c0")["total_frames"] == 3 and f.get_stats("c0")["skipped_frames"] == 2
    assert f.get_stats()["total_frames"] == 5 and f.get_stats("nope")["total_frames"] == 0
    f.reset("c1")
    assert f.has_motion_batch([b, a], ["c1", "c0"]) == [True, False]                    # c1 starts over, c0 still holds a


# ---- BatchCoordinator with a fake gate --------------------------------------------------------------------------------------------
class _Det:
    def __init__(self, delay=0.0):
        self.seen, self.delay = [], delay

    def detect_batch(self, frames):
        time.sleep(self.delay)
        self.seen.append(list(frames))
        return [[{"frame": f}] for f in frames]


class _Gate:
    """frames are ints: even = static, odd = moving; a camera None is never gated (as EmptyFrameFilter)"""

    def __init__(self):
        self.calls = 0

    def has_motion_batch(self, frames, keys):
        self.calls += 1
        return [k is None or f % 2 == 1 for f, k in zip(frames, keys)]

    def get_stats(self):
        return {"total_frames": self.calls}


def _run(coord, asks, gap=0.0):
    got, done = {}, threading.Event()
    order = []

    def cb(i):
        def f(d):
            got[i] = d
            order.append(i)
            if len(got) == len(asks):
                done.set()
        return f

    with coord:
        for i, (frame, cam) in enumerate(asks):
            coord.infer_async(frame, cb(i), cam)
            if gap:
                time.sleep(gap)
        assert done.wait(10)
    return got, order


def test_static_frames_answered_empty_and_never_detected():
    det, gate = _Det(), _Gate()
    c = BatchCoordinator(det, max_batch_size=4, max_batch_wait_ms=50, empty_frame_filter=gate)
    got, _ = _run(c, [(1, "a"), (2, "b"), (3, "c"), (4, None)])
    assert got[0] == [{"frame": 1}] and got[1] == [] and got[2] == [{"frame": 3}] and got[3] == [{"frame": 4}]
    assert [f for b in det.seen for f in b] == [1, 3, 4]
    st = c.get_stats()
    assert st["empty_frame_filter"] == {"total_frames": gate.calls} and st["total_frames"] == 3
    assert "empty_frame_filter" not in BatchCoordinator(_Det()).get_stats()


def test_all_static_batch_does_not_overtake_a_slow_batch_in_flight():
    det, gate = _Det(delay=0.3), _Gate()
    c = BatchCoordinator(det, max_batch_size=2, max_batch_wait_ms=5, empty_frame_filter=gate, extra_detectors=[_Det(delay=0.3)])
    got, order = _run(c, [(1, "a"), (3, "b"), (2, "a"), (4, "b")], gap=0.05)
    assert got == {0: [{"frame": 1}], 1: [{"frame": 3}], 2: [], 3: []}
    assert order.index(0) < order.index(2) and order.index(1) < order.index(3)      # per camera, in submission order
    assert c.get_stats()["total_frames"] == 2


# ---- make_rtdetr_coordinator --------------------------------------------------------------------------------------------------------
class _CfgDet:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def load_model(self, max_retries=1):
        return True

    def detect_batch(self, frames):
        return [[] for _ in frames]


class _RefCoord:
    def __init__(self, detector, max_batch_size, max_batch_wait_ms, enable_metrics):
        self.detector = detector


def _config(**perf):
    c = {"detection": {"detector_type": "rtdetr", "device": "cuda:0", "batching": {"enabled": True, "max_batch_size": 4}}}
    if perf:
        c["performance"] = perf
    return c


def test_config_key_builds_a_filtered_coordinator(monkeypatch):
    built = {}

    class _F:
        def __init__(self, min_motion_area, threshold, blur_size, device):
            built.update(min_motion_area=min_motion_area, threshold=threshold, blur_size=blur_size, device=device)

    import telescope_cam_detection_amd.motion as motion
    monkeypatch.setattr(motion, "EmptyFrameFilter", _F)
    c = make_rtdetr_coordinator(_config(empty_frame_filter={"enabled": True, "threshold": 30}), coordinator_cls=_RefCoord, detector_cls=_CfgDet)
    assert isinstance(c, BatchCoordinator) and isinstance(c.empty_frame_filter, _F)
    assert built == {"min_motion_area": 200, "threshold": 30, "blur_size": 21, "device": "cuda:0"}


def test_without_the_key_nothing_changes(monkeypatch):
    for cfg in (_config(), _config(empty_frame_filter={"enabled": False, "threshold": 3})):
        c = make_rtdetr_coordinator(cfg, coordinator_cls=_RefCoord, detector_cls=_CfgDet)
        assert type(c) is _RefCoord
    # a filter that cannot be built: logged, served unfiltered
    import telescope_cam_detection_amd.motion as motion

    def boom(**kw):
        raise RuntimeError("no device")
    monkeypatch.setattr(motion, "EmptyFrameFilter", boom)
    c = make_rtdetr_coordinator(_config(empty_frame_filter={"enabled": True}), coordinator_cls=_RefCoord, detector_cls=_CfgDet)
    assert type(c) is _RefCoord
    assert batching.BatchCoordinator is BatchCoordinator
