"""The empty-frame filter on the MI355X (csrc/motion.hip): stored blurred frames bit-identical to the numpy restatement of OpenCV's
arithmetic (tests/motion_ref.py), exact motion areas, batching across cameras, reset / size change, stream ordering of device frames,
and the filtered BatchCoordinator in front of a real detector."""
import threading

import numpy as np
import pytest
import torch

from tests import motion_ref as ref
from telescope_cam_detection_amd.motion import DeviceBackend, EmptyFrameFilter
from telescope_cam_detection_amd.synth import scene_frame

pytestmark = pytest.mark.gpu

SIZES = [(1080, 1920), (720, 1280), (487, 641), (5, 8), (1, 1), (1, 37)]


def _frames(C, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, C), dtype=np.uint8) for h, w in SIZES]


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 21, 31, 63])
def test_stored_state_is_bit_identical_to_the_restatement(k):
    be = DeviceBackend(0, k)
    try:
        for C in (1, 3):
            frames = _frames(C, seed=k * 10 + C)
            want = [ref.blurred(f, k) for f in frames]
            n = len(frames)
            for dev in (False, True):
                slots = list(range(n))
                args = [torch.from_numpy(f).cuda() for f in frames] if dev else frames
                torch.cuda.synchronize()
                be.reset(-1)
                assert be.check(args, dev, slots, 25) == [-1] * n              # one call over six sizes: all first frames
                for s, (f, w) in enumerate(zip(frames, want)):
                    got = be.state(s, w.shape)
                    assert (got == w).all(), (k, C, dev, f.shape, int((got != w).sum()))
    finally:
        be.close()


def _sequence(n=6, h=360, w=640):
    """synth.scene_frame with a moving bright blob and +-3 noise"""
    base = scene_frame(5, h, w).astype(np.int16)
    rng = np.random.default_rng(1)
    out = []
    for t in range(n):
        f = base + rng.integers(-3, 4, base.shape)
        y, x = 40 + 20 * t, 60 + 45 * t
        f[y:y + 50, x:x + 70] = 240
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def test_areas_are_exact_over_a_sequence():
    seq = _sequence()
    blurred = [ref.blurred(f, 21) for f in seq]
    thresholds = [-1, 0, 25, 254, 255]
    be = DeviceBackend(0, 21)
    try:
        for t, f in enumerate(seq):
            for s, thr in enumerate(thresholds):
                got = be.check([f], False, [s], thr)[0]
                want = -1 if t == 0 else ref.motion_area(blurred[t - 1], blurred[t], thr)
                assert got == want, (t, thr, got, want)
        assert be.check([seq[0]], False, [0], -1)[0] == 360 * 640
    finally:
        be.close()


def test_one_call_over_eight_cameras_equals_eight_filters_and_repeated_slots_apply_in_order():
    frames = [[scene_frame(10 + 3 * c + (t if c % 2 else 0), 120 + 8 * c, 200) for c in range(8)] for t in range(3)]
    batch = EmptyFrameFilter(min_motion_area=50, threshold=10, blur_size=21, device=0)
    singles = [EmptyFrameFilter(min_motion_area=50, threshold=10, blur_size=21, device=0) for _ in range(8)]
    for t in range(3):
        got = batch.has_motion_batch(frames[t], [f"cam{c}" for c in range(8)])
        assert got == [singles[c].has_motion(frames[t][c]) for c in range(8)], t
        if t:
            assert got == [bool(c % 2) for c in range(8)]
    for key in ("total_frames", "skipped_frames", "motion_frames"):
        assert batch.get_stats()[key] == sum(s.get_stats()[key] for s in singles), key
    assert batch.get_stats("cam1") == singles[1].get_stats()
    # the same slot three times in one call: applied in order
    be = DeviceBackend(0, 9)
    try:
        a, b, c = (scene_frame(s, 64, 96) for s in (1, 2, 3))
        got = be.check([a, b, c], False, [0, 0, 0], 5)
        ba, bb, bc = (ref.blurred(x, 9) for x in (a, b, c))
        assert got == [-1, ref.motion_area(ba, bb, 5), ref.motion_area(bb, bc, 5)]
        assert (be.state(0, bc.shape) == bc).all()
    finally:
        be.close()


def test_reset_and_size_change_give_first_frames():
    be = DeviceBackend(0, 5)
    try:
        a, b = scene_frame(1, 50, 70), scene_frame(2, 50, 70)
        assert be.check([a, a], False, [0, 1], 0) == [-1, -1]
        assert be.check([a, b], False, [0, 1], 0)[0] == 0
        be.reset(0)
        assert be.check([b, a], False, [0, 1], 0)[0] == -1               # slot 0 reset, slot 1 kept
        be.reset(-1)
        assert be.check([b, b], False, [0, 1], 0) == [-1, -1]
        c = scene_frame(3, 33, 44)
        assert be.check([c], False, [0], 0) == [-1]                      # size change: first frame, new state
        assert (be.state(0, (33, 44)) == ref.blurred(c, 5)).all()
        be.reset(0)
        with pytest.raises(Exception):
            be.state(0, (33, 44))
        with pytest.raises(Exception):
            be.check([np.zeros((4, 4, 2), np.uint8)], False, [0], 0)    # C = 2 is refused (RTD_E_INVALID)
    finally:
        be.close()


def test_device_frames_written_on_torch_stream_just_before_the_call():
    f = EmptyFrameFilter(min_motion_area=1, threshold=0, blur_size=21, device=0)
    big = scene_frame(400, 1080, 1920)
    dev = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    for i in range(4):
        filler = [torch.empty(64 << 20, device="cuda").normal_() for _ in range(4)]   # keeps torch's stream busy ahead of the producer
        view = dev.roll(shifts=37 * (i + 1), dims=1)                                # written on torch's current stream
        f.has_motion_batch([view], ["cam"])
        want = ref.blurred(np.roll(big, 37 * (i + 1), axis=1), 21)
        got = f._backend.state(f._slots["cam"], want.shape)
        assert (got == want).all(), (i, int((got != want).sum()))
        del filler


def test_filtered_coordinator_in_front_of_a_real_detector():
    from telescope_cam_detection_amd.batching import BatchCoordinator
    from telescope_cam_detection_amd.rtdetr_detector import RTDETRDetector
    det = RTDETRDetector(config_path="r18", model_path="synthetic:r18:0", device="cuda:0", conf_threshold=0.0, input_size=(640, 640),
                         wildlife_only=False, max_batch=4)
    assert det.load_model()
    gate = EmptyFrameFilter(device=0)
    coord = BatchCoordinator(det, max_batch_size=4, max_batch_wait_ms=200.0, empty_frame_filter=gate)
    rounds = 4
    frames = [[scene_frame(100 + 10 * c + (t if c < 2 else 0), 480, 640) for c in range(4)] for t in range(rounds)]
    submits0 = det.model.engine.stats()["submits"]
    results = {}
    with coord:
        for t in range(rounds):
            done = threading.Event()

            def cb(d, key):
                results[key] = d
                if sum(1 for k in results if k[0] == key[0]) == 4:
                    done.set()
            for c in range(4):
                coord.infer_async(frames[t][c], lambda d, key=(t, c): cb(d, key), camera_id=f"cam{c}")
            assert done.wait(30.0)
        stats = coord.get_stats()
    ran = det.model.engine.stats()["submits"] - submits0
    assert stats["failed_batches"] == 0 and stats["first_error"] is None, stats
    for t in range(rounds):
        for c in range(4):
            if t > 0 and c >= 2:
                assert results[(t, c)] == [], (t, c)                                   # static after its first frame
            else:
                assert len(results[(t, c)]) > 0 and results[(t, c)] == det.detect(frames[t][c]), (t, c)
    assert stats["total_frames"] == 4 + 2 * (rounds - 1)
    assert ran == stats["total_batches"] >= rounds                                      # one submit per batch that held a moving frame
    assert stats["empty_frame_filter"]["skipped_frames"] == 2 * (rounds - 1)
