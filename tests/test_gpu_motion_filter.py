"""The motion filter on the MI355X (csrc/mog2.hip): the MOG2 model bit-identical to the numpy restatement of OpenCV's arithmetic
(tests/mog2_ref.py) after every call, exact foreground masks and box counts for many boxes per call, fused updates equal to single
ones, numpy / host-tensor / device-tensor frames, stream ordering, re-initialisation, and two filters on two threads."""
import threading

import numpy as np
import pytest
import torch

from tests import mog2_ref as ref
from telescope_cam_detection_amd.motion_filter import DeviceBackend, MotionFilter

pytestmark = pytest.mark.gpu


def _same(got: dict, want: dict, where=""):
    assert got is not None and want is not None, where
    for k in ("weight", "variance", "mean", "modes_used"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (where, k, a.shape, b.shape)
        bad = (a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else (a != b)
        assert not bad.any(), (where, k, int(bad.sum()), np.argwhere(bad)[:3].tolist())
    assert got["nframes"] == want["nframes"], where


def _fg(masks, shape) -> np.ndarray:
    """the words rtd_debug_mog2_fg_bits returns for these masks"""
    words = np.zeros(((len(masks) + 31) // 32,) + tuple(shape), np.uint32)
    for i, m in enumerate(masks):
        words[i // 32] |= (m == 255).astype(np.uint32) << np.uint32(i % 32)
    return words


def _rects(rng, h, w, n):
    edges = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, w, h), (0, max(0, h - 5), min(w, 7), h), (max(0, w - 9), 0, w, min(h, 4)),
             (min(3, w), min(3, h), min(3, w), h)]                  # the last one is empty
    out = []
    for i in range(n):
        if i < len(edges):
            out.append(edges[i])
            continue
        x1, x2 = sorted(rng.integers(0, w + 1, 2))
        y1, y2 = sorted(rng.integers(0, h + 1, 2))
        out.append((int(x1), int(y1), int(x2), int(y2)))
    return out


@pytest.mark.parametrize("h,w,C,shadows,history,frames", [
    (1080, 1920, 3, True, 500, 2),
    (487, 641, 3, False, 3, 3),
    (487, 641, 1, True, 500, 3),
    (5, 8, 3, True, 3, 40),
    (5, 8, 1, False, 500, 40),
    (1, 1, 3, True, 500, 30),
    (1, 1, 1, True, 3, 30),
])
def test_model_and_masks_are_bit_identical_to_the_restatement(h, w, C, shadows, history, frames):
    rng = np.random.default_rng(h * w + C)
    seq = ref.sequence(h, w, C, frames, seed=C)
    if h * w < 100:                                                    # tiny frames: noise as well, for many modes and prunes
        seq = [f if t % 4 else rng.integers(0, 256, f.shape, dtype=np.uint8) for t, f in enumerate(seq)]
    be = DeviceBackend(0, history, 16, shadows)
    mog = ref.Mog2(history, 16, shadows)
    try:
        for t, f in enumerate(seq):
            counts = be.apply(f, False, [(0, 0, w, h)], 21)
            mask = mog.apply(f)
            _same(be.model(), mog.model(), (h, w, C, t))
            assert (be.fg_bits(1, (h, w)) == _fg([mask], (h, w))).all(), t
            assert counts == [ref.box_count(ref.motion_map(mask, 21), (0, 0, w, h))], t
    finally:
        be.close()


@pytest.mark.parametrize("k", [1, 3, 5, 21, 63])
def test_counts_are_exact_for_many_boxes_per_call(k):
    h, w = 61, 97
    rng = np.random.default_rng(k)
    seq = ref.sequence(h, w, 3, 7, seed=k)
    # the first call's 250 updates settle the model (lr = 1 / 500 after it): every later update of a frame then still sees that frame's
    # motion, where a young model learns a frame within two updates and calls a new object a shadow of its own new mode
    ns = (250, 1, 7, 0, 32, 33, 70)
    be = DeviceBackend(0, 500, 16, True)
    mog = ref.Mog2(500, 16, True)
    try:
        for t, (f, n) in enumerate(zip(seq, ns)):
            rects = _rects(rng, h, w, n)
            before = be.model()
            got = be.apply(f, False, rects, k)
            if n == 0:                                                 # no update at all
                assert got == [] and be.model()["nframes"] == before["nframes"]
                _same(be.model(), mog.model())
                continue
            masks = [mog.apply(f) for _ in range(n)]
            want = [ref.box_count(ref.motion_map(m, k), r) for m, r in zip(masks, rects)]
            assert got == want, (n, [i for i in range(n) if got[i] != want[i]][:5])
            assert (be.fg_bits(n, (h, w)) == _fg(masks, (h, w))).all(), n
            _same(be.model(), mog.model(), n)
            if t > 0 and n > 1:
                assert sum(1 for c in got if c) >= 3, (n, got)         # the boxes do see motion
    finally:
        be.close()


def test_n_updates_in_one_call_equal_n_calls_of_one_box():
    h, w = 120, 160
    seq = ref.sequence(h, w, 3, 4, seed=9)
    rects = _rects(np.random.default_rng(9), h, w, 45)
    fused, single = DeviceBackend(0, 500, 16, True), DeviceBackend(0, 500, 16, True)
    try:
        for f in seq:
            a = fused.apply(f, False, rects, 21)
            b = [single.apply(f, False, [r], 21)[0] for r in rects]
            assert a == b
            _same(fused.model(), single.model())
    finally:
        fused.close()
        single.close()


def _dets(h, w):
    boxes = [(0, 0, w, h), (w * 0.1, h * 0.2, w * 0.6, h * 0.7), (w * 0.5, h * 0.5, w * 1.2, h * 1.1), (-4, -4, 30.5, 20.5),
             (w * 0.3, h * 0.1, w * 0.2, h * 0.05)]
    return [{"class_name": "bird", "confidence": 0.9, "bbox": {"x1": a, "y1": b, "x2": c, "y2": d}} for a, b, c, d in boxes]


def test_numpy_host_tensor_and_device_tensor_frames_agree():
    h, w = 240, 320
    seq = ref.sequence(h, w, 3, 5, seed=4)
    filters = [MotionFilter(device=0, history=50) for _ in range(3)]
    for f in seq:
        dev = torch.from_numpy(f).cuda()
        outs = [m.filter_detections(x, _dets(h, w)) for m, x in zip(filters, (f, torch.from_numpy(f), dev))]
        assert outs[0] == outs[1] == outs[2]
    models = [m.bg_subtractor.model() for m in filters]
    _same(models[1], models[0])
    _same(models[2], models[0])
    assert filters[0].get_stats() == filters[2].get_stats()
    for m in filters:
        m.cleanup()


def test_device_frame_written_on_another_stream_is_waited_for():
    h, w = 1080, 1920
    base = ref.sequence(h, w, 3, 1, seed=11)[0]
    src = torch.from_numpy(base).cuda()
    torch.cuda.synchronize()
    m = MotionFilter(device=0, history=500, detect_shadows=False)
    mog = ref.Mog2(500, 16, False)
    side = torch.cuda.Stream()
    box = [{"bbox": {"x1": 0, "y1": 0, "x2": w, "y2": h}}]
    for i in range(2):
        with torch.cuda.stream(side):
            filler = [torch.empty(64 << 20, device="cuda").normal_() for _ in range(4)]   # keeps the producer's stream busy
            frame = src.roll(shifts=53 * (i + 1), dims=1)                                 # written on `side`, the current stream
            m.filter_detections(frame, [dict(b) for b in box])
            del filler
        mog.apply(np.roll(base, 53 * (i + 1), axis=1))
        _same(m.bg_subtractor.model(), mog.model(), i)
    m.cleanup()


def test_size_change_reinitialises_and_configure_resets():
    be = DeviceBackend(0, 500, 16, True)
    try:
        a, b = ref.sequence(20, 30, 3, 3, seed=1), ref.sequence(21, 30, 3, 1, seed=2)[0]
        for f in a:
            be.apply(f, False, [(0, 0, 30, 20)], 5)
        assert be.model()["nframes"] == 3
        be.apply(b, False, [(0, 0, 30, 21)], 5)                       # a new size: a new model
        mog = ref.Mog2()
        mog.apply(b)
        _same(be.model(), mog.model())
        g = np.ascontiguousarray(b[:, :, :1])
        be.apply(g, False, [(0, 0, 30, 21)], 5)                       # a new channel count too
        mog = ref.Mog2()
        mog.apply(g)
        _same(be.model(), mog.model())
        be.configure(3, 25.0, False)                                  # a new subtractor: no model until the next update
        assert be.model() is None
        be.apply(b, False, [(0, 0, 30, 21)], 5)
        mog = ref.Mog2(3, 25.0, False)
        mog.apply(b)
        _same(be.model(), mog.model())
        with pytest.raises(Exception):
            be.apply(b, False, [(0, 0, 31, 21)], 5)                   # boxes must be clamped (RTD_E_INVALID)
        with pytest.raises(Exception):
            be.apply(b, False, [(0, 0, 30, 21)], 65)
        with pytest.raises(Exception):
            be.configure(0, 16.0, True)
        _same(be.model(), mog.model())                                # refused calls change nothing
    finally:
        be.close()


def test_two_filters_on_two_threads_equal_serial_runs():
    h, w = 96, 128
    seqs = [ref.sequence(h, w, 3, 12, seed=s) for s in (21, 22)]

    def run(seq, out):
        m = MotionFilter(device=0, history=30)
        out.append([m.filter_detections(f, _dets(h, w)) for f in seq])
        out.append(m.bg_subtractor.model())
        m.cleanup()

    serial = [[], []]
    for s, o in zip(seqs, serial):
        run(s, o)
    threaded = [[], []]
    ts = [threading.Thread(target=run, args=(s, o)) for s, o in zip(seqs, threaded)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    for a, b in zip(serial, threaded):
        assert len(b) == 2 and a[0] == b[0]
        _same(b[1], a[1])
