"""Host side of the motion filter (no GPU): the numpy restatement of OpenCV's MOG2 (tests/mog2_ref.py) checked against its literal
scalar transcription and against the model's known properties, and MotionFilter / AdaptiveMotionFilter on that restatement (RefBackend):
early returns, one update per detection, the decision rules, box handling, hot reload and install()."""
import types

import numpy as np
import pytest

from tests import mog2_ref as ref
from telescope_cam_detection_amd import motion_filter as mf
from telescope_cam_detection_amd.motion_filter import AdaptiveMotionFilter, MotionFilter


def _same(a: dict, b: dict):
    for k in ("weight", "variance", "mean", "modes_used"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k
    assert a["nframes"] == b["nframes"]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("history", [3, 500])
def test_scalar_and_vectorised_restatements_agree_bit_for_bit(C, shadows, history):
    rng = np.random.default_rng(C + 10 * history)
    seq = ref.sequence(9, 11, C, 24, seed=C)
    seq += [rng.integers(0, 256, (9, 11, C), dtype=np.uint8) for _ in range(8)]       # many modes, prunes and replacements
    seq += [seq[0]] * 4
    a, b = ref.Mog2(history, 16, shadows), ref.Mog2Scalar(history, 16, shadows)
    seen, most = set(), 0
    for t, f in enumerate(seq):
        ma, mb = a.apply(f), b.apply(f)
        assert (ma == mb).all(), t
        _same(a.model(), b.model())
        seen |= set(np.unique(ma).tolist())
        most = max(most, int(a.model()["modes_used"].max()))
    assert most >= 4                                                     # the replace-the-weakest path is exercised
    assert {0, 127 if shadows else 255} <= seen <= {0, 127, 255}


@pytest.mark.parametrize("shadows", [True, False])
def test_first_frame_and_static_scene(shadows):
    f = ref.sequence(8, 10, 3, 1)[0]
    f[0, :3] = 0
    m = ref.Mog2(500, 16, shadows)
    mask = m.apply(f)
    # no model yet: nothing is background.  The shadow test runs on the updated model, where the pixel's only mode is the pixel itself
    # (a = 1, distortion 0): with shadows on the first frame is all shadow, except black pixels (den = 0), so MotionFilter sees no motion.
    assert (mask[0, :3] == 255).all() and (mask.ravel()[3:] == (127 if shadows else 255)).all()
    st = m.model()
    assert (st["modes_used"] == 1).all() and st["nframes"] == 1
    assert (st["weight"][..., 0] == 1).all() and (st["weight"][..., 1:] == 0).all()
    assert (st["variance"][..., 0] == 15).all() and (st["mean"][..., 0, :] == f).all()
    for _ in range(3):
        assert (m.apply(f) == 0).all()                                  # background from the second frame on
    assert (m.model()["modes_used"] == 1).all()


@pytest.mark.parametrize("history", [1, 3, 500])
def test_learning_rate_schedule(history):
    for n in range(1, 700, 7):
        a, a1, pr = ref.rates(n, history)
        lr = 1.0 / min(2 * n, history)
        assert a == np.float32(lr) and a1 == np.float32(1) - np.float32(lr) and pr == np.float32(-lr * float(np.float32(0.05)))
    # second frame of another value: the old mode decays by alpha1, the new one enters with alphaT (history 1: the old one is pruned and
    # the zero total leaves the new mode alone, with weight 1)
    m = ref.Mog2(history)
    m.apply(np.full((2, 3), 10, np.uint8))
    m.apply(np.full((2, 3), 200, np.uint8))
    st = m.model()
    a, a1, _ = ref.rates(2, history)
    if history == 1:
        assert (st["modes_used"] == 1).all() and (st["weight"][..., 0] == 1).all() and (st["mean"][..., 0, 0] == 200).all()
    else:
        assert (st["modes_used"] == 2).all()
        w = sorted([a1, a], reverse=True) if a1 != a else [a, a1]
        assert (st["weight"][..., 0] == w[0]).all() and (st["weight"][..., 1] == w[1]).all()
        assert (st["mean"][..., 0, 0] == (200 if a >= a1 else 10)).all()   # a tie sorts the new mode first


def test_model_invariants_over_a_long_sequence():
    rng = np.random.default_rng(3)
    seq = ref.sequence(16, 20, 3, 40, seed=3) + [rng.integers(0, 256, (16, 20, 3), dtype=np.uint8) for _ in range(10)]
    for history in (3, 500):
        m = ref.Mog2(history)
        for f in seq:
            m.apply(f)
            st = m.model()
            n = st["modes_used"].astype(int)
            assert 1 <= n.min() and n.max() <= 5
            used = np.arange(5)[None, None, :] < n[..., None]
            v = st["variance"][used]
            assert (v >= 4).all() and (v <= 75).all()
            w = np.where(used, st["weight"], 0)
            tot = w.sum(-1)
            # renormalised, except where a sixth mode replaced the weakest (its weight is dropped, the rest scaled by alpha1) or every
            # mode was pruned (a zero total leaves the weights at 0 and the new mode enters with alphaT)
            a, _, _ = ref.rates(m.nframes, history)
            pruned_out = ((w > 0).sum(-1) == 1) & (w.max(-1) == a)
            assert (np.abs(tot - 1) < 1e-5)[(n < 5) & ~pruned_out].all()
            w = np.where(used, st["weight"], -1)
            assert (np.diff(w, axis=-1)[used[..., 1:]] <= 0).all()    # sorted by weight


@pytest.mark.parametrize("C", [1, 3])
def test_shadow_values(C):
    bg = np.full((6, 8, C), 200, np.uint8)
    dark = bg.copy()
    dark[:, :4] = 120                                                   # 0.6 of the background: a shadow
    dark[:, 4:] = 60                                                    # 0.3: below tau, foreground
    for shadows, want in ((True, 127), (False, 255)):
        m = ref.Mog2(500, 16, shadows)
        for _ in range(8):
            m.apply(bg)
        mask = m.apply(dark)
        assert (mask[:, :4] == want).all() and (mask[:, 4:] == 255).all(), shadows


def test_matches_cv2_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    for C, shadows, history in ((3, True, 500), (1, True, 3), (3, False, 20)):
        seq = ref.sequence(48, 64, C, 20, seed=C)
        ours = ref.Mog2(history, 16, shadows)
        theirs = cv2.createBackgroundSubtractorMOG2(history=history, varThreshold=16, detectShadows=shadows)
        for t, f in enumerate(seq):
            a = ours.apply(f)
            b = theirs.apply(f if C == 3 else f[:, :, 0])
            assert (a == b).all(), (C, shadows, history, t, int((a != b).sum()))
            for k in (1, 21, 63):
                fg = cv2.threshold(b, 200, 255, cv2.THRESH_BINARY)[1]
                got = cv2.threshold(cv2.GaussianBlur(fg, (k, k), 0), 25, 255, cv2.THRESH_BINARY)[1] > 0
                assert (got == ref.motion_map(a, k)).all(), (t, k)


# ---- MotionFilter on the restatement --------------------------------------------------------------------------------------------------
def _filter(**kw):
    be = ref.RefBackend(kw.get("history", 500), kw.get("var_threshold", 16), kw.get("detect_shadows", True))
    return MotionFilter(device=0, backend=be, **kw), be


def _det(x1, y1, x2, y2, name="bird"):
    return {"class_name": name, "confidence": 0.8, "bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}}


def test_early_returns_do_not_touch_the_model():
    f = ref.sequence(20, 30, 3, 1)[0]
    m, be = _filter(motion_required=False)
    dets = [_det(0, 0, 10, 10)]
    assert m.filter_detections(f, dets) is dets and be.calls == 0 and "has_motion" not in dets[0]
    assert m.get_stats() == {"total_frames": 0, "total_detections_filtered": 0, "motion_required": False}
    m, be = _filter()
    empty = []
    assert m.filter_detections(f, empty) is empty and be.calls == 0 and m.get_stats()["total_frames"] == 0


def test_n_detections_make_n_updates_in_one_call_and_match_the_chain():
    seq = ref.sequence(40, 60, 3, 6, seed=5)
    m, be = _filter(history=20)
    mog = ref.Mog2(20)
    boxes = [(0, 0, 60, 40), (10.7, 5.2, 30.9, 25.0), (50, 30, 80, 90), (-5, -5, 12, 9), (30, 20, 10, 2), (100, 100, 120, 120)]
    kept = 0
    for t, f in enumerate(seq):
        dets = [_det(*b) for b in boxes]
        out = m.filter_detections(f, [dict(d) for d in dets])
        assert be.calls == t + 1 and be.updates == (t + 1) * len(boxes)
        want = []
        for d in dets:
            mask = mog.apply(f)
            rect = mf.roi(d["bbox"], 40, 60)
            c = ref.box_count(ref.motion_map(mask, 21), rect)
            area = max(rect[2] - rect[0], 0) * max(rect[3] - rect[1], 0)
            if area and c >= 10 and c / area > 0.05:
                want.append((d["bbox"], c / area))
        assert [(d["bbox"], d["motion_ratio"]) for d in out] == want, t
        assert all(d["has_motion"] is True and isinstance(d["motion_ratio"], float) for d in out)
        _same(be.model(), mog.model())
        kept += len(want)
    assert 0 < kept < len(seq) * len(boxes)
    assert m.get_stats() == {"total_frames": len(seq), "total_detections_filtered": len(seq) * len(boxes) - kept, "motion_required": True}


def test_decision_rules_boxes_and_empty_rois():
    bg = np.full((30, 40, 3), 100, np.uint8)
    f = bg.copy()
    f[:20, :20] = 255                                                     # a white block on a learned background
    m, be = _filter(detect_shadows=False)
    whole = {"x1": 0, "y1": 0, "x2": 40, "y2": 30}
    assert m.has_motion_in_bbox(bg, whole) == (True, 1.0)                 # the first frame is all foreground without shadows
    for _ in range(59):                                                   # lr = 1 / 120 by then: the block stays foreground for 10 updates
        assert m.has_motion_in_bbox(bg, whole) == (False, 0.0)
    be.updates = 0
    assert mf.roi({"x1": 20, "y1": 9, "x2": 10, "y2": 3}, 30, 40) == (10, 3, 20, 9)          # inverted corners are swapped
    assert mf.roi({"x1": -5.5, "y1": -0.5, "x2": 3.9, "y2": 2.99}, 30, 40) == (0, 0, 3, 2)  # int() truncates towards zero, then clamp
    assert mf.roi({"x1": 5, "y1": 5, "x2": 5, "y2": 5}, 30, 40) == (5, 5, 6, 6)              # min size 1
    assert mf.roi({"x1": 38, "y1": 0, "x2": 90, "y2": 99}, 30, 40) == (38, 0, 40, 30)
    assert mf.roi({"x1": 45, "y1": 0, "x2": 50, "y2": 10}, 30, 40) == (45, 0, 40, 10)        # empty after the clamp
    dets = [_det(0, 0, 3, 3), _det(0, 0, 2, 5), _det(45, 0, 50, 10), _det(5, 5, 15, 15), _det(25, 22, 40, 30)]
    out = m.filter_detections(f, dets)
    assert be.updates == 5                                                # the empty box still updated the model
    assert [d["bbox"]["x2"] for d in out] == [2, 15]                      # 9 pixels < 10; exactly 10 passes; empty -> False; static
    assert out[0]["motion_ratio"] == 1.0 and out[1]["motion_ratio"] == 1.0
    assert m.get_stats() == {"total_frames": 1, "total_detections_filtered": 3, "motion_required": True}
    assert m.has_motion_in_bbox(f, {"x1": 45, "y1": 0, "x2": 50, "y2": 10}) == (False, 0.0) and be.updates == 6
    strict, _ = _filter(min_motion_ratio=1.0, detect_shadows=False)
    assert strict.filter_detections(f, [_det(0, 0, 10, 10)]) == []       # ratio 1.0 is not > 1.0
    assert strict.has_motion_in_bbox(ref.sequence(30, 40, 1, 1)[0][:, :, 0], {"x1": 0, "y1": 0, "x2": 4, "y2": 4},
                                     min_motion_pixels=16) == (False, 1.0)


def test_update_params_recreate_rules_reset_and_cleanup():
    f = ref.sequence(20, 30, 3, 1)[0]
    m, be = _filter()
    m.filter_detections(f, [_det(0, 0, 5, 5)])
    for cfg in ({"motion_blur_size": 8}, {"min_motion_ratio": 0.2}, {"min_motion_area": 5}, {"history": 500}, {"motion_required": False}):
        m.update_params(cfg)
        assert be.configures == 0 and be.model() is not None, cfg
    assert m.motion_blur_size == 9 and m.min_motion_ratio == 0.2 and m.min_motion_area == 5 and m.motion_required is True
    for i, cfg in enumerate(({"history": 200}, {"var_threshold": 25}, {"detect_shadows": False})):
        m.update_params(cfg)
        assert be.configures == i + 1 and be.model() is None, cfg
        m.filter_detections(f, [_det(0, 0, 5, 5)])
    assert (be.mog.history, be.mog.tb, be.mog.shadows) == (200, 25, False)
    m.reset_background()
    assert be.configures == 4 and be.model() is None
    with pytest.raises(ValueError):
        m.update_params({"motion_blur_size": 64})                         # 65 taps: deliberate deviation
    with pytest.raises(ValueError):
        m.update_params({"history": 0})
    assert m.history == 200 and m.motion_blur_size == 9
    m.cleanup()
    assert be.closed and m.bg_subtractor is None
    m.cleanup()


def test_deliberate_deviations_raise():
    for kw in ({"motion_blur_size": 64}, {"motion_blur_size": -3}, {"history": 0}, {"history": -5}, {"history": 2.5}):
        with pytest.raises(ValueError):
            _filter(**kw)
    m, _ = _filter(motion_blur_size=20)
    assert m.motion_blur_size == 21 and _filter(motion_blur_size=0)[0].motion_blur_size == 1 and _filter(motion_blur_size=63)[0].motion_blur_size == 63


def test_adaptive_threshold_follows_the_clock(monkeypatch):
    hour = {"h": 12}

    class Clock:
        @staticmethod
        def now():
            return types.SimpleNamespace(hour=hour["h"])
    monkeypatch.setattr(mf, "datetime", Clock)
    be = ref.RefBackend()
    a = AdaptiveMotionFilter(device=0, backend=be, history=50)
    assert a.var_threshold == 16 and a.history == 50
    f = ref.sequence(20, 30, 3, 1)[0]
    a.filter_detections(f, [_det(0, 0, 5, 5)])
    assert be.configures == 0
    hour["h"] = 22
    a.filter_detections(f, [_det(0, 0, 5, 5)])
    assert be.configures == 1 and a.var_threshold == 32 and be.mog.tb == 32 and be.mog.nframes == 1
    a.filter_detections(f, [_det(0, 0, 5, 5)])
    assert be.configures == 1
    hour["h"] = 6
    a.filter_detections(f, [])
    assert be.configures == 2 and a.var_threshold == 16


def test_install_on_a_stand_in_module():
    dp = types.SimpleNamespace(MotionFilter=object)
    mf.install(dp)
    assert dp.MotionFilter is MotionFilter
