"""YOLOX post-processing without a GPU: the restatement (tests/yolox_ref.py) against two independently written versions, the margin
conditions of every seeded input the GPU tests use, the pure-host entry points and refusals of rtd_yolox_post_*, and YOLOXDetector on the
numpy back end with a stand-in network.

The margin conditions are conditions on the INPUTS, not tolerances: the device evaluates every same-class candidate pair in fp32, so no
pair's fp64 IoU may lie within 1e-5 of the threshold (the fp32 IoU of coordinates below 200 carries a few ulp, about 5e-7; this is 20
times that), no row's score within 1e-5 of the confidence threshold, and fp32 and fp64 must keep the same rows."""
import ctypes as C
import logging
import sys
import types

import numpy as np
import pytest

from telescope_cam_detection_amd import _capi, yolox_detector as yd
from telescope_cam_detection_amd.coco_constants import COCO_CLASSES, WILDLIFE_CLASSES
from tests import yolox_ref as ref

CONF, NMS = ref.CONF, ref.NMS
MARGIN = 1e-5


# ---- the restatement against two other ways of writing it ---------------------------------------------------------------------------
def per_class_loop(pred, conf, nms):
    """fp64, class by class: anchors kept, in output order"""
    p = np.asarray(pred, np.float64)
    cid = p[:, 5:].argmax(1)
    score = p[:, 4] * p[:, 5:].max(1)
    kept = []
    for c in np.unique(cid):
        idx = [a for a in range(len(p)) if cid[a] == c and score[a] >= conf]
        idx.sort(key=lambda a: (-score[a], a))
        dead = set()
        for pos, a in enumerate(idx):
            if a in dead:
                continue
            kept.append(a)
            ax1, ay1, ax2, ay2 = p[a, 0] - p[a, 2] / 2, p[a, 1] - p[a, 3] / 2, p[a, 0] + p[a, 2] / 2, p[a, 1] + p[a, 3] / 2
            for b in idx[pos + 1:]:
                bx1, by1, bx2, by2 = p[b, 0] - p[b, 2] / 2, p[b, 1] - p[b, 3] / 2, p[b, 0] + p[b, 2] / 2, p[b, 1] + p[b, 3] / 2
                inter = max(0.0, min(ax2, bx2) - max(ax1, bx1)) * max(0.0, min(ay2, by2) - max(ay1, by1))
                union = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter
                if union > 0 and inter / union > nms:
                    dead.add(b)
    kept.sort(key=lambda a: (-score[a], a))
    return kept


def torch_offset_trick(pred, conf, nms):
    """torchvision's other batched_nms: boxes of class c moved by c * (largest coordinate + 1), then one class-blind NMS; torch, fp64"""
    import torch
    p = torch.from_numpy(np.asarray(pred, np.float64))
    cconf, cid = p[:, 5:].max(1)
    score = p[:, 4] * cconf
    idx = torch.nonzero(score >= conf).flatten()
    boxes = torch.stack([p[idx, 0] - p[idx, 2] / 2, p[idx, 1] - p[idx, 3] / 2, p[idx, 0] + p[idx, 2] / 2, p[idx, 1] + p[idx, 3] / 2], 1)
    boxes = boxes + (cid[idx].to(boxes) * (boxes.max() + 1))[:, None]
    order = sorted(range(len(idx)), key=lambda k: (-float(score[idx[k]]), int(idx[k])))
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    kept = []
    for k in order:
        ok = True
        for j in kept:
            lt, rb = torch.maximum(boxes[k, :2], boxes[j, :2]), torch.minimum(boxes[k, 2:], boxes[j, 2:])
            wh = (rb - lt).clamp(min=0)
            inter = wh[0] * wh[1]
            if float(inter / (area[k] + area[j] - inter)) > nms:
                ok = False
                break
        if ok:
            kept.append(k)
    return [int(idx[k]) for k in kept]


def images():
    for name, *_ in ref.SEEDED:
        for i, img in enumerate(ref.seeded(name)):
            yield f"{name}[{i}]", img


@pytest.mark.parametrize("name", [s[0] for s in ref.SEEDED])
def test_the_restatement_equals_a_per_class_loop_and_the_offset_trick(name):
    for img in ref.seeded(name):
        rows, passed, kept = ref.postprocess(img, CONF, NMS, np.float64)
        assert list(kept) == per_class_loop(img, float(np.float32(CONF)), float(np.float32(NMS)))
        assert list(kept) == torch_offset_trick(img, float(np.float32(CONF)), float(np.float32(NMS)))
        assert len(rows) == len(kept) and passed >= len(kept)
        # rows: corners of the kept anchors, obj, the class maximum and its index, score descending
        p = img.astype(np.float64)
        assert (rows[:, 4] == p[kept, 4]).all() and (rows[:, 5] == p[kept, 5:].max(1)).all() and (rows[:, 6] == p[kept, 5:].argmax(1)).all()
        assert (np.diff(rows[:, 4] * rows[:, 5]) <= 0).all()


def test_the_seeded_shapes_give_the_candidate_counts_the_gpu_tests_count_on():
    want = {"a126_c80": 30, "a126_c3": 96, "a504_c80": 300, "a126_cut": 100}
    for name, *_ in ref.SEEDED:
        for img in ref.seeded(name):
            rows, passed, kept = ref.postprocess(img, CONF, NMS)
            assert passed == want[name]
            assert 6 <= len(kept) <= 42, (name, len(kept))


def check_margins(label, img, **kw):
    d_iou, d_score = ref.margins(img, CONF, NMS, **kw)
    print(f"{label}: min |IoU - {NMS}| over same-class candidate pairs {d_iou:.3e}, min |score - {CONF}| {d_score:.3e}")
    assert d_iou >= MARGIN and d_score >= MARGIN, (label, d_iou, d_score)
    r32, p32, k32 = ref.postprocess(img, CONF, NMS, np.float32, **kw)
    r64, p64, k64 = ref.postprocess(img, CONF, NMS, np.float64, **kw)
    assert p32 == p64 and list(k32) == list(k64), label


def test_margin_conditions_hold_for_every_seeded_input():
    for label, img in images():
        check_margins(label, img)
    check_margins("a126_cut at 64", ref.seeded("a126_cut")[0], max_candidates=ref.CUT)
    check_margins("a126_c80 wildlife", ref.seeded("a126_c80")[0], class_keep=sorted(WILDLIFE_CLASSES))
    for i, img in enumerate(wildlife_pred()):                # what the detector tests feed, with the class filter and without
        check_margins(f"wildlife variant[{i}]", img)
        check_margins(f"wildlife variant[{i}] filtered", img, class_keep=sorted(WILDLIFE_CLASSES))


@pytest.mark.parametrize("name", [s[0] for s in ref.HEAD_SEEDED])
def test_margin_conditions_hold_for_the_decoded_head_inputs(name):
    pred, in_hw = ref.head_seeded(name)
    assert pred.shape[1] == ref.anchors(*in_hw)
    assert pred[:, :, 2:4].min() >= -1.0 and pred[:, :, 2:4].max() <= 2.0
    for i, img in enumerate(pred):
        check_margins(f"{name}[{i}]", img, in_hw=in_hw)
        rows, passed, kept = ref.postprocess(img, CONF, NMS, np.float64, in_hw=in_hw)
        assert passed > len(kept) >= 3                      # something is suppressed and something stays


def test_the_restatement_s_edge_rules():
    def row(cx, cy, w, h, obj, *cls):
        return [cx, cy, w, h, obj, *cls]
    # >= at the confidence threshold; IoU exactly at the threshold keeps both; 0 / 0 keeps both
    p = np.array([row(2, 2, 4, 4, 0.5, 0.5, 0), row(2, 1, 4, 2, 0.9, 0.9, 0)], np.float32)
    rows, passed, kept = ref.postprocess(p, 0.25, 0.5)
    assert passed == 2 and list(kept) == [1, 0]
    z = np.array([row(5, 5, 0, 0, 0.9, 0.9, 0), row(5, 5, 0, 0, 0.8, 0.9, 0)], np.float32)
    assert list(ref.postprocess(z, 0.25, 0.5)[2]) == [0, 1]
    # equal scores: the lower anchor first, and it suppresses the other; equal class maxima: the lower class id
    e = np.array([row(9, 9, 4, 4, 0.8, 0.5, 0.5), row(9, 9, 4, 4, 0.8, 0.5, 0.5)], np.float32)
    rows, passed, kept = ref.postprocess(e, 0.25, 0.5)
    assert list(kept) == [0] and rows[0, 6] == 0
    # NaN never passes
    n = np.array([row(9, 9, 4, 4, np.nan, 0.9, 0.1), row(9, 9, 4, 4, 0.9, np.nan, 0.95), row(9, 9, 4, 4, 0.9, 0.9, 0.1)], np.float32)
    assert list(ref.postprocess(n, 0.25, 0.5)[2]) == [2]


# ---- the library's pure-host parts --------------------------------------------------------------------------------------------------
def create_error() -> bytes:
    return _capi.lib().rtd_yolox_post_last_error(None) or b""


def test_anchor_counts():
    L = _capi.lib()
    out = C.c_int32(-1)
    for (h, w), want in (((640, 640), 8400), ((416, 416), 3549), ((64, 96), 126), ((160, 160), 525)):
        assert L.rtd_yolox_anchors(h, w, C.byref(out)) == _capi.RTD_OK and out.value == want == ref.anchors(h, w) == yd.anchors(h, w)
    out.value = -1
    assert L.rtd_yolox_anchors(100, 96, C.byref(out)) == _capi.RTD_E_INVALID and out.value == -1
    assert b"multiple of 32" in create_error()
    with pytest.raises(_capi.RtdError, match="multiple of 32"):
        yd.anchors(100, 96)


def raw_create(device=0, **kw):
    cfg = _capi.RtdYoloxPostConfig()
    cfg.struct_size = C.sizeof(_capi.RtdYoloxPostConfig)
    cfg.device, cfg.num_classes, cfg.max_batch, cfg.max_anchors, cfg.max_candidates = device, 80, 8, 8400, 2048
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p(0xDEAD)                                  # a refused create must overwrite this with NULL
    rc = _capi.lib().rtd_yolox_post_create(C.byref(cfg), C.byref(h))
    return rc, h.value


@pytest.mark.parametrize("kw, msg", [({"num_classes": 0}, b"num_classes must be 1..1024"), ({"max_candidates": 100}, b"multiple of 64"),
                                      ({"max_batch": 0}, b"max_batch must be 1..64"), ({"struct_size": 4}, b"bad struct_size"),
                                      ({"max_anchors": (1 << 20) + 1}, b"max_anchors must be 1..2^20")])
def test_a_bad_config_is_refused_before_any_hip_call(kw, msg):
    rc, h = raw_create(**kw)
    assert rc == _capi.RTD_E_INVALID and h is None
    assert msg in create_error(), create_error()


def test_a_device_that_does_not_exist_is_refused():
    import torch
    rc, h = raw_create(device=10 ** 6)
    assert rc == (_capi.RTD_E_INVALID if torch.cuda.is_available() else _capi.RTD_E_HIP), (rc, create_error())
    assert h is None and len(create_error()) > 0


def test_the_binding_s_structs_and_keep_words():
    assert C.sizeof(_capi.RtdYoloxPostConfig) == 24 and C.sizeof(_capi.RtdYoloxPostParams) == 32
    assert yd.keep_words(80, None) is None
    w = yd.keep_words(80, [0, 14, 15, 16, 21, 79, 80, -1])
    assert list(w) == [(1 << 0) | (1 << 14) | (1 << 15) | (1 << 16) | (1 << 21), 0, 1 << 15]


# ---- YOLOXDetector on the numpy back end --------------------------------------------------------------------------------------------
INPUT = (64, 96)                                            # 126 anchors


def reference_format(rows, orig_h, orig_w, input_size, wildlife_only):
    """src/yolox_detector.py:_format_model_output_to_detections, restated"""
    out = []
    ratio_h, ratio_w = orig_h / input_size[0], orig_w / input_size[1]
    for x1, y1, x2, y2, obj, cconf, cid in rows:
        x1, y1, x2, y2 = float(x1 * ratio_w), float(y1 * ratio_h), float(x2 * ratio_w), float(y2 * ratio_h)
        cid = int(cid)
        if wildlife_only and cid not in WILDLIFE_CLASSES:
            continue
        out.append({"class_id": cid, "class_name": COCO_CLASSES[cid] if cid < len(COCO_CLASSES) else f"class_{cid}", "confidence": float(obj * cconf),
                    "bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2, "area": int((x2 - x1) * (y2 - y1))}})
    return out


def wildlife_pred():
    return ref.wildlife_variant(ref.seeded("a126_c80"), sorted(WILDLIFE_CLASSES))


def make_detector(pred, **kw):
    backend = kw.pop("backend", None) or ref.RefBackend(num_classes=80, max_batch=8, max_anchors=126, max_candidates=kw.pop("max_candidates", 2048))
    det = yd.YOLOXDetector(device="cpu", input_size=INPUT, model=ref.StandInModel(pred), backend=backend, **kw)
    assert det.load_model() is True
    return det


def frames_of_two_sizes():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, (48, 80, 3), dtype=np.uint8), rng.integers(0, 256, (120, 100, 3), dtype=np.uint8)]


@pytest.mark.parametrize("wildlife_only", [True, False])
def test_detector_dicts_equal_the_reference_s_formatting(wildlife_only):
    pred = wildlife_pred()
    det = make_detector(pred, wildlife_only=wildlife_only)
    frames = frames_of_two_sizes()
    got = det.detect_batch(frames)
    assert det.model.shapes == [(2, 3) + INPUT]
    total = 0
    for i, f in enumerate(frames):
        rows, _, _ = ref.postprocess(pred[i], CONF, NMS)                      # the filter after the NMS, as the reference has it
        want = reference_format(rows, f.shape[0], f.shape[1], INPUT, wildlife_only)
        assert got[i] == want and len(want) > 0
        assert det.detect(f) == reference_format(ref.postprocess(pred[0], CONF, NMS)[0], f.shape[0], f.shape[1], INPUT, wildlife_only)
        total += len(want)
    keep = det._backend.calls[0][4]
    assert keep == (tuple(sorted(WILDLIFE_CLASSES)) if wildlife_only else None)
    if wildlife_only:
        assert all(d["class_id"] in WILDLIFE_CLASSES for dets in got for d in dets)
        assert total < sum(len(d) for d in make_detector(pred, wildlife_only=False).detect_batch(frames))


def test_a_threshold_written_to_the_attribute_is_used_by_the_next_call():
    det = make_detector(ref.seeded("a126_c80"), wildlife_only=False)
    f = frames_of_two_sizes()[0]
    first = det.detect(f)
    det.conf_threshold, det.nms_threshold = 0.97 * 0.97, 0.9
    second = det.detect(f)
    assert det._backend.calls[0][:2] == (0.25, 0.45) and det._backend.calls[1][:2] == (0.97 * 0.97, 0.9)
    assert len(second) < len(first) and all(d["confidence"] >= 0.97 * 0.97 for d in second)


def test_the_truncation_warning_fires_once(caplog):
    det = make_detector(ref.seeded("a126_cut"), wildlife_only=False, max_candidates=ref.CUT)
    f = frames_of_two_sizes()[0]
    with caplog.at_level(logging.WARNING, logger=yd.logger.name):
        a = det.detect(f)
        b = det.detect(f)
    assert a == b and len(a) > 0
    assert len([r for r in caplog.records if "max_candidates" in r.getMessage()]) == 1


def test_the_reference_s_corner_cases():
    import torch
    pred = ref.seeded("a126_c80")
    det = yd.YOLOXDetector(device="cpu", input_size=INPUT, model=ref.StandInModel(pred), backend=ref.RefBackend(max_anchors=126), wildlife_only=False)
    f = frames_of_two_sizes()
    assert det.model is None and det.detect(f[0]) == [] and det.detect_batch(f) == [[], []]
    assert det.load_model() and det.detect_batch([]) == []
    hwc = det.detect_batch([torch.from_numpy(f[0])])
    assert hwc == det.detect_batch([f[0]]) and len(hwc[0]) > 0
    with pytest.raises(ValueError, match="Unexpected tensor dimensions"):
        det.detect_batch([torch.zeros(4)])
    # the reference's attributes and helpers
    assert (det.model_name, det.model_path, det.use_tensorrt, det.is_tensorrt, det.exp) == ("yolox-s", "models/yolox/yolox_s.pth", False, False, None)
    assert det.is_wildlife_relevant(14) and not det.is_wildlife_relevant(1)
    assert [det.get_class_category(c) for c in (0, 14, 15, 16, 21, 2)] == ["person", "bird", "mammal", "mammal", "mammal", "other"]
    # without a back end the CPU is refused, as RTDETRDetector refuses it; without a network (no yolox package here) loading fails
    assert yd.YOLOXDetector(device="cpu", model=ref.StandInModel(pred)).load_model() is False
    try:
        import yolox  # noqa: F401
    except ImportError:
        assert yd.YOLOXDetector(device="cuda:0", backend=ref.RefBackend()).load_model() is False


def test_install_sets_the_class_on_the_reference_s_module(monkeypatch):
    monkeypatch.delitem(sys.modules, "src.yolox_detector", raising=False)
    with pytest.raises(RuntimeError, match="src.yolox_detector"):
        yd.install()
    stand_in = types.ModuleType("src.yolox_detector")
    stand_in.YOLOXDetector = object
    monkeypatch.setitem(sys.modules, "src.yolox_detector", stand_in)
    yd.install()
    assert stand_in.YOLOXDetector is yd.YOLOXDetector
