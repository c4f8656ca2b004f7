"""The crop enhancement on the MI355X (csrc/enhance.hip): every comparison is exact equality with the numpy restatement
(tests/enhance_ref.py), stage by stage through rtd_debug_enhance_stage (Lab, tile LUTs, BGR before the bilateral filter) and on the
final bytes - crops that divide the tile grid and crops that are padded on both axes, several ragged bilateral tiles, a crop that is
its whole frame, a one-pixel CLAHE tile, four contents, the parameter corners, mixed batches, the 64-crop limit and chunking, the
limits, stream ordering, and the enhanced crops through the crop batcher and BatchedStage2."""
import ctypes as C
import types
from collections import deque

import numpy as np
import pytest
import torch

from tests import enhance_ref as ref
from tests.standins import StandInPipeline
from telescope_cam_detection_amd import _capi, enhance
from telescope_cam_detection_amd.stage2 import BatchedStage2, CropBatcher, crop_rect, format_predictions, normalised_bbox

pytestmark = pytest.mark.gpu

CONTENTS = ("noise", "ramp", "zero", "full")
# (frame h, frame w, rect x1 y1 x2 y2)
CROPS = {
    "64x64_interior": (96, 128, (20, 10, 84, 74)),          # divides the 8 x 8 grid
    "67x73": (90, 100, (13, 9, 80, 82)),                    # padded on both axes
    "64x73": (90, 100, (30, 5, 94, 78)),                    # padded on both axes because of one
    "131x70": (80, 140, (4, 6, 135, 76)),                   # several bilateral tiles with ragged edges
    "whole_80x96": (80, 96, (0, 0, 96, 80)),                # touches all four frame edges
}


def make_frame(name, kind, seed):
    """a noise frame whose crop rectangle holds `kind`: a halo read from the frame instead of reflected inside the crop shows"""
    fh, fw, (x1, y1, x2, y2) = CROPS[name]
    frame = np.random.default_rng(1000 + seed).integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    frame[y1:y2, x1:x2] = ref.content(kind, y2 - y1, x2 - x1, seed)
    return frame


_REF = {}


def reference(crop: np.ndarray, params: dict):
    """ref.stages of a crop, computed once per (bytes, parameters)"""
    key = (crop.shape, crop.tobytes(), tuple(sorted((k, str(v)) for k, v in params.items())))
    if key not in _REF:
        _REF[key] = ref.stages(crop, **params)
    return _REF[key]


def ref_params(e: enhance.CropEnhancer) -> dict:
    p = e.params
    return {"clip_limit": p["clip_limit"], "tile_grid_size": p["tile_grid_size"], "bilateral_d": p["bilateral_d"], "sigma_color": p["sigma_color"],
            "sigma_space": p["sigma_space"]}


@pytest.fixture(scope="module")
def default_enhancer():
    e = enhance.CropEnhancer()
    yield e
    e.close()


def check_call(e, frames_np, rects_per_frame, stages=True):
    """one enhance() of at most 64 crops against the restatement, every stage of every crop"""
    frames = [torch.from_numpy(f).cuda() for f in frames_np]
    buf, offsets, shapes = e.enhance(frames, rects_per_frame)
    got = buf.cpu().numpy()
    flat = [(f, r) for f, rects in zip(frames_np, rects_per_frame) for r in rects]
    assert len(flat) <= enhance.MAX_CROPS_PER_CALL and len(offsets) == len(flat) + 1
    tx, ty = e.params["tile_grid_size"]
    for i, (f, (x1, y1, x2, y2)) in enumerate(flat):
        crop = np.ascontiguousarray(f[y1:y2, x1:x2])
        want = reference(crop, ref_params(e))
        h, w = crop.shape[:2]
        assert shapes[i] == (h, w)
        if stages:
            for stage, key, shape in ((0, "lab", (h, w, 3)), (1, "luts", (ty, tx, 256)), (2, "bgr", (h, w, 3))):
                g = e.debug_stage(i, stage, shape)
                assert (g == want[key]).all(), (i, (h, w), key, int((g != want[key]).sum()), np.argwhere(g != want[key])[:3].tolist())
        g = got[offsets[i]:offsets[i] + h * w * 3].reshape(h, w, 3)
        assert (g == want["out"]).all(), (i, (h, w), "out", int((g != want["out"]).sum()), np.argwhere(g != want["out"])[:3].tolist())
    for f_np, f in zip(frames_np, frames):
        assert (f.cpu().numpy() == f_np).all()                  # the frames are only read
    return got, offsets


def test_every_crop_and_content_with_the_defaults(default_enhancer):
    frames, rects = [], []
    for name in CROPS:
        for s, kind in enumerate(CONTENTS):
            frames.append(make_frame(name, kind, s))
            rects.append([CROPS[name][2]])
    check_call(default_enhancer, frames, rects)


PARAMS = {
    "clip0": dict(clip_limit=0.0),
    "clip40": dict(clip_limit=40.0),
    "grid4x2": dict(tile_grid_size=(4, 2)),
    "d3": dict(bilateral_d=3),
    "d15": dict(bilateral_d=15),
    "sigma10": dict(sigma_color=10, sigma_space=10),
    "sigma150": dict(sigma_color=150, sigma_space=150),
}


@pytest.mark.parametrize("name", list(PARAMS))
def test_parameter_corners(name):
    e = enhance.CropEnhancer(**PARAMS[name])
    try:
        frames, rects = [], []
        for crop in ("67x73", "131x70", "whole_80x96"):
            for s, kind in enumerate(("noise", "ramp")):
                frames.append(make_frame(crop, kind, 10 + s))
                rects.append([CROPS[crop][2]])
        check_call(e, frames, rects)
    finally:
        e.close()


def test_one_pixel_tiles():
    e = enhance.CropEnhancer(tile_grid_size=(16, 16))
    try:
        frames = [np.random.default_rng(50 + s).integers(0, 256, (40, 48, 3), dtype=np.uint8) for s in range(len(CONTENTS))]
        for s, kind in enumerate(CONTENTS):
            frames[s][12:28, 20:36] = ref.content(kind, 16, 16, s)
        check_call(e, frames, [[(20, 12, 36, 28)]] * len(frames))
        check_call(e, [make_frame("67x73", "noise", 3)], [[CROPS["67x73"][2]]])     # 16 x 16 tiles of 5 x 5 from a padded crop
    finally:
        e.close()


def test_three_mixed_crops_from_two_frames_in_one_call(default_enhancer):
    a = np.random.default_rng(60).integers(0, 256, (120, 200, 3), dtype=np.uint8)
    b = ref.content("ramp", 90, 70, 0)
    check_call(default_enhancer, [a, b], [[(0, 0, 67, 73), (100, 30, 200, 120)], [(3, 10, 70, 90)]])


def small_crops(n, seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), ref.content("ramp", 48, 64, 1), np.full((20, 16, 3), 255, np.uint8)]
    rects = [[], [], []]
    for i in range(n):
        fi = i % 3
        fh, fw = frames[fi].shape[:2]
        x, y = int(rng.integers(0, fw - 15)), int(rng.integers(0, fh - 15))
        rects[fi].append((x, y, x + 16, y + 16))
    return frames, rects


def test_64_crops_in_one_call(default_enhancer):
    frames, rects = small_crops(64, 70)
    check_call(default_enhancer, frames, rects, stages=False)
    assert default_enhancer.debug_stage(63, 1, (8, 8, 256)).shape == (8, 8, 256)


def test_65_crops_are_chunked(default_enhancer):
    e = default_enhancer
    frames_np, rects = small_crops(65, 71)
    frames = [torch.from_numpy(f).cuda() for f in frames_np]
    buf, offsets, shapes = e.enhance(frames, rects)
    got = buf.cpu().numpy()
    flat = [(f, r) for f, rs in zip(frames_np, rects) for r in rs]
    assert len(shapes) == 65 and len(offsets) == 66
    for i, (f, (x1, y1, x2, y2)) in enumerate(flat):
        want = reference(np.ascontiguousarray(f[y1:y2, x1:x2]), ref_params(e))
        assert (got[offsets[i]:offsets[i] + 768].reshape(16, 16, 3) == want["out"]).all(), i
    f, (x1, y1, x2, y2) = flat[64]                               # the second call held the 65th crop alone
    assert (e.debug_stage(0, 0, (16, 16, 3)) == reference(np.ascontiguousarray(f[y1:y2, x1:x2]), ref_params(e))["lab"]).all()
    with pytest.raises(_capi.RtdError):
        e.debug_stage(1, 0, (16, 16, 3))


def raw_call(e, frames, rects, out, out_cap=None, n=None):
    k = len(rects)
    ptrs = (C.c_void_p * max(k, 1))(*[f.data_ptr() for f in frames])
    hw = (C.c_int32 * max(2 * k, 1))(*[int(v) for f in frames for v in f.shape[:2]])
    rc = (C.c_int32 * max(4 * k, 1))(*[int(v) for r in rects for v in r])
    return _capi.lib().rtd_enhance_crops(e._h, k if n is None else n, ptrs, hw, rc, C.c_void_p(out.data_ptr()), out.numel() if out_cap is None else out_cap,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_limits_are_refused_and_leave_the_output_untouched(default_enhancer):
    e = default_enhancer
    frame = torch.from_numpy(ref.content("noise", 60, 80, 2)).cuda()
    out = torch.full((64 * 64 * 3 * 2,), 0xAB, dtype=torch.uint8, device="cuda")
    good = (8, 8, 40, 40)
    need = enhance.layout([good])[-1]
    cases = {"15 px wide": [(0, 0, 15, 30)], "15 px high": [(0, 0, 30, 15)], "right of its frame": [(60, 0, 81, 30)], "below its frame": [(0, 40, 30, 61)],
             "negative corner": [(-1, 0, 30, 30)], "second crop bad": [good, (0, 0, 15, 30)]}
    for what, rects in cases.items():
        assert raw_call(e, [frame] * len(rects), rects, out) == _capi.RTD_E_INVALID, what
        assert _capi.lib().rtd_enhance_last_error(e._h)
    assert raw_call(e, [frame], [good], out, out_cap=need - 1) == _capi.RTD_E_INVALID              # one byte short
    assert raw_call(e, [frame], [good], out, n=0) == _capi.RTD_E_INVALID
    assert raw_call(e, [frame] * 65, [good] * 65, out) == _capi.RTD_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    assert raw_call(e, [frame], [good], out, out_cap=need) == _capi.RTD_OK                         # ... and exactly enough is enough
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:32 * 32 * 3].reshape(32, 32, 3) == reference(frame.cpu().numpy()[8:40, 8:40].copy(), ref_params(e))["out"]).all()
    assert (o[need:] == 0xAB).all()
    for bad in (dict(tile_grid_size=(17, 17)), dict(tile_grid_size=(8, 0)), dict(bilateral_d=17), dict(bilateral_d=0, sigma_space=75)):
        with pytest.raises(_capi.RtdError) as ei:
            enhance.CropEnhancer(**bad)
        assert ei.value.code == _capi.RTD_E_INVALID, bad


def test_stream_order_needs_no_synchronisation(default_enhancer):
    e = default_enhancer
    batcher = CropBatcher(input_size=64, min_crop_size=16)
    base = torch.from_numpy(np.random.default_rng(80).integers(0, 200, (300, 400, 3), dtype=np.uint8)).cuda()
    rects = [[(10, 20, 141, 90), (200, 100, 267, 173)]]
    final = base + 37
    want = batcher.preprocess_batch([final], rects, enhancer=e)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    frame = torch.zeros_like(base)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(37):                                      # the producer: the frame is complete only when the stream has run all of it
            frame += 1
        frame += base
        got = batcher.preprocess_batch([frame], rects, enhancer=e)          # rtd_enhance_crops and rtd_crop_resize_batch follow on s, no sync between
    s.synchronize()
    assert torch.equal(got, want)


def test_batcher_with_enhancer_equals_the_batcher_on_reference_enhanced_crops(default_enhancer):
    e = default_enhancer
    batcher = CropBatcher(input_size=96, min_crop_size=16)
    frames_np = [make_frame("131x70", "noise", 5), make_frame("67x73", "ramp", 6)]
    rects = [[CROPS["131x70"][2], (0, 0, 64, 64)], [CROPS["67x73"][2]]]
    got = batcher.preprocess_batch([torch.from_numpy(f).cuda() for f in frames_np], rects, enhancer=e)
    enhanced = [reference(np.ascontiguousarray(f[y1:y2, x1:x2]), ref_params(e))["out"] for f, rs in zip(frames_np, rects) for (x1, y1, x2, y2) in rs]
    want = batcher.preprocess_batch([torch.from_numpy(c).cuda() for c in enhanced], [[(0, 0, c.shape[1], c.shape[0])] for c in enhanced])
    assert got.shape == (3, 3, 96, 96) and torch.equal(got, want)                  # the same resize kernel on the same bytes
    plain = batcher.preprocess_batch([torch.from_numpy(f).cuda() for f in frames_np], rects)
    assert not torch.equal(got, plain)


def test_batched_stage2_auto_equals_a_per_detection_loop():
    p = StandInPipeline(min_crop_size=64)
    p.enhancer = types.SimpleNamespace(method="clahe", clahe_clip_limit=2.0, clahe_tile_grid_size=(8, 8), bilateral_d=9, bilateral_sigma_color=75,
                                       bilateral_sigma_space=75)
    p.enhancement_times = deque(maxlen=1000)
    p.process_detections = lambda *a: pytest.fail("the per-detection fallback ran")
    batcher = CropBatcher(input_size=96, min_crop_size=p.min_crop_size, crop_padding_percent=p.crop_padding_percent)     # a small classifier input: quick
    s2 = BatchedStage2(p, batcher=batcher, enhancer="auto")
    assert isinstance(s2.enhancer, enhance.CropEnhancer)
    rng = np.random.default_rng(90)
    frames_np = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8), ref.content("ramp", 200, 260, 4)]
    boxes = [[(14, 20.5, 30.2, 120.9, 140.0), (15, 150, 10, 300, 200), (14, 0, 0, 40, 40), (2, 50, 50, 150, 150)],
             [(21, 30, 40, 130, 160), (14, 100, 60, 255, 199.5)]]
    dets = [[{"class_id": c, "class_name": "x", "confidence": 0.9, "bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}} for c, x1, y1, x2, y2 in per]
            for per in boxes]
    want = [[dict(d, bbox=dict(d["bbox"])) for d in per] for per in dets]
    got = s2.process_batch([torch.from_numpy(f).cuda() for f in frames_np], dets)

    n_crops = 0
    for f, per in zip(frames_np, want):                            # the reference's loop: one detection at a time, enhanced on the CPU
        for d in per:
            d["bbox"] = normalised_bbox(d["bbox"])
            category = p.class_id_to_category.get(d["class_id"])
            if category not in p.species_classifiers:
                d["species"], d["species_confidence"] = None, 0.0
                continue
            rect = crop_rect(d["bbox"], f.shape[:2], p.min_crop_size, p.crop_padding_percent)
            if rect is None:
                s2._set(d, None, 0.0, category, None)
                continue
            x1, y1, x2, y2 = rect
            crop = reference(np.ascontiguousarray(f[y1:y2, x1:x2]), ref_params(s2.enhancer))["out"]
            x = s2.batcher.preprocess_batch([torch.from_numpy(crop).cuda()], [[(0, 0, x2 - x1, y2 - y1)]])
            clf = p.species_classifiers[category]
            with torch.no_grad():
                probs = torch.softmax(clf.model(x), dim=1).float().cpu()
            s2._conclude(d, category, format_predictions(clf, probs[0], 1))
            n_crops += 1
    assert n_crops == 4 and len(p.enhancement_times) == n_crops and all(t > 0 for t in p.enhancement_times)
    for g_per, w_per in zip(got, want):
        assert len(g_per) == len(w_per)
        for g, w in zip(g_per, w_per):
            assert set(g) == set(w) and g["bbox"] == w["bbox"] and g["class_id"] == w["class_id"]
            for k in ("species", "taxonomic_level", "stage2_category"):
                assert g.get(k) == w.get(k), (k, g, w)
            # the same input bytes; a batched and a single-row forward of the fp32 stand-in net may sum in another order
            assert g["species_confidence"] == pytest.approx(w["species_confidence"], rel=1e-4, abs=1e-6)
    s2.enhancer.close()
