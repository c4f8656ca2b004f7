"""GPU: the r50vd_m and sp1 / sp2 / sp3 variants, and the fused decoder kernel at 2 and 3 sampling points per level.

Engine cases (tests/variants_ref.py ENGINE_CASES): R18 with 2 and 3 points and either sampler on two 320 x 320 frames - 300 queries in 19 row
tiles, the last with 12 rows - which the plan must run FUSED (one dec_layer_kernel launch per layer; before the point count became a
template parameter of the row kernel they ran per-op, so the path assertions fail there), and r18_sp1, which stays PER_OP.  r50_m runs on
its HF fixture's frames.  The reference is the oracle in fp64; tests/test_variants_host.py asserts that each case's data is well posed.
Every tolerance is one the suite already has: check_fp32_engine, x3_check and the stage bounds of tests/test_gpu_parity.py, the fused
versus per-op bounds of tests/test_gpu_head_configs.py, and for the discrete sampler the row allowance of tests/test_gpu_dsp.py
(yardstick + one row: a single tap that flips at a rounding boundary moves one query)."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

from oracle import rtdetr_oracle as orc
from telescope_cam_detection_amd.arch import ARCHS
from tests import variants_ref as vr
from tests.engine_checks import (check_f16x3_stages, check_fused_decoder_equals_per_op, check_graph_replay_and_batch_invariance,
                                 check_side_stream_equals_serial, make_engine, oracle64_refs, plan_paths)
from tests.util import match_detections

pytestmark = pytest.mark.gpu

M1 = "m1_r50m_160x224"
ALL_CASES = list(vr.ENGINE_CASES) + [M1]
UPSTREAM = "RT-DETR/rtdetrv2_pytorch/configs/rtdetrv2/"


def data(name):
    return vr.fixture_data(name) if name in vr.POINTS_CASES else vr.engine_data(name)


def assert_decoder_path(eng, d):
    got = plan_paths(eng, len(d["frames"]))[0]
    print(f"{d['name']}: decoder {got}")
    assert got == d["decoder"], (d["name"], got)


def dsp_case_of(d):
    """the case layout tests.test_gpu_dsp.check_rows reads, both of its references being the fp64 oracle; allowance = yardstick (the fp32
    oracle loses no row on these cases: test_engine_case_is_well_posed) + one row"""
    l64, b64, s64 = d["out64"]
    return dict(name=d["name"], arch=d["arch"], w=d["w"], input_size=d["input_size"], frames=d["frames"], oracle=[l64, b64, s64],
                g={"labels": l64, "boxes": b64, "scores": s64}, topk=d["col"]["topk"].numpy(), enc=d["col"]["enc_cls_max"].numpy(),
                allowance=[0 + 1] * len(d["frames"]))


# ------------------------------------------------------------------------------------------ 1. against the fp64 oracle
@pytest.mark.parametrize("name", ALL_CASES)
def test_fp32_engine_matches_the_fp64_oracle(name):
    from telescope_cam_detection_amd import _capi
    from tests.test_gpu_parity import check_fp32_engine
    d = data(name)
    eng = make_engine(d, "fp32")
    try:
        check_fp32_engine(eng, d, refs=[r + (d["col"]["enc_cls_max"].numpy(),) for r in oracle64_refs(d)])
        assert_decoder_path(eng, d)
    finally:
        eng.close()
        _capi.debug_option("reset", 0)


@pytest.mark.parametrize("name", ALL_CASES)
def test_f16x3_engine_matches_the_fp64_oracle(name):
    """the stage bounds of test_gpu_parity.test_f16x3_engine_matches_oracle_and_golden, then x3_check against the fp64 oracle - for the
    discrete sampler test_gpu_dsp.check_rows with its allowance instead"""
    from telescope_cam_detection_amd import _capi
    from tests.test_gpu_dsp import check_rows
    from tests.test_gpu_parity import x3_check
    d = data(name)
    col, frames, arch = d["col"], d["frames"], d["arch"]
    eng = make_engine(d, "f16x3")
    try:
        check_f16x3_stages(eng, d)
        if arch.dec_method == "discrete":
            check_rows(dsp_case_of(d), eng, f"{name} f16x3")
        else:
            x3_check(name, arch, d["w"], d["input_size"], eng, frames, col["topk"].numpy(), col["enc_cls_max"].numpy(), oracle64_refs(d), 5e-4)
        assert_decoder_path(eng, d)
    finally:
        eng.close()
        _capi.debug_option("reset", 0)


# ------------------------------------------------------------------------------------------ 2. fused against per-op
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", vr.FUSED_ENGINE_CASES)
def test_fused_decoder_equals_per_op_decoder(name, precision):
    """dec_fused 1 against 0 at 2 and 3 points, both samplers: tests.test_gpu_head_configs.test_fused_decoder_equals_per_op_decoder on
    these cases, same bounds, same two passes (free-running by token, then under the reference's selection row by row)"""
    check_fused_decoder_equals_per_op(data(name), precision)


# ------------------------------------------------------------------------------------------ 3. bit-exact equalities
@pytest.mark.parametrize("name", ALL_CASES)
def test_f16x3_graph_replay_and_batch_invariance(name):
    check_graph_replay_and_batch_invariance(data(name))


@pytest.mark.parametrize("name", ALL_CASES)
def test_f16x3_side_stream_plan_equals_the_serial_plan(name):
    check_side_stream_equals_serial(data(name))


# ------------------------------------------------------------------------------------------ 4. against the HF rows
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", vr.POINTS_CASES)
def test_engine_matches_the_hf_fixture_rows(name, precision):
    """1e-3 / 1e-2 px against HF's rows; the allowance is the yardstick's, which is zero on every frame by the choice of seeds"""
    d = data(name)
    g, frames = d["g"], d["frames"]
    allowance = vr.yardstick()[name]["fp32_vs_fp64_rows_outside_1e-3_1e-2px"]
    eng = make_engine(d, precision)
    try:
        labels, boxes, scores = eng.infer_raw(frames)
        assert_decoder_path(eng, d)
    finally:
        eng.close()
    for b in range(len(frames)):
        m, n, ws, wb = match_detections(g["labels"][b], g["boxes"][b], g["scores"][b], labels[b], boxes[b], scores[b], 1e-3, 1e-2)
        print(f"{name}[{b}] {precision} vs HF: matched {m}/{n} worst dscore={ws:.2e} dbox={wb:.2e}px (allowed to miss {allowance[b]})")
        assert n == d["arch"].num_queries and m >= n - allowance[b], (b, m, n, ws, wb)


# ------------------------------------------------------------------------------------------ 5. detector class
def rows_of(dets):
    return (np.array([x["class_id"] for x in dets]), np.array([[x["bbox"][k] for k in ("x1", "y1", "x2", "y2")] for x in dets]).reshape(-1, 4),
            np.array([x["confidence"] for x in dets]))


def test_detector_serves_sp2_from_its_upstream_config_name(caplog):
    from telescope_cam_detection_amd.rtdetr_detector import RTDETRDetector
    d = data("p2_r18sp2_160x224")                                   # synthetic:r18_sp2:0 are this fixture's weights
    # the oracle's rows on either side of the threshold: a score within the tolerance of it may be kept or dropped
    conf, tol = 0.3, 1e-3
    want_hi = orc.detect_batch(d["arch"], d["w"], d["frames"], d["input_size"], conf + tol, False)
    want_lo = orc.detect_batch(d["arch"], d["w"], d["frames"], d["input_size"], conf - tol, False)
    det = RTDETRDetector(config_path=UPSTREAM + "rtdetrv2_r18vd_sp2_120e_coco.yml", model_path="synthetic:r18_sp2:0", device="cuda:0",
                         conf_threshold=conf, input_size=(160, 224), wildlife_only=False, max_batch=1)
    with caplog.at_level(logging.INFO, logger="telescope_cam_detection_amd.rtdetr_detector"):
        assert det.load_model(verify=True) is True
    try:
        assert det.arch is ARCHS["r18_sp2"] and det.last_check is not None
        assert "bilinear cross-attention sampler at 2 point(s) per level" in caplog.text
        for b, f in enumerate(d["frames"]):
            got = det.detect(f)
            m, n, ws, wb = match_detections(*rows_of(want_hi[b]), *rows_of(got), tol, 1e-2)
            m2, n2, _, _ = match_detections(*rows_of(got), *rows_of(want_lo[b]), tol, 1e-2)
            print(f"sp2 detector [{b}]: {len(got)} rows; oracle rows above {conf + tol}: matched {m}/{n} worst dscore={ws:.2e} dbox={wb:.2e}px; "
                  f"rows with a partner among the oracle's above {conf - tol}: {m2}/{n2}")
            assert n > 50 and m == n and m2 == n2 == len(got) and len(want_hi[b]) <= len(got) <= len(want_lo[b]), (m, n, m2, n2)
            assert [x["class_name"] for x in got] and set(got[0]) == {"class_id", "class_name", "confidence", "bbox"}
    finally:
        det.model.engine.close()


def test_detector_serves_a_six_layer_r50_m_file_as_its_three_layer_decoder(tmp_path):
    """upstream's r50vd_m file stores 6 decoder layers and evaluates at index 2: served under its own config name it equals the
    synthetic r50_m engine of the same weights bit for bit, and under the plain r50 name it is still r50_m - the file decides"""
    from telescope_cam_detection_amd.rtdetr_detector import RTDETRDetector
    from tests.test_variants_host import six_layer_upstream_state
    seed = 4
    state, _ = six_layer_upstream_state(seed)
    ckpt = str(tmp_path / "rtdetrv2_r50vd_m_7x_coco_ema.pth")
    torch.save({"ema": {"module": state}}, ckpt)
    frames = data(M1)["frames"]
    got = {}
    for tag, cfg, mp in (("synthetic", "unused", f"synthetic:r50_m:{seed}"), ("m config", UPSTREAM + "rtdetrv2_r50vd_m_7x_coco.yml", ckpt),
                         ("plain r50 config", UPSTREAM + "rtdetrv2_r50vd_6x_coco.yml", ckpt)):
        det = RTDETRDetector(config_path=cfg, model_path=mp, device="cuda:0", conf_threshold=0.2, input_size=(160, 224), wildlife_only=False,
                             max_batch=2)
        assert det.load_model(verify=False) is True, tag
        try:
            assert det.arch is ARCHS["r50_m"], tag
            assert plan_paths(det.model.engine, 2)[0] == vr.FUSED
            got[tag] = det.detect_batch(frames)
        finally:
            det.model.engine.close()
    assert sum(len(x) for x in got["synthetic"]) > 0
    assert got["m config"] == got["synthetic"] and got["plain r50 config"] == got["synthetic"]


def test_bf16_is_refused_for_r50_m_dsp():
    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.rtdetr_detector import RTDETRDetector
    L = _capi.lib()
    cfg = _capi.cfg_for(ARCHS["r50_m_dsp"], precision=_capi.PREC_BF16, input_size=(160, 224))
    h = C.c_void_p()
    assert L.rtd_create(C.byref(cfg), C.byref(h)) == _capi.RTD_E_INVALID
    msg = L.rtd_last_error(None).decode()
    assert "bf16" in msg and "discrete" in msg
    det = RTDETRDetector(config_path=UPSTREAM + "rtdetrv2_r50vd_m_dsp_3x_coco.yml", model_path="synthetic:r50_m_dsp:0", device="cuda:0",
                         input_size=(160, 224), precision="bf16", max_batch=1)
    assert det.load_model(max_retries=1) is False and det.model is None
    det = RTDETRDetector(config_path=UPSTREAM + "rtdetrv2_r50vd_m_dsp_3x_coco.yml", model_path="synthetic:r50_m_dsp:0", device="cuda:0",
                         input_size=(160, 224), max_batch=1)
    assert det.load_model(verify=False) is True and det.arch is ARCHS["r50_m_dsp"]
    det.model.engine.close()
