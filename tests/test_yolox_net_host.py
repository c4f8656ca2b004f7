"""The YOLOX network's host side, without a GPU: the restatement (tests/yolox_net_ref.py) against hand-worked literals and against
yolox_ref's decode input, fold_state against the unfolded arithmetic, the variants served and refused, the blob's table, configs refused
before any HIP call, the detector's `network` keyword, and the input conditions of the end-to-end case."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import yolox_net_ref as ref
from tests import yolox_ref
from telescope_cam_detection_amd import _capi, yolox_detector, yolox_network
from telescope_cam_detection_amd.weights import unpack_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARD = json.load(open(os.path.join(ROOT, "tests", "golden", "yolox_net_yardstick.json")))["cases"]


def test_rows_have_yolox_ref_s_shape_and_anchor_order():
    """A = rtd_yolox_anchors; a head whose pred convs are zero but for the biases, with one level's reg bias distinct, shows the level
    order; a delta at one pixel of a level's feature map shows the row-major order within it"""
    sd = dict(ref.case_state("s_64x96_n2"))
    x = ref.case_input("s_64x96_n2")[:1]
    out = ref.forward(sd, x)
    A = yolox_detector.anchors(64, 96)
    assert A == yolox_ref.anchors(64, 96) == yolox_network.anchors(64, 96) == 126 and tuple(out.shape) == (1, A, 85)
    for l in range(3):
        for kind in ("cls", "reg", "obj"):
            sd[f"head.{kind}_preds.{l}.weight"] = torch.zeros_like(sd[f"head.{kind}_preds.{l}.weight"])
        sd[f"head.reg_preds.{l}.bias"] = torch.full((4,), float(l + 1))
    out = ref.forward(sd, x)[0]
    first = np.cumsum([0] + [(64 // s) * (96 // s) for s in yolox_ref.STRIDES])
    for l in range(3):
        assert (out[first[l]:first[l + 1], :4] == l + 1).all()
    gx, gy, gs = yolox_ref.grids(64, 96)
    assert list(gs[first[1]:first[2]]) == [16] * 24 and (gx[first[1] + 7], gy[first[1] + 7]) == (1, 1)      # row-major: anchor 7 of the 4 x 6 level is (y 1, x 1)
    dec = yolox_ref.decode(out.numpy(), (64, 96), np.float64)
    assert dec[first[1] + 7, 0] == (2.0 + 1) * 16 and dec[first[1] + 7, 1] == (2.0 + 1) * 16


def test_base_conv_and_focus_order_against_hand_worked_literals():
    x = torch.arange(16, dtype=torch.float64).reshape(1, 1, 4, 4).repeat(1, 3, 1, 1) + torch.tensor([0.0, 100.0, 200.0]).reshape(1, 3, 1, 1)
    f = ref.focus_split(x)
    assert tuple(f.shape) == (1, 12, 2, 2)
    # quadrants: top-left (0, 2, 8, 10), bottom-left (4, 6, 12, 14), top-right (1, 3, 9, 11), bottom-right (5, 7, 13, 15); 3 channels each
    for k, vals in enumerate(((0, 2, 8, 10), (4, 6, 12, 14), (1, 3, 9, 11), (5, 7, 13, 15))):
        for c in range(3):
            assert f[0, 3 * k + c].flatten().tolist() == [v + 100.0 * c for v in vals]
    # a BaseConv(1, 1, 3, 1) of ones on a 2 x 2 map of ones: every output sums the 4 pixels inside its window = 4; BN: (4 - 1) / sqrt(3.999 + 1e-3) * 2 + 0.5
    sd = {"c.conv.weight": torch.ones(1, 1, 3, 3), "c.bn.weight": torch.tensor([2.0]), "c.bn.bias": torch.tensor([0.5]),
          "c.bn.running_mean": torch.tensor([1.0]), "c.bn.running_var": torch.tensor([3.999])}
    v = (4.0 - 1.0) / 2.0 * 2.0 + 0.5
    want = v / (1 + np.exp(-v))
    got = ref.base_conv_of(sd, "c", torch.ones(1, 1, 2, 2, dtype=torch.float64))
    assert np.allclose(got.numpy(), want, rtol=0, atol=1e-6) and abs(want - 3.39741) < 1e-5      # (3.999 is not exact in fp32)


@pytest.mark.parametrize("h,w", [(2, 3), (5, 5), (7, 13)])
def test_pool9_and_pool13_are_repeated_pool5(h, w):
    x = torch.from_numpy(np.random.default_rng(h * w).normal(0, 1, (2, 8, h, w)))
    p5 = ref.pool5(x)
    p9 = ref.pool5(p5)
    assert torch.equal(p5, F.max_pool2d(x, 5, 1, 2)) and torch.equal(p9, F.max_pool2d(x, 9, 1, 4)) and torch.equal(ref.pool5(p9), F.max_pool2d(x, 13, 1, 6))


def test_fold_state_against_the_unfolded_restatement():
    """every folded conv, applied to a random input in fp64, equals conv -> BatchNorm of the unfolded state to 1e-12 relative; the blob
    round trip keeps the fp32 roundings of exactly those tensors"""
    sd = ref.case_state("s_64x96_n2")
    v = yolox_network.variant_of("yolox_s", sd)
    assert v == yolox_network.Variant("yolox-s", 32, 1, 80)
    folded = yolox_network.fold_tensors(sd, v)
    rng = torch.Generator().manual_seed(0)
    table = yolox_network.conv_table(v.base, v.depth)
    assert len(table) == len(ref.base_conv_names(v.base, v.depth)) and len(folded) == 2 * (len(table) + 6)
    for name, cin, cout, k, stride in table:
        x = torch.randn((1, cin, 5, 6), generator=rng, dtype=torch.float64)
        w, b = folded[name + ".weight"], folded[name + ".bias"]
        assert tuple(w.shape) == (cout, k, k, 32 if cin == 12 else cin)
        if cin == 12:
            assert (w[..., 12:] == 0).all()
        got = F.conv2d(x, w[..., :cin].permute(0, 3, 1, 2), b, stride=stride, padding=(k - 1) // 2)
        t = F.conv2d(x, sd[name + ".conv.weight"].double(), None, stride=stride, padding=(k - 1) // 2)
        g, bb, m, var = (sd[f"{name}.bn.{s}"].double()[None, :, None, None] for s in ("weight", "bias", "running_mean", "running_var"))
        want = (t - m) / torch.sqrt(var + 1e-3) * g + bb
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
    for l in range(3):
        w = folded[f"head.regobj_preds.{l}.weight"]
        assert tuple(w.shape) == (5, 1, 1, 128)
        assert torch.equal(w[:4, 0, 0], sd[f"head.reg_preds.{l}.weight"][:, :, 0, 0].double()) and torch.equal(w[4, 0, 0], sd[f"head.obj_preds.{l}.weight"][0, :, 0, 0].double())
        assert torch.equal(folded[f"head.regobj_preds.{l}.bias"][4:], sd[f"head.obj_preds.{l}.bias"].double())
        assert tuple(folded[f"head.cls_preds.{l}.weight"].shape) == (80, 1, 1, 128)
    back = unpack_blob(yolox_network.fold_state(sd, v))
    assert set(back) == set(folded)
    for k_, t in folded.items():
        assert np.array_equal(back[k_], t.to(torch.float32).numpy()), k_


def test_variants_served_and_refused():
    s, l = ref.case_state("s_64x96_n2"), ref.case_state("l_64x96_n1")
    assert yolox_network.variant_of("yolox-s", s) == yolox_network.variant_of("yolox_s", s)
    assert yolox_network.variant_of("yolox-l", l) == yolox_network.Variant("yolox-l", 64, 3, 80)
    for name, why in (("yolox-m", "48 channels"), ("yolox-x", "80 channels"), ("yolox-tiny", "24 channels"), ("yolox-nano", "depthwise"), ("yolov8", "unknown")):
        with pytest.raises(_capi.RtdError, match=why):
            yolox_network.variant_of(name, s)
    with pytest.raises(_capi.RtdError, match="base width of 64 channels, the checkpoint's stem has 32"):
        yolox_network.variant_of("yolox-l", s)
    with pytest.raises(_capi.RtdError, match="1 bottlenecks in dark2"):
        yolox_network.variant_of("yolox-s", {k: v for k, v in l.items() if "dark" in k or "cls_preds" in k} | {"backbone.backbone.stem.conv.conv.weight": s["backbone.backbone.stem.conv.conv.weight"]})
    with pytest.raises(_capi.RtdError, match="not a YOLOX checkpoint"):
        yolox_network.variant_of("yolox-s", {})
    assert yolox_network.state_dict_of({"model": s}) is s and yolox_network.state_dict_of(s) is s
    c3 = ref.synth_state("yolox-s", 3, 4)
    assert yolox_network.variant_of("yolox-s", c3).num_classes == 3
    missing = {k: v for k, v in s.items() if k != "backbone.C3_n3.conv3.bn.running_var"}
    with pytest.raises(_capi.RtdError, match="missing tensor backbone.C3_n3.conv3.bn.running_var"):
        yolox_network.fold_state(missing, yolox_network.variant_of("yolox-s", s))


def test_configs_are_refused_before_any_hip_call():
    L = _capi.lib()
    sd = ref.case_state("s_64x96_n2")
    blob = yolox_network.fold_state(sd, yolox_network.variant_of("yolox-s", sd))
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)

    def create(**changes):
        cfg = _capi.RtdYoloxNetConfig()
        cfg.struct_size, cfg.precision, cfg.num_classes, cfg.base_channels, cfg.depth, cfg.max_batch = C.sizeof(cfg), _capi.PREC_F16X3, 80, 32, 1, 8
        for k, v in changes.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        rc = L.rtd_yolox_net_create(C.byref(cfg), buf, len(blob), C.byref(h))
        assert not h.value
        return rc, L.rtd_yolox_net_last_error(None).decode()

    for changes, why in (({"struct_size": 8}, "struct_size"), ({"precision": _capi.PREC_BF16}, "bf16"), ({"base_channels": 48}, "base_channels 48"),
                         ({"base_channels": 24}, "base_channels 24"), ({"depth": 0}, "depth"), ({"num_classes": 0}, "num_classes"), ({"max_batch": 65}, "max_batch"),
                         ({"num_classes": 3}, "not this variant"), ({"depth": 3}, "not this variant"), ({"base_channels": 64}, "not this variant")):
        rc, msg = create(**changes)
        assert rc == _capi.RTD_E_INVALID and why in msg, (changes, rc, msg)
    assert L.rtd_yolox_net_create(None, buf, len(blob), C.byref(C.c_void_p())) == _capi.RTD_E_INVALID
    cfg = _capi.RtdYoloxNetConfig()
    cfg.struct_size, cfg.precision, cfg.num_classes, cfg.base_channels, cfg.depth, cfg.max_batch = C.sizeof(cfg), _capi.PREC_F16X3, 80, 32, 1, 8
    assert L.rtd_yolox_net_create(C.byref(cfg), buf, len(blob), None) == _capi.RTD_E_INVALID
    h = C.c_void_p()
    assert L.rtd_yolox_net_create(C.byref(cfg), None, 0, C.byref(h)) == _capi.RTD_E_INVALID and not h.value
    assert L.rtd_yolox_net_create(C.byref(cfg), buf, 64, C.byref(h)) == _capi.RTD_E_WEIGHTS and b"weight blob: " in L.rtd_yolox_net_last_error(None)      # (a cut blob)
    assert L.rtd_yolox_net_run(None, 1, None, 64, 96, None, None) == _capi.RTD_E_INVALID and L.rtd_yolox_net_arena_bytes(None) == 0
    L.rtd_yolox_net_destroy(None)
    # the kernel-level entry points check their arguments before they touch a device
    p = C.c_void_p(4096)
    three = (C.c_void_p * 3)(4096, 4096, 4096)
    assert L.rtd_op_yolox_focus(_capi.DT_F32, p, p, 1, 63, 96) == _capi.RTD_E_INVALID
    assert L.rtd_op_yolox_focus(_capi.DT_BF16, p, p, 1, 64, 96) == _capi.RTD_E_INVALID
    assert L.rtd_op_yolox_spp(_capi.DT_F16X2, p, 1, 5, 5, 8) == _capi.RTD_E_INVALID and b"32-channel groups" in L.rtd_yolox_net_last_error(None)
    assert L.rtd_op_yolox_spp(_capi.DT_F32, p, 1, 0, 5, 32) == _capi.RTD_E_INVALID
    assert L.rtd_op_yolox_head_emit(three, three, 96, 32, 1, 64, 100, 80, p) == _capi.RTD_E_INVALID
    assert L.rtd_op_yolox_head_emit(three, three, 64, 32, 1, 64, 96, 80, p) == _capi.RTD_E_INVALID


def test_detector_network_keyword(tmp_path, caplog):
    with pytest.raises(ValueError, match="network"):
        yolox_detector.YOLOXDetector(network="torch")
    for path in (str(tmp_path / "missing.pth"), str(tmp_path)):
        det = yolox_detector.YOLOXDetector(network="mi355", model_path=path, device="cuda:0")
        with caplog.at_level(logging.ERROR, logger=yolox_detector.logger.name):
            caplog.clear()
            assert det.load_model() is False
        assert len(caplog.records) == 1 and "does not exist or cannot be read" in caplog.records[0].getMessage()
        assert det.model is None and det.decode is False
    # a file that is no checkpoint, and a checkpoint of a variant that is not served: refused on the host, one error each
    junk = tmp_path / "junk.pth"
    junk.write_bytes(b"not a checkpoint")
    wrong = tmp_path / "wrong.pth"
    torch.save({"model": ref.case_state("s_64x96_n2")}, wrong)
    for path, name in ((junk, "yolox-s"), (wrong, "yolox-l"), (wrong, "yolox-m")):
        det = yolox_detector.YOLOXDetector(network="mi355", model_name=name, model_path=str(path), device="cuda:0")
        with caplog.at_level(logging.ERROR, logger=yolox_detector.logger.name):
            caplog.clear()
            assert det.load_model() is False
        assert len(caplog.records) == 1 and "is refused" in caplog.records[0].getMessage()
    # an injected model behaves as before, whatever `network` says
    pred = yolox_ref.seeded("a126_c80")
    det = yolox_detector.YOLOXDetector(device="cpu", input_size=(64, 96), model=yolox_ref.StandInModel(pred), backend=yolox_ref.RefBackend(max_anchors=126),
                                       wildlife_only=False, network="mi355")
    assert det.load_model() and det.decode is False and isinstance(det.model, yolox_ref.StandInModel)


def test_restatement_against_upstream_where_yolox_is_importable():
    yolox = pytest.importorskip("yolox")
    from yolox.exp import get_exp
    exp = get_exp(None, "yolox-s")
    model = exp.get_model().eval()
    model.head.decode_in_inference = False
    x = ref.case_input("s_64x96_n2")
    with torch.no_grad():
        want = model(x)
    got = ref.forward(model.state_dict(), x)
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_end_to_end_input_conditions_hold_on_the_restatement_alone():
    """conditions on the INPUT of the end-to-end GPU test, not tolerances: with m = 100 x the recorded torch-fp32 head error of the case,
    20..500 rows pass per image, no score lies within m of the confidence threshold, no same-class pair's IoU within m of the NMS
    threshold, and the fp32 restatement keeps fp64's rows in fp64's order"""
    rec = YARD["e2e"]
    assert tuple(rec["input_size"]) == tuple(ref.E2E["input_size"]) and [tuple(f) for f in rec["frames"]] == [tuple(f) for f in ref.E2E["frames"]]
    assert rec["state_seed"] == ref.E2E["state_seed"] and rec["head"] == ref.E2E["head"]
    m = 100.0 * rec["errors"]["head"]["fp32"]
    cond = ref.e2e_conditions(ref.e2e_batch(ref.e2e_frames()), rec["errors"]["head"]["fp32"])
    assert len(cond) == 2
    for c, r in zip(cond, rec["images"]):
        print(c)
        assert 20 <= c["passed"] <= 500 and c["passed"] == r["passed"] and c["kept"] == r["kept"]
        assert c["d_score"] > m and c["d_iou"] > m and c["same_rows"]


def test_yardstick_belongs_to_the_cases_and_leaves_fp32_four_times_inside_the_gate():
    for name, (model, classes, state_seed, input_seed, n, h, w) in ref.NET_CASES.items():
        rec = YARD[name]
        assert (rec["model"], rec["classes"], rec["state_seed"], rec["input_seed"], rec["n"], rec["h"], rec["w"]) == (model, classes, state_seed, input_seed, n, h, w)
    for name, rec in YARD.items():
        assert set(rec["errors"]) == {"head", *ref.STAGES}
        for k, e in rec["errors"].items():
            assert 0 < e["fp32"] * 16 <= e["fp16"], (name, k, e)
