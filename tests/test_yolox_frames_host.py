"""The YOLOX uint8 front end's host side, without a GPU: the float32 restatement (tests/yolox_frames_ref.py) against its own fp64 blend
and against F.interpolate on the CPU, the refusals of rtd_yolox_net_run_frames / rtd_op_yolox_focus_u8 before any HIP call, and
YOLOXDetector's `frontend` keyword - its values, the injected-model refusal, and which frames take which path."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import yolox_frames_ref as fr
from tests import yolox_ref
from telescope_cam_detection_amd import _capi, yolox_detector, yolox_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(48, 80), (120, 200), (64, 96), (37, 53), (1, 1), (3, 2000), (2047, 2048)]      # each -> 64 x 96
IN_H, IN_W = 64, 96
# nine roundings of at most 2^-24 relative on values <= 255: 9 * 255 * 2^-24 = 1.37e-4
BOUND_F64 = 1.4e-4
# one ulp of a source coordinate below 2048 (2^-12) times the largest pixel step (255): torch may order or contract the index arithmetic
# differently (sides <= 2048)
BOUND_TORCH = 255 * 2.0 ** -12

_frames = {}


def frame(h, w):
    if (h, w) not in _frames:
        _frames[(h, w)] = fr.seeded_frame(1000 * h + w, h, w)
    return _frames[(h, w)]


def interpolate(f, in_h, in_w):
    """the reference's preprocess on the CPU"""
    return F.interpolate(torch.from_numpy(f).permute(2, 0, 1).unsqueeze(0).float(), size=(in_h, in_w), mode="bilinear", align_corners=False)[0].numpy()


@pytest.mark.parametrize("h,w", CASES)
def test_restatement_against_its_fp64_blend_and_against_interpolate(h, w):
    f = frame(h, w)
    got = fr.resize(f, IN_H, IN_W)
    assert got.dtype == np.float32 and got.shape == (3, IN_H, IN_W)
    e64 = float(np.abs(got.astype(np.float64) - fr.resize64(f, IN_H, IN_W)).max())
    et = float(np.abs(got - interpolate(f, IN_H, IN_W)).max())
    print(f"{h} x {w} -> {IN_H} x {IN_W}: fp32 against its fp64 blend {e64:.3e} (bound {BOUND_F64:.1e}), against F.interpolate {et:.3e} (bound {BOUND_TORCH:.4f})")
    assert e64 <= BOUND_F64 and et <= BOUND_TORCH
    assert got.min() >= 0 and got.max() <= 255


@pytest.mark.parametrize("h,w,in_h,in_w", [(64, 96, 64, 96), (1080, 1920, 640, 640), (1440, 2560, 640, 640)])
def test_exact_coordinates_are_bit_equal_to_interpolate(h, w, in_h, in_w):
    """identity, and the two camera sizes: 1080 / 640 = 1.6875, 1920 / 640 = 3, 1440 / 640 = 2.25 and 2560 / 640 = 4 are dyadic, so the
    scale factors and every source coordinate are exact in fp32"""
    f = frame(h, w)
    got = fr.resize(f, in_h, in_w)
    assert np.array_equal(got.view(np.uint32), interpolate(f, in_h, in_w).view(np.uint32))
    if (h, w) == (in_h, in_w):
        assert np.array_equal(got, f.transpose(2, 0, 1).astype(np.float32))


def test_taps_at_the_edges_and_hand_worked_values():
    # 2 -> 4: scale 0.5; f = max(0.5 (d + 0.5) - 0.5, 0) = 0, 0.25, 0.75, 1.25 -> (0, 1, .), (0, 1, .25), (0, 1, .75), (1, 1, .25)
    i0, i1, l0, l1 = fr.taps(2, 4)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and l1.tolist() == [0.0, 0.25, 0.75, 0.25] and l0.tolist() == [1.0, 0.75, 0.25, 0.75]
    # 1 -> n: every tap is pixel 0 and the blend returns it whatever the fraction is
    i0, i1, _, _ = fr.taps(1, 5)
    assert not i0.any() and not i1.any()
    assert np.array_equal(fr.resize(np.full((1, 1, 3), 255, np.uint8), 4, 6), np.full((3, 4, 6), 255, np.float32))
    # 4 -> 2: scale 2; f = 0.5, 2.5
    i0, i1, l0, l1 = fr.taps(4, 2)
    assert i0.tolist() == [0, 2] and i1.tolist() == [1, 3] and l1.tolist() == [0.5, 0.5]
    f = np.arange(4 * 4 * 3, dtype=np.uint8).reshape(4, 4, 3)
    got = fr.resize(f, 2, 2)
    assert got[0, 0, 0] == (0 + 3 + 12 + 15) / 4 and got[2, 1, 1] == (32 + 35 + 44 + 47) / 4       # BGR order kept: channel c of the frame is plane c


def test_refusals_happen_before_any_hip_call():
    L = _capi.lib()
    p = 4096
    y = C.c_void_p(4096)

    def op(dt, ptrs, hw, n, in_h, in_w, out):
        frames, sizes = yolox_network.frame_arrays(ptrs, hw)
        rc = L.rtd_op_yolox_focus_u8(dt, frames, sizes, n, in_h, in_w, out)
        return rc, L.rtd_yolox_net_last_error(None).decode()

    ok_hw = [(48, 80), (1, 16384)]
    for args, why in (((_capi.DT_F32, None, ok_hw, 2, 64, 96, y), "null"), ((_capi.DT_F32, [p, p], None, 2, 64, 96, y), "null"),
                      ((_capi.DT_F32, [p, 0], ok_hw, 2, 64, 96, y), "frame 1: null"), ((_capi.DT_F32, [p, p], ok_hw, 0, 64, 96, y), "max_batch"),
                      ((_capi.DT_F32, [p] * 65, [(4, 4)] * 65, 65, 64, 96, y), "max_batch"),
                      ((_capi.DT_F32, [p, p], [(48, 80), (0, 5)], 2, 64, 96, y), "frame 1: sides"),
                      ((_capi.DT_F32, [p, p], [(48, 16385), (5, 5)], 2, 64, 96, y), "frame 0: sides"),
                      ((_capi.DT_F32, [p, p], [(48, 80), (5, -1)], 2, 64, 96, y), "frame 1: sides"),
                      ((_capi.DT_F32, [p, p], ok_hw, 2, 63, 96, y), "even"), ((_capi.DT_F32, [p, p], ok_hw, 2, 64, 0, y), "even"),
                      ((_capi.DT_F32, [p, p], ok_hw, 2, 64, 96, None), "even"), ((_capi.DT_F32, [p, p], ok_hw, 2, 64, 96, C.c_void_p(4100)), "alignment"),
                      ((_capi.DT_BF16, [p, p], ok_hw, 2, 64, 96, y), "dtype")):
        rc, msg = op(*args)
        assert rc == _capi.RTD_E_INVALID and why in msg, (args, rc, msg)
    # the product entry: a null handle is refused before its arguments are looked at
    frames, sizes = yolox_network.frame_arrays([p], [(48, 80)])
    assert L.rtd_yolox_net_run_frames(None, 1, frames, sizes, 64, 96, y, None) == _capi.RTD_E_INVALID
    assert L.rtd_yolox_net_run_frames(None, 1, None, None, 64, 96, None, None) == _capi.RTD_E_INVALID


def test_the_entry_points_are_declared_exported_and_counted():
    code = {f: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", f)).read(), flags=re.S) for f in ("rtdetr_mi355.h", "rtdetr_mi355_test.h")}
    assert "rtd_yolox_net_run_frames" in code["rtdetr_mi355.h"] and "rtd_yolox_net_run_frames" in _capi.EXPORTS and "rtd_yolox_net_run_frames" not in _capi.TEST_EXPORTS
    assert "rtd_op_yolox_focus_u8" in code["rtdetr_mi355_test.h"] and "rtd_op_yolox_focus_u8" in _capi.TEST_EXPORTS and "rtd_op_yolox_focus_u8" not in _capi.EXPORTS
    L = _capi.lib()
    assert hasattr(L, "rtd_yolox_net_run_frames") and hasattr(L, "rtd_op_yolox_focus_u8")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{len(_capi.EXPORTS)} entry points" in readme


def test_is_u8_frame():
    ok = np.zeros((4, 5, 3), np.uint8)
    assert yolox_network.is_u8_frame(ok) and yolox_network.is_u8_frame(torch.from_numpy(ok))
    for bad in (ok.astype(np.float32), torch.from_numpy(ok).float(), np.zeros((3, 4, 5), np.uint8), torch.zeros((1, 4, 5, 3), dtype=torch.uint8), np.zeros((4, 5), np.uint8),
                np.zeros((4, 5, 3), np.int8), [[1, 2, 3]]):
        assert not yolox_network.is_u8_frame(bad)


# ------------------------------------------------------------------------------------------------------------ the frontend keyword
class RecordingNetwork(yolox_network.YoloxNetwork):
    """a YoloxNetwork that owns no handle: the rows of `pred` whichever way it is called, and a record of the way"""

    def __init__(self, pred, input_size):
        self.pred, self.input_size, self.num_classes, self.max_batch = pred, input_size, pred.shape[2] - 5, 8
        self.calls = []

    def __call__(self, batch):
        self.calls.append(("batch", tuple(batch.shape)))
        return torch.from_numpy(self.pred[:batch.shape[0]])

    def run_frames(self, frames, input_size=None):
        assert all(yolox_network.is_u8_frame(f) for f in frames) and tuple(input_size) == tuple(self.input_size)
        self.calls.append(("frames", tuple(tuple(f.shape) for f in frames)))
        return torch.from_numpy(self.pred[:len(frames)])

    def close(self):
        pass


def detector(pred, frontend, **kw):
    det = yolox_detector.YOLOXDetector(device="cpu", input_size=(IN_H, IN_W), backend=yolox_ref.RefBackend(max_anchors=126), wildlife_only=False, network="mi355",
                                       frontend=frontend, **kw)
    net = RecordingNetwork(pred, (IN_H, IN_W))
    det._load_own_network = lambda: net                                  # (the checkpoint and the device are not what this test is about)
    assert det.load_model() is True and det.model is net
    return det, net


def test_frontend_keyword_values_and_the_injected_model():
    pred = yolox_ref.seeded("a126_c80")
    for bad in ("hip", "", None, "MI355"):
        with pytest.raises(ValueError, match="frontend"):
            yolox_detector.YOLOXDetector(frontend=bad)
    with pytest.raises(ValueError, match="injected model"):
        yolox_detector.YOLOXDetector(frontend="mi355", model=yolox_ref.StandInModel(pred))
    assert yolox_detector.YOLOXDetector().frontend == "auto"
    for fe in ("auto", "torch"):                                         # an injected model goes through preprocess(), uint8 frames too
        model = yolox_ref.StandInModel(pred)
        det = yolox_detector.YOLOXDetector(device="cpu", input_size=(IN_H, IN_W), model=model, backend=yolox_ref.RefBackend(max_anchors=126), wildlife_only=False, frontend=fe)
        assert det.load_model() and len(det.detect(frame(48, 80))) > 0 and model.shapes == [(1, 3, IN_H, IN_W)]
    # frontend="mi355" asks for this library's network as network="mi355" does
    assert yolox_detector.YOLOXDetector(frontend="mi355")._wants_own_network() is True


def test_which_frames_take_which_path():
    pred = yolox_ref.seeded("a126_c80")
    u8 = [frame(48, 80), frame(120, 200)]
    today, _ = detector(pred, "torch")
    want_one, want_two = today.detect(u8[0]), today.detect_batch(u8)
    assert len(want_one) > 0 and len(want_two) == 2 and want_one == want_two[0]
    for fe in ("auto", "mi355"):
        det, net = detector(pred, fe)
        assert det.detect(u8[0]) == want_one and det.detect_batch(u8) == want_two
        assert det.detect_batch([torch.from_numpy(f) for f in u8]) == want_two and det.detect(torch.from_numpy(u8[0])) == want_one
        assert net.calls == [("frames", ((48, 80, 3),)), ("frames", ((48, 80, 3), (120, 200, 3))), ("frames", ((48, 80, 3), (120, 200, 3))), ("frames", ((48, 80, 3),))]
        assert det.detect_batch([]) == []
    # "torch" never takes the fused path
    det, net = detector(pred, "torch")
    assert det.detect_batch(u8) == want_two and [c[0] for c in net.calls] == ["batch"]
    # "auto": a float tensor, a CHW tensor and a list with one float frame in it go through preprocess(), with today's result
    flt = torch.from_numpy(u8[0]).float()
    chw = torch.from_numpy(u8[0]).permute(2, 0, 1).contiguous()
    for frames, orig in (([flt], (48, 80)), ([u8[0], flt], None), ([u8[1], torch.from_numpy(u8[0]).float()], None)):
        det, net = detector(pred, "auto")
        assert det.detect_batch(frames) == today.detect_batch(frames) and [c[0] for c in net.calls] == ["batch"]
    det, net = detector(pred, "auto")
    assert det.detect(flt) == today.detect(flt) == want_one and net.calls == [("batch", (1, 3, IN_H, IN_W))]
    # a CHW tensor: detect_batch reads its size as the reference does and preprocess() permutes it as the reference does - today's
    # behaviour, whatever it is, on the same path
    det, net = detector(pred, "auto")
    try:
        want = ("ok", today.detect_batch([chw]))
    except Exception as e:                                               # noqa: BLE001
        want = ("raises", type(e))
    try:
        got = ("ok", det.detect_batch([chw]))
    except Exception as e:                                               # noqa: BLE001
        got = ("raises", type(e))
    assert got == want and all(c[0] == "batch" for c in net.calls)
    # "mi355" raises for what the kernel cannot read instead of falling back
    det, net = detector(pred, "mi355")
    for frames in ([flt], [u8[0], flt], [chw]):
        with pytest.raises(ValueError, match="frontend='mi355'"):
            det.detect_batch(frames)
    with pytest.raises(ValueError, match="frontend='mi355'"):
        det.detect(flt)
    assert net.calls == []
    # a list longer than the back end's max_batch runs as several device batches on either path
    many = [u8[i % 2] for i in range(3)]
    for fe in ("auto", "torch"):
        det, net = detector(pred, fe)
        det._backend.max_batch = 2
        out = det.detect_batch(many)
        assert out == [want_two[0], want_two[1], want_two[0]] and len(net.calls) == 2
    # no model: the reference's answers
    det = yolox_detector.YOLOXDetector(frontend="auto")
    assert det.detect(u8[0]) == [] and det.detect_batch(u8) == [[], []]
