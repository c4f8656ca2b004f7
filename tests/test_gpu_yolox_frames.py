"""The YOLOX uint8 front end on the MI355X (csrc/yolox_net.hip yolox_focus_u8, rtd_yolox_net_run_frames, YoloxNetwork.run_frames,
YOLOXDetector(frontend=...)) against the numpy float32 restatement (tests/yolox_frames_ref.py), which has the kernel's operation order
and therefore its bits: the Focus map from the bytes must equal rtd_op_yolox_focus of the uploaded restatement bit for bit, and the
whole call must equal rtd_yolox_net_run on it.  Against torch's own F.interpolate on the device the two camera sizes are exact and any
other size lies inside one ulp of a source coordinate times the largest pixel step."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import yolox_frames_ref as fr
from tests import yolox_net_ref as ref
from telescope_cam_detection_amd import _capi, yolox_detector, yolox_network

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARD = json.load(open(os.path.join(ROOT, "tests", "golden", "yolox_net_yardstick.json")))["cases"]
ENGINES = ("f16x3", "fp32")
DT = {"f16x3": _capi.DT_F16X2, "fp32": _capi.DT_F32}
IN_H, IN_W = 64, 96
GUARD = 256            # buffer elements on either side of an output (a multiple of 16 bytes in both storage types)
BOUND_TORCH = 255 * 2.0 ** -12

_NET = {}


def network(precision):
    if precision not in _NET:
        _NET[precision] = yolox_network.YoloxNetwork(ref.case_state("s_64x96_n2"), "yolox-s", max_batch=2, precision=precision, input_size=(IN_H, IN_W))
    return _NET[precision]


@pytest.fixture(scope="module", autouse=True)
def _close_networks():
    yield
    for n in _NET.values():
        n.close()
    _NET.clear()


def op_ok(rc):
    assert rc == _capi.RTD_OK, (rc, _capi.lib().rtd_yolox_net_last_error(None))


def out_buffer(dt, n, in_h, in_w):
    """a guarded Focus output: (the whole buffer, the 16-byte aligned address of the map, its elements)"""
    numel = n * (in_h // 2) * (in_w // 2) * 32 * (1 if dt == _capi.DT_F32 else 2)
    buf = torch.full((numel + 2 * GUARD,), 77, dtype=torch.float32 if dt == _capi.DT_F32 else torch.int16).cuda()
    ptr = buf.data_ptr() + GUARD * buf.element_size()
    assert ptr % 16 == 0
    return buf, ptr, numel


def focus_of_float(dt, x):
    """rtd_op_yolox_focus of a float32 [n][3][h][w] batch: the raw storage as a flat CPU tensor"""
    n, _, h, w = x.shape
    buf, ptr, numel = out_buffer(dt, n, h, w)
    dev = torch.from_numpy(x).cuda()
    op_ok(_capi.lib().rtd_op_yolox_focus(dt, dev.data_ptr(), C.c_void_p(ptr), n, h, w))
    return buf[GUARD:GUARD + numel].cpu()


def focus_of_frames(dt, ptrs, hw, in_h, in_w):
    """rtd_op_yolox_focus_u8: (the raw storage as a flat CPU tensor, the guards)"""
    buf, ptr, numel = out_buffer(dt, len(hw), in_h, in_w)
    frames, sizes = yolox_network.frame_arrays(ptrs, hw)
    op_ok(_capi.lib().rtd_op_yolox_focus_u8(dt, frames, sizes, len(hw), in_h, in_w, C.c_void_p(ptr)))
    out = buf.cpu()
    return out[GUARD:GUARD + numel], torch.cat([out[:GUARD], out[GUARD + numel:]])


def as_float(raw, dt, shape):
    a = raw.numpy()
    if dt == _capi.DT_F32:
        return a.reshape(shape)
    return _capi.from_split(a.view(np.uint16).reshape(shape[:-1] + (2 * shape[-1],)))


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("sizes", [((48, 80), (120, 200), (64, 96)), ((37, 53), (1, 1), (3, 2000))])
def test_mixed_sizes_in_one_launch_are_the_restatement_s_focus_bit_for_bit(engine, sizes):
    """an up-scale, a down-scale and the identity; an odd size, one pixel and a 3-row strip: three frames of one launch, carved from one
    byte buffer at addresses 1, 2 and 3 mod 4"""
    dt = DT[engine]
    frames = [fr.seeded_frame(100 * h + w, h, w) for h, w in sizes]
    host, starts = fr.carve(frames, offsets=(1, 2, 3))
    dev = torch.from_numpy(host).cuda()
    ptrs = [dev.data_ptr() + s for s in starts]
    assert [p % 4 for p in ptrs] == [1, 2, 3]
    got, guards = focus_of_frames(dt, ptrs, sizes, IN_H, IN_W)
    want = focus_of_float(dt, fr.batch(frames, IN_H, IN_W))
    assert torch.equal(got, want)                                        # the stored bits (pairs: both halves)
    shape = (3, IN_H // 2, IN_W // 2, 32)
    vals = as_float(got, dt, shape)
    assert (vals[..., 12:] == 0).all() and (vals[..., :12] >= 0).all() and (vals[..., :12] <= 255).all() and vals[..., :12].std() > 10
    assert (guards == 77).all()
    assert np.array_equal(dev.cpu().numpy(), host)                       # the frames and the bytes between them


@pytest.mark.parametrize("engine", ENGINES)
def test_a_frame_at_the_input_size_passes_as_its_integers(engine):
    dt = DT[engine]
    f = fr.seeded_frame(7, IN_H, IN_W)
    dev = torch.from_numpy(f).cuda()
    got, guards = focus_of_frames(dt, [dev.data_ptr()], [(IN_H, IN_W)], IN_H, IN_W)
    want = focus_of_float(dt, torch.from_numpy(f).float().permute(2, 0, 1).unsqueeze(0).contiguous().numpy())
    assert torch.equal(got, want) and (guards == 77).all()
    vals = as_float(got, dt, (1, IN_H // 2, IN_W // 2, 32))
    assert vals[0, 3, 5, 0] == f[6, 10, 0] and vals[0, 3, 5, 3 + 1] == f[7, 10, 1] and vals[0, 3, 5, 6 + 2] == f[6, 11, 2] and vals[0, 3, 5, 9] == f[7, 11, 0]


# ------------------------------------------------------------------------------------------------------------ the whole call
@pytest.mark.parametrize("engine", ENGINES)
def test_run_frames_equals_run_on_the_restatement_s_batch(engine):
    net = network(engine)
    frames = [fr.seeded_frame(31, 48, 80), fr.seeded_frame(32, 120, 200)]                   # one up-scaled, one down-scaled
    want = net(torch.from_numpy(fr.batch(frames, IN_H, IN_W)).cuda())
    want_focus = net.debug_tensor("focus")
    arena = net.arena_bytes()
    assert arena > 0
    got = net.run_frames(frames)
    assert got.shape == want.shape == (2, 126, 85) and torch.equal(got, want)
    focus = net.debug_tensor("focus")
    assert focus.shape == (2, IN_H // 2, IN_W // 2, 32) and np.array_equal(focus, want_focus) and focus[..., :12].std() > 10
    # device tensors are read in place and give the same rows
    assert torch.equal(net.run_frames([torch.from_numpy(f).cuda() for f in frames]), want)
    # other sizes on the same handle: the same plan, nothing allocated
    others = [fr.seeded_frame(33, 37, 53), fr.seeded_frame(34, 3, 2000)]
    other = net.run_frames(others)
    assert net.arena_bytes() == arena and torch.equal(other, net(torch.from_numpy(fr.batch(others, IN_H, IN_W)).cuda())) and not torch.equal(other, want)
    assert net.arena_bytes() == arena
    # a refused call between two valid ones: the outputs are untouched, the next call is bit-identical
    dev = [torch.from_numpy(f).cuda() for f in frames]
    pred = torch.full_like(want, 5.0)
    stream = torch.cuda.current_stream().cuda_stream
    ptrs, hw = [t.data_ptr() for t in dev], [(48, 80), (120, 200)]
    L = _capi.lib()
    for args, why in (((2, [ptrs[0], 0], hw, IN_H, IN_W), "frame 1: null"), ((2, None, hw, IN_H, IN_W), "null"), ((2, ptrs, [(48, 80), (0, 200)], IN_H, IN_W), "sides"),
                      ((2, ptrs, [(48, 80), (120, 16385)], IN_H, IN_W), "sides"), ((3, ptrs + ptrs[:1], hw + hw[:1], IN_H, IN_W), "max_batch"),
                      ((2, ptrs, hw, IN_H, 100), "multiple of 32")):
        assert net.run_frames_raw(*args, pred.data_ptr(), stream) == _capi.RTD_E_INVALID, args
        assert why in L.rtd_yolox_net_last_error(net._h).decode(), (why, L.rtd_yolox_net_last_error(net._h))
    assert net.run_frames_raw(2, ptrs, hw, IN_H, IN_W, None, stream) == _capi.RTD_E_INVALID
    torch.cuda.synchronize()
    assert (pred == 5.0).all() and net.arena_bytes() == arena
    assert net.run_frames_raw(2, ptrs, hw, IN_H, IN_W, pred.data_ptr(), stream) == _capi.RTD_OK
    assert torch.equal(pred, want) and torch.equal(net.run_frames(frames), want)
    # lists longer than max_batch run as several calls
    three = net.run_frames(frames + others[:1])
    assert torch.equal(three[:2], want) and torch.equal(three[2], net.run_frames(others[:1])[0])
    with pytest.raises(TypeError, match="uint8"):
        net.run_frames([frames[0].astype(np.float32)])


# ------------------------------------------------------------------------------------------------------------ against torch on the device
@pytest.mark.parametrize("h,w,in_h,in_w,bound", [(1080, 1920, 640, 640, 0.0), (1440, 2560, 640, 640, 0.0), (120, 200, IN_H, IN_W, BOUND_TORCH)])
def test_focus_map_against_focus_of_interpolate_on_the_device(h, w, in_h, in_w, bound):
    """1080 / 640 = 1.6875, 1920 / 640 = 3, 1440 / 640 = 2.25 and 2560 / 640 = 4 are dyadic, so every source coordinate is exact: exact.  Elsewhere
    torch may order or contract the index arithmetic differently: one ulp of a coordinate below 2048 (2^-12) times 255"""
    f = fr.seeded_frame(h + w, h, w)
    dev = torch.from_numpy(f).cuda()
    got, guards = focus_of_frames(_capi.DT_F32, [dev.data_ptr()], [(h, w)], in_h, in_w)
    got = as_float(got, _capi.DT_F32, (1, in_h // 2, in_w // 2, 32))
    resized = F.interpolate(dev.permute(2, 0, 1).unsqueeze(0).float(), size=(in_h, in_w), mode="bilinear", align_corners=False)
    want = ref.focus_split(resized).permute(0, 2, 3, 1).cpu().numpy()
    err = float(np.abs(got[..., :12] - want).max())
    print(f"{h} x {w} -> {in_h} x {in_w}: fused Focus map against Focus of F.interpolate on the device, max |delta| {err:.3e} (bound {bound:.4f})")
    assert err <= bound and (got[..., 12:] == 0).all() and (guards == 77).all()


# ------------------------------------------------------------------------------------------------------------ the detector
def test_detector_front_ends_agree_end_to_end(tmp_path):
    """the two scene frames of the end-to-end case (120 x 200 and 240 x 176 -> 160 x 160), as numpy frames and as device tensors, through
    detect and detect_batch: the fused front end against preprocess().  The case's margins to both thresholds exceed 100 x its recorded
    fp32 head error (tests/test_yolox_net_host.py), which is the gate here"""
    sd = ref.case_state("e2e")
    path = tmp_path / "yolox_s_seeded.pth"
    torch.save({"model": sd, "start_epoch": 300}, path)
    size = tuple(ref.E2E["input_size"])
    dets = {fe: yolox_detector.YOLOXDetector(model_path=str(path), network="mi355", input_size=size, wildlife_only=False, frontend=fe) for fe in ("mi355", "auto", "torch")}
    assert yolox_detector.YOLOXDetector(model_path=str(path), network="mi355").frontend == "auto"                      # the default
    try:
        assert all(d.load_model() for d in dets.values())
        calls = {}
        for fe, d in dets.items():
            assert isinstance(d.model, yolox_network.YoloxNetwork) and d.decode is True
            calls[fe] = []
            inner = d.model.run_frames
            d.model.run_frames = lambda frames, input_size=None, _inner=inner, _log=calls[fe]: (_log.append(len(frames)), _inner(frames, input_size))[1]
        frames = ref.e2e_frames()
        assert [f.shape for f in frames] == [(120, 200, 3), (240, 176, 3)] and all(f.dtype == np.uint8 for f in frames)
        on_dev = [torch.from_numpy(f).cuda() for f in frames]

        def answers(d):
            return [d.detect(frames[0]), d.detect(on_dev[1])] + d.detect_batch(frames) + d.detect_batch(on_dev)

        got, want, auto = answers(dets["mi355"]), answers(dets["torch"]), answers(dets["auto"])
        assert calls["mi355"] == [1, 1, 2, 2] and calls["torch"] == [] and calls["auto"] == [1, 1, 2, 2]
        assert auto == got                                               # "auto" IS the fused path for these frames
        gate = 100.0 * YARD["e2e"]["errors"]["head"]["fp32"]
        worst_c = worst_b = 0.0
        for g, w_ in zip(got, want):
            assert len(g) == len(w_) >= 20
            assert [d["class_id"] for d in g] == [d["class_id"] for d in w_] and [d["class_name"] for d in g] == [d["class_name"] for d in w_]
            for a, b in zip(g, w_):
                assert set(a) == set(b) and set(a["bbox"]) == set(b["bbox"])
                worst_c = max(worst_c, abs(a["confidence"] - b["confidence"]))
                tol = gate * max(b["bbox"]["x2"] - b["bbox"]["x1"], b["bbox"]["y2"] - b["bbox"]["y1"])    # (frame pixels: the ratio is in them)
                for k in ("x1", "y1", "x2", "y2"):
                    worst_b = max(worst_b, abs(a["bbox"][k] - b["bbox"][k]) / tol)
        print(f"front ends end to end: {[len(g) for g in got]} detections, worst confidence delta {worst_c:.3e} (gate {gate:.3e}), worst box delta {worst_b:.3e} of its tolerance")
        assert worst_c <= gate and worst_b <= 1.0
        assert got[2:4] == got[4:6]                                      # numpy frames or device frames: the same bytes, the same rows
    finally:
        for d in dets.values():
            d.close()
