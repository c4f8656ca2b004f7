"""The YOLOX network on the MI355X (csrc/yolox_net.hip) against the fp64 restatement (tests/yolox_net_ref.py).

The three kernels of the file are held to exact results on the smallest shapes at which each can go wrong; the whole network, for the
f16x3 and the fp32 engine alike, to a quarter of what plain fp16 costs against fp64 on the same case (tests/golden/yolox_net_yardstick.json,
tools/make_yolox_net_yardstick.py), on the head rows and - at 64 x 96 - on every named stage.  64 x 96 gives the levels 8 x 12, 4 x 6 and
2 x 3 (A = 126), 160 x 160 odd maps up to 20 x 20."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import yolox_net_ref as ref
from tests import yolox_ref
from telescope_cam_detection_amd import _capi, yolox_detector, yolox_network

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARD = json.load(open(os.path.join(ROOT, "tests", "golden", "yolox_net_yardstick.json")))["cases"]
ENGINES = ("f16x3", "fp32")
DT = {"f16x3": _capi.DT_F16X2, "fp32": _capi.DT_F32}
SENTINEL = 12345.0

_REF, _NET = {}, {}


def reference(name):
    """the fp64 restatement of a yardstick case, computed once: (head rows [n][A][5 + C], stages)"""
    if name not in _REF:
        st = {}
        out = ref.forward(ref.case_state(name), ref.case_input(name).double(), st)
        _REF[name] = (out.numpy(), {k: v.numpy() for k, v in st.items()})
    return _REF[name]


def network(name, precision, max_batch=2):
    k = (name, precision, max_batch)
    if k not in _NET:
        model = ref.E2E["model"] if name == "e2e" else ref.NET_CASES[name][0]
        _NET[k] = yolox_network.YoloxNetwork(ref.case_state(name), model, max_batch=max_batch, precision=precision)
    return _NET[k]


@pytest.fixture(scope="module", autouse=True)
def _close_networks():
    yield
    for n in _NET.values():
        n.close()
    _NET.clear()


def gate1(got, want, fp16_err, what):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: max |delta| {err:.3e} (gate {fp16_err / 4:.3e} = fp16 yardstick {fp16_err:.3e} / 4)")
    assert np.isfinite(got).all() and err <= fp16_err / 4, (what, err, fp16_err / 4)
    return err


def op_ok(rc):
    assert rc == _capi.RTD_OK, (rc, _capi.lib().rtd_yolox_net_last_error(None))


def stored(x, dtype):
    """an fp32 [..., C] array as the kernels store it: (the values they see, the device buffer as a flat tensor)"""
    if dtype == _capi.DT_F32:
        return x, torch.from_numpy(x.copy()).reshape(-1)
    s = _capi.to_split(x)
    return _capi.from_split(s), torch.from_numpy(s.view(np.int16).copy()).reshape(-1)


def read_back(t, dtype, shape):
    a = t.cpu().numpy()
    if dtype == _capi.DT_F32:
        return a.reshape(shape)
    return _capi.from_split(a.view(np.uint16).reshape(shape[:-1] + (2 * shape[-1],)))


# ------------------------------------------------------------------------------------------------------------ Focus
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("h,w,integer", [(64, 96, False), (32, 32, True)])
def test_focus_is_the_restatement_s_split_bit_for_bit(engine, h, w, integer):
    dt, n = DT[engine], 2
    x = ref.seeded_input(40 + h, n, h, w, integer=integer)
    want = np.zeros((n, h // 2, w // 2, 32), np.float32)
    want[..., :12] = ref.focus_split(torch.from_numpy(x)).permute(0, 2, 3, 1).numpy()
    want_seen, _ = stored(want, dt)
    per = 1 if dt == _capi.DT_F32 else 2                                 # buffer elements per channel
    numel, guard = want.size * per, 256
    buf = torch.full((numel + guard,), 77, dtype=torch.float32 if dt == _capi.DT_F32 else torch.int16).cuda()
    op_ok(_capi.lib().rtd_op_yolox_focus(dt, torch.from_numpy(x).cuda().data_ptr(), buf.data_ptr(), n, h, w))
    got = read_back(buf[:numel], dt, want.shape)
    assert np.array_equal(got, want_seen)
    if dt == _capi.DT_F16X2:                                             # the stored halves themselves, not only their sums
        assert np.array_equal(buf[:numel].cpu().numpy().view(np.uint16), _capi.to_split(want).reshape(-1))
    assert (got[..., 12:] == 0).all() and (buf[numel:].cpu() == 77).all()
    if not integer:
        assert (x != np.round(x)).any()


# ------------------------------------------------------------------------------------------------------------ SPP
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("h,w,c", [(2, 3, 32), (5, 5, 32), (7, 13, 256), (20, 20, 32), (23, 41, 32)])
def test_spp_pools_equal_max_pool2d_on_the_stored_values(engine, h, w, c):
    """2 x 3: every window is mostly padding; 7 x 13: one side under the 13-window, one over; 20 x 20: the map at 640 px, exactly one
    tile; 23 x 41: several tiles with ragged edges (the halo crosses tile borders)"""
    dt, n = DT[engine], 2
    rng = np.random.default_rng(h * 100 + w)
    x = rng.normal(0, 3, (n, h, w, 4 * c)).astype(np.float32)
    x[..., c:] = SENTINEL
    seen, buf = stored(x, dt)
    guard = torch.full((256,), 77, dtype=buf.dtype)
    dev = torch.cat([buf, guard]).cuda()
    op_ok(_capi.lib().rtd_op_yolox_spp(dt, dev.data_ptr(), n, h, w, c))
    got = read_back(dev[:buf.numel()], dt, x.shape)
    s0 = torch.from_numpy(seen[..., :c]).permute(0, 3, 1, 2)
    assert np.array_equal(got[..., :c], seen[..., :c]) and (dev[buf.numel():].cpu() == 77).all()
    p = s0
    for k, win in enumerate((5, 9, 13), 1):
        p = ref.pool5(p)
        assert torch.equal(p, F.max_pool2d(s0, win, 1, win // 2)), win                     # pool9 = pool5 o pool5, pool13 = pool5^3
        assert np.array_equal(got[..., k * c:(k + 1) * c], p.permute(0, 2, 3, 1).numpy()), (win, h, w)


# ------------------------------------------------------------------------------------------------------------ head emit
@pytest.mark.parametrize("num_classes", [80, 3])
def test_head_emit_rows_order_and_sigmoids(num_classes):
    n, in_h, in_w = 2, 64, 96
    cls_ld, ro_ld = (num_classes + 31) // 32 * 32, 32
    rng = np.random.default_rng(num_classes)
    cls, ro, want = [], [], []
    for s in yolox_ref.STRIDES:
        hw = (in_h // s) * (in_w // s)
        c = rng.normal(0, 4, (n, hw, cls_ld)).astype(np.float32)
        r = rng.normal(0, 4, (n, hw, ro_ld)).astype(np.float32)
        c[0, 0, :3] = (100.0, -100.0, np.nan)
        c[1, hw - 1, :3] = (0.0, -0.0, 88.0)
        r[0, hw - 1, 4], r[1, 0, 4] = -100.0, np.nan
        cls.append(c), ro.append(r)
        want.append(np.concatenate([r[..., :4].astype(np.float64), 1 / (1 + np.exp(-r[..., 4:5].astype(np.float64))),
                                    1 / (1 + np.exp(-c[..., :num_classes].astype(np.float64)))], 2))
    want = np.concatenate(want, 1)                                       # levels in stride order, row-major within a level
    A, Fw = yolox_ref.anchors(in_h, in_w), 5 + num_classes
    assert want.shape == (n, A, Fw) and A == 126
    dcls, dro = [torch.from_numpy(a).cuda() for a in cls], [torch.from_numpy(a).cuda() for a in ro]
    buf = torch.full((1 + n * A * Fw + 64,), SENTINEL, dtype=torch.float32).cuda()
    pred_ptr = buf.data_ptr() + 4                                        # 4-byte aligned and no more
    assert pred_ptr % 8 == 4
    pc, pr = (C.c_void_p * 3)(*[t.data_ptr() for t in dcls]), (C.c_void_p * 3)(*[t.data_ptr() for t in dro])
    op_ok(_capi.lib().rtd_op_yolox_head_emit(pc, pr, cls_ld, ro_ld, n, in_h, in_w, num_classes, C.c_void_p(pred_ptr)))
    out = buf.cpu().numpy()
    assert out[0] == SENTINEL and (out[1 + n * A * Fw:] == SENTINEL).all()
    got = out[1:1 + n * A * Fw].reshape(n, A, Fw)
    assert np.array_equal(got[..., :4].view(np.uint32), want[..., :4].astype(np.float32).view(np.uint32))       # box terms: the conv rows' bits
    nan = np.isnan(want[..., 4:])
    assert nan.sum() == 2 * 3 and np.array_equal(np.isnan(got[..., 4:]), nan)
    err = np.abs(got[..., 4:].astype(np.float64) - want[..., 4:])[~nan].max()
    print(f"head emit C = {num_classes}: worst sigmoid error {err:.3e} (bound 2^-22 = {2.0 ** -22:.3e})")
    assert err <= 2.0 ** -22
    assert got[0, 0, 5] == 1.0 and got[0, 0, 6] == 0.0 and got[1, (in_h // 8) * (in_w // 8) - 1, 5] == 0.5 and got[1, (in_h // 8) * (in_w // 8) - 1, 6] == 0.5


# ------------------------------------------------------------------------------------------------------------ the whole network
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", list(ref.NET_CASES))
def test_network_against_fp64(name, engine):
    want, stages = reference(name)
    net = network(name, engine)
    got = net(ref.case_input(name).cuda()).cpu().numpy()
    assert got.shape == want.shape
    yard = YARD[name]["errors"]
    gate1(got, want, yard["head"]["fp16"], f"{name} {engine} head rows")
    if name == "s_64x96_n2":
        for st in ref.STAGES:
            t = net.debug_tensor(st)
            assert t.shape == stages[st].shape, st
            gate1(t, stages[st], yard[st]["fp16"], f"{name} {engine} {st}")


# ------------------------------------------------------------------------------------------------------------ handle behaviour
def test_handle_sizes_refusals_and_repeats():
    net = network("s_64x96_n2", "f16x3")
    big = torch.from_numpy(ref.seeded_input(9, 2, 160, 160)).cuda()
    small = ref.case_input("s_64x96_n2").cuda()
    first = net(big)
    arena = net.arena_bytes()
    assert arena > 0
    a = net(small[:1])                                                   # a small call after a large one, another input size on one handle
    assert net.arena_bytes() == arena
    pred = torch.empty_like(a)
    stream = torch.cuda.current_stream().cuda_stream
    L = _capi.lib()
    for args, why in (((3, small.data_ptr(), 64, 96, pred.data_ptr()), "max_batch"), ((0, small.data_ptr(), 64, 96, pred.data_ptr()), "max_batch"),
                      ((1, small.data_ptr(), 64, 100, pred.data_ptr()), "multiple of 32"), ((1, None, 64, 96, pred.data_ptr()), "null"),
                      ((1, small.data_ptr(), 64, 96, None), "null"), ((1, small.data_ptr() + 4, 64, 96, pred.data_ptr()), "16-byte")):
        assert net.run_raw(*args, stream) == _capi.RTD_E_INVALID, args
        assert why in L.rtd_yolox_net_last_error(net._h).decode(), (why, L.rtd_yolox_net_last_error(net._h))
    assert torch.equal(net(small[:1]), a) and torch.equal(net(big), first) and net.arena_bytes() == arena
    # batches above max_batch run as several calls
    three = torch.cat([small, small[:1]])
    assert torch.equal(net(three)[2], a[0])
    # refused configs and blobs: nothing is left behind, the message names the reason
    sd = ref.case_state("s_64x96_n2")
    with pytest.raises(_capi.RtdError, match="bf16") as e:
        yolox_network.YoloxNetwork(sd, "yolox-s", precision="bf16")
    assert e.value.code == _capi.RTD_E_INVALID
    with pytest.raises(_capi.RtdError, match="not this variant") as e:
        bad = yolox_network.YoloxNetwork.__new__(yolox_network.YoloxNetwork)
        cfg = _capi.RtdYoloxNetConfig()
        cfg.struct_size, cfg.precision, cfg.num_classes, cfg.base_channels, cfg.depth, cfg.max_batch = C.sizeof(cfg), _capi.PREC_F16X3, 80, 64, 3, 1
        blob = yolox_network.fold_state(sd, yolox_network.variant_of("yolox-s", sd))
        bad._open(C.byref(cfg), (C.c_char * len(blob)).from_buffer_copy(blob), len(blob))
    assert e.value.code == _capi.RTD_E_INVALID
    nan = dict(sd)
    key = "backbone.C3_p3.m.0.conv2.conv.weight"
    nan[key] = sd[key].clone()
    nan[key][3, 2, 1, 1] = float("nan")
    with pytest.raises(_capi.RtdError, match=r"backbone\.C3_p3\.m\.0\.conv2\.weight holds a NaN") as e:
        yolox_network.YoloxNetwork(nan, "yolox-s")
    assert e.value.code == _capi.RTD_E_WEIGHTS


# ------------------------------------------------------------------------------------------------------------ end to end
def test_detector_with_the_library_s_network_equals_the_fp64_restatement(tmp_path):
    sd = ref.case_state("e2e")
    path = tmp_path / "yolox_s_seeded.pth"
    torch.save({"model": sd, "start_epoch": 300}, path)
    size = tuple(ref.E2E["input_size"])
    det = yolox_detector.YOLOXDetector(model_path=str(path), network="mi355", input_size=size, wildlife_only=False)
    want_det = yolox_detector.YOLOXDetector(model=ref.RefModel(sd, torch.float64), backend=yolox_ref.RefBackend(), decode=True, input_size=size,
                                            wildlife_only=False)
    try:
        assert det.load_model() and want_det.load_model()
        assert det.decode is True and det.num_classes == ref.E2E["classes"] and isinstance(det.model, yolox_network.YoloxNetwork)
        frames = ref.e2e_frames()
        assert frames[0].shape != frames[1].shape
        got = [det.detect(frames[0])] + det.detect_batch(frames)
        want = [want_det.detect(frames[0])] + want_det.detect_batch(frames)
        gate = YARD["e2e"]["errors"]["head"]["fp16"] / 4
        worst_c = worst_b = 0.0
        for g, w_ in zip(got, want):
            assert len(g) == len(w_) >= 20
            assert [d["class_id"] for d in g] == [d["class_id"] for d in w_] and [d["class_name"] for d in g] == [d["class_name"] for d in w_]
            for a, b in zip(g, w_):
                assert set(a) == set(b) and set(a["bbox"]) == set(b["bbox"])
                worst_c = max(worst_c, abs(a["confidence"] - b["confidence"]))
                assert abs(a["confidence"] - b["confidence"]) <= gate
                tol = gate * max(b["bbox"]["x2"] - b["bbox"]["x1"], b["bbox"]["y2"] - b["bbox"]["y1"])    # (frame pixels: the ratio is in them)
                for k in ("x1", "y1", "x2", "y2"):
                    worst_b = max(worst_b, abs(a["bbox"][k] - b["bbox"][k]) / tol)
                    assert abs(a["bbox"][k] - b["bbox"][k]) <= tol, (k, a, b)
        print(f"end to end: {[len(g) for g in got]} detections, worst confidence delta {worst_c:.3e} (gate {gate:.3e}), worst box delta {worst_b:.3e} of its tolerance")
    finally:
        det.close()
        want_det.close()
