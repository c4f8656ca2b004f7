"""The overlay renderer on the MI355X (csrc/overlay.hip): every comparison is exact equality with the numpy restatement
(tests/overlay_ref.py) - frame shapes around the tile size, one and three channels, host and device frames, in place and out of place,
hand-made and seeded primitive lists, a mixed batch, the launched tile count, the limits, stream ordering, the MJPEG tick and a whole
1080p web overlay."""
import numpy as np
import pytest
import torch

from tests import jpeg_ref
from tests import overlay_ref as ref
from tests.overlay_ref import FILL, MASK, OUTLINE, prim, prims
from telescope_cam_detection_amd import _capi, overlay as ov
from telescope_cam_detection_amd.synth import scene_frame

pytestmark = pytest.mark.gpu

MASKS = np.random.default_rng(11).integers(0, 256, 4096, dtype=np.uint8)
MASKS[::5] = 0
MASKS[1::5] = 255


@pytest.fixture(scope="module")
def be():
    b = ov.DeviceBackend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def tile(be):
    th, tw, _ = be.tiles()
    assert th >= 1 and tw >= 1
    return th, tw


def seeded(seed, n, H, W):
    """n primitives of every kind around and across an H x W frame; masks are windows of MASKS"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        kind = int(rng.integers(0, 3))
        x, y = int(rng.integers(-W // 4 - 4, W + W // 4 + 4)), int(rng.integers(-H // 4 - 4, H + H // 4 + 4))
        bgr = tuple(int(v) for v in rng.integers(0, 256, 3))
        if kind == MASK:
            w, h = int(rng.integers(1, 40)), int(rng.integers(1, 24))
            out.append(prim(MASK, x, y, w, h, bgr, mask_offset=int(rng.integers(0, len(MASKS) - w * h))))
        else:
            x2, y2 = x + int(rng.integers(-W // 2 - 2, W // 2 + 2)), y + int(rng.integers(-H // 2 - 2, H // 2 + 2))
            out.append(prim(kind, x, y, x2, y2, bgr, int(rng.integers(1, 8)) if kind == OUTLINE else 0))
    return prims(*out)


def cases(H, W, tile):
    th, tw = tile
    c = {"none": prims()}
    c["outside"] = prims(prim(FILL, W, 0, W + 30, H, (1, 2, 3)), prim(OUTLINE, 0, H + 4, W, H + 20, (1, 2, 3), 7), prim(MASK, -50, -30, 40, 20, (1, 2, 3)),
                         prim(FILL, -9, -9, -1, H + 9, (1, 2, 3)), prim(OUTLINE, -40, -40, -4, -4, (4, 5, 6), 7), prim(MASK, W, H, 10, 10, (7, 8, 9)))
    c["partly_outside"] = prims(prim(FILL, -7, H // 3, W // 4, H // 2, (10, 20, 30)), prim(FILL, W - 1 - W // 4, -5, W + 9, H // 4, (40, 50, 60)),
                                prim(FILL, W // 3, H - 1 - H // 5, W // 2, H + 3, (70, 80, 90)), prim(FILL, W // 2, -3, W // 2 + 2, 0, (100, 110, 120)),
                                prim(OUTLINE, -2, -2, W + 1, H + 1, (130, 140, 150), 7), prim(OUTLINE, -1, H // 2, W, H + 5, (160, 170, 180), 2),
                                prim(MASK, -5, -3, 30, 12, (190, 200, 210), mask_offset=100), prim(MASK, W - 6, H - 4, 30, 12, (220, 230, 240), mask_offset=700))
    c["inverted"] = prims(prim(FILL, W // 2, H // 2, W // 5, H // 5, (9, 99, 199)), prim(OUTLINE, W - 2, H - 2, 1, 1, (19, 29, 39), 3),
                          prim(OUTLINE, W // 4, H - 1, W - W // 4, 0, (49, 59, 69), 2))
    for t in (1, 2, 3, 7):                                   # boxes whose strips run through the corners where four tiles meet
        c[f"outline_t{t}"] = prims(prim(OUTLINE, tw - 5, th - 4, tw + 9, th + 6, (11, 22, 33), t), prim(OUTLINE, tw - 1, th - 1, 2 * tw, 2 * th, (44, 55, 66), t),
                                   prim(OUTLINE, tw, th, 3 * tw - 1, 3 * th - 1, (77, 88, 99), t), prim(OUTLINE, 2, 1, W - 3, H - 2, (111, 122, 133), t))
    c["masks"] = prims(prim(MASK, tw - 3, th - 2, 9, 7, (255, 0, 128), mask_offset=5), prim(MASK, W - 4, H - 3, 10, 8, (0, 255, 64), mask_offset=300),
                       prim(MASK, tw - 20, 2 * th - 1, 39, 2, (90, 90, 250), mask_offset=1000), prim(MASK, 0, 0, 0, 5, (1, 1, 1)), prim(MASK, 1, 1, 1, 1, (200, 100, 50), mask_offset=1))
    c["order"] = seeded(1000 + H + W, 40, H, W)
    c["whole"] = prims(prim(FILL, 0, 0, W - 1, H - 1, (12, 34, 56)), prim(MASK, 0, 0, min(W, 40), min(H, 20), (250, 240, 230), mask_offset=2000))
    c["many"] = seeded(2000 + H + W, 300, H, W)             # more than one round of 256 in the kernel's compaction
    return c


def shapes(tile):
    th, tw = tile
    return [(1, 1), (5, 8), (37, 53), (th, tw), (th + 1, tw + 1), (130, 250), (487, 641)]


_REF = {}


def reference(H, W, C, tile):
    """(names, frames, primitive lists, composited frames) of a shape: computed once"""
    key = (H, W, C)
    if key not in _REF:
        cs = cases(H, W, tile)
        names = list(cs)
        rng = np.random.default_rng(H * 1000 + W + C)
        frames = [rng.integers(0, 256, (H, W, C), dtype=np.uint8) for _ in names]
        want = [ref.composite(f, cs[n], MASKS) for f, n in zip(frames, names)]
        _REF[key] = (names, frames, [cs[n] for n in names], want)
    return _REF[key]


def run(be, frames, plists, mode):
    """-> (outputs as numpy, inputs after the call as numpy, the tensors returned, the tensors given)"""
    if mode == "host":
        given = [f.copy() for f in frames]
        outs = be.draw(given, False, plists, MASKS, False)
        after = given
    else:
        given = [torch.from_numpy(f).cuda() for f in frames]
        torch.cuda.synchronize()
        outs = be.draw(given, True, plists, MASKS, mode == "device_inplace")
        after = [g.cpu().numpy() for g in given]
    return [o.cpu().numpy() for o in outs], after, outs, given


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mode", ["host", "device", "device_inplace"])
def test_every_shape_and_primitive_list_equals_the_restatement(be, tile, C, mode):
    for H, W in shapes(tile):
        names, frames, plists, want = reference(H, W, C, tile)
        got, after, outs, given = run(be, frames, plists, mode)
        assert be.tiles()[2] == sum(ref.tiles_touched(p, (H, W, C), tile) for p in plists), (H, W)
        for n, g, w, a, f, o, gv in zip(names, got, want, after, frames, outs, given):
            assert g.shape == (H, W, C) and (g == w).all(), (H, W, C, mode, n, int((g != w).sum()), np.argwhere(g != w)[:3].tolist())
            if mode == "device_inplace":
                assert o is gv
            else:
                assert (a == f).all(), (H, W, C, mode, n, "the input frame changed")
        assert (got[names.index("none")] == frames[names.index("none")]).all()
        assert (got[names.index("outside")] == frames[names.index("outside")]).all()


def test_one_batch_of_six_frames_of_different_sizes_and_counts(be, tile):
    hw = [(37, 53, 3), (130, 250, 1), (5, 8, 3), (tile[0] + 1, tile[1] + 1, 3), (200, 333, 3), (64, 48, 1)]
    counts = [7, 300, 0, 40, 513, 1]
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s in hw]
    plists = [seeded(70 + i, n, s[0], s[1]) for i, (s, n) in enumerate(zip(hw, counts))]
    want = [ref.composite(f, p, MASKS) for f, p in zip(frames, plists)]
    for mode in ("host", "device", "device_inplace"):
        got, _, _, _ = run(be, frames, plists, mode)
        for i, (g, w) in enumerate(zip(got, want)):
            assert (g == w).all(), (mode, i, hw[i])
        assert be.tiles()[2] == sum(ref.tiles_touched(p, s, tile) for p, s in zip(plists, hw))
    assert (want[2] == frames[2]).all()


def test_past_the_limits_the_call_is_refused_and_nothing_is_drawn(be):
    a = np.full((20, 30, 3), 7, np.uint8)
    dev = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    one = prims(prim(FILL, 0, 0, 29, 19, (1, 1, 1)))
    many = prims(*([one] * (ov.MAX_PRIMS + 1)))
    assert be.draw_raw([dev.data_ptr()], [a.shape], True, [many], MASKS, [dev.data_ptr()]) == _capi.RTD_E_INVALID
    assert b"primitives" in be._L.rtd_overlay_last_error(be._h)
    n = ov.MAX_FRAMES + 1
    assert be.draw_raw([dev.data_ptr()] * n, [a.shape] * n, True, [one] * n, MASKS, [dev.data_ptr()] * n) == _capi.RTD_E_INVALID
    for bad in (prim(MASK, 0, 0, 8, 8, mask_offset=len(MASKS) - 63), prim(MASK, 0, 0, 8, 8, mask_offset=-1), prim(OUTLINE, 0, 0, 5, 5, thickness=0),
                prim(3, 0, 0, 5, 5), prim(MASK, 0, 0, -1, 4)):
        assert be.draw_raw([dev.data_ptr()], [a.shape], True, [prims(one, bad)], MASKS, [dev.data_ptr()]) == _capi.RTD_E_INVALID, bad
    for shape in ((20, 30, 2), (0, 30, 3), (20, 65536, 3)):
        assert be.draw_raw([dev.data_ptr()], [shape], True, [one], MASKS, [dev.data_ptr()]) == _capi.RTD_E_INVALID, shape
    assert be.draw_raw([None], [a.shape], True, [one], MASKS, [dev.data_ptr()]) == _capi.RTD_E_INVALID
    assert be.tiles()[2] == 0
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == a).all()                                   # none of the refused calls drew
    at_limit = prims(*([one] * ov.MAX_PRIMS))
    assert be.draw_raw([dev.data_ptr()], [a.shape], True, [at_limit], MASKS, [dev.data_ptr()]) == _capi.RTD_OK
    assert (dev.cpu().numpy() == 1).all()                                   # the handle is still good, and the limit itself is allowed


def test_a_frame_written_on_a_side_stream_just_before_the_call_is_the_one_drawn_on():
    r = ov.OverlayRenderer(device=0, rasteriser=ref.FakeRasteriser())
    a, b = scene_frame(7, 720, 1280), scene_frame(8, 720, 1280)
    s = ref.load_golden()["scenarios"]
    result = [x for x in s if x["name"] == "web_floats_inverted"][0]["result"]
    plan = ov.plan_web(result, r.rasteriser)
    p, m = ov.lower([plan], r.cache)
    want = ref.composite(b, p[0], m)
    frame = torch.from_numpy(a).cuda()
    src = torch.from_numpy(b).cuda()
    big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):
            big.fill_(1)                                                    # keeps the side stream busy ahead of the write
        frame.copy_(src)
        got = r.draw_batch([frame], [plan], inplace=True)[0]
    assert got is frame and (got.cpu().numpy() == want).all()
    r.close()


def test_mjpeg_tick_bytes_equal_the_restatements_jpeg_of_the_restatements_frame():
    r = ov.OverlayRenderer(device=0, rasteriser=ref.FakeRasteriser())
    s = {x["name"]: x for x in ref.load_golden()["scenarios"]}
    frames = [scene_frame(9, 64, 48), scene_frame(10, 130, 250)]
    results = [s["web_top_edge"]["result"], s["web_species"]["result"]]
    want = []
    for f, res in zip(frames, results):
        p, m = ov.lower([ov.plan_web(res, r.rasteriser)], r.cache)
        drawn = ref.composite(f, p[0], m)
        assert (drawn != f).any()
        want.append(jpeg_ref.encode(drawn, 90))
    dev = [torch.from_numpy(f).cuda() for f in frames]
    assert r.mjpeg_tick(dev, results, 90) == want
    assert r.mjpeg_tick(frames, results, 90) == want                        # host frames: uploaded, drawn, encoded
    assert r.mjpeg_tick([dev[0], frames[1]], results, 90) == want           # a mixed batch
    assert all((d.cpu().numpy() == f).all() for d, f in zip(dev, frames))   # the cameras' frames stay as they were
    assert r.mjpeg_tick(dev[:1], [None], 90) == [jpeg_ref.encode(frames[0], 90)]
    r.close()


def test_a_1080p_frame_with_the_fixtures_web_scenario_compared_whole(tile):
    r = ov.OverlayRenderer(device=0, rasteriser=ref.FakeRasteriser())
    res = [x for x in ref.load_golden()["scenarios"] if x["name"] == "web_1080p"][0]["result"]
    f = scene_frame(40, 1080, 1920)
    p, m = ov.lower([ov.plan_web(res, r.rasteriser)], r.cache)
    want = ref.composite(f, p[0], m)
    dev = torch.from_numpy(f).cuda()
    got = r.web_draw(dev, res)
    assert got.is_cuda and got.data_ptr() != dev.data_ptr() and (got.cpu().numpy() == want).all()
    touched = ref.tiles_touched(p[0], f.shape, tile)
    assert r._backend.tiles()[2] == touched and 0 < touched < -(-1080 // tile[0]) * -(-1920 // tile[1])     # sparse: not every tile
    assert (dev.cpu().numpy() == f).all()
    r.close()


def test_draw_detections_and_install_keep_device_frames_on_the_device():
    import types
    r = ov.OverlayRenderer(device=0, rasteriser=ref.FakeRasteriser())
    s = [x for x in ref.load_golden()["scenarios"] if x["name"] == "snap_species"][0]
    f = scene_frame(12, *s["hw"])
    p, m = ov.lower([ov.plan_snapshot(s["detections"], 3, 0.7, True, rasteriser=r.rasteriser)], r.cache)
    want = ref.composite(f, p[0], m)
    mod = types.ModuleType("detection_processor")
    mod.draw_detections = lambda *a, **k: "original"
    ov.install(mod, r)
    dev = torch.from_numpy(f).cuda()
    got = mod.draw_detections(dev, s["detections"])
    assert got.is_cuda and (got.cpu().numpy() == want).all() and (dev.cpu().numpy() == f).all()
    assert mod.draw_detections(f, s["detections"]) == "original"
    host = r.draw_detections(f, s["detections"])
    assert isinstance(host, np.ndarray) and (host == want).all()
    r.close()
