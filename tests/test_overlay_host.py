"""The overlay feature without a GPU: the plans against the calls the reference makes (tests/golden/overlay_calls.json), the pixel rules
of the numpy compositor (tests/overlay_ref.py), OverlayRenderer over RefBackend, the host mask LRU and the rasterisers."""
import numpy as np
import pytest

from tests import overlay_ref as ref
from tests.overlay_ref import FILL, MASK, OUTLINE, prim, prims
from telescope_cam_detection_amd import overlay as ov

GOLD = ref.load_golden()
SCENARIOS = {s["name"]: s for s in GOLD["scenarios"]}


def plan_of(s, rasteriser):
    if s["kind"] == "web":
        return ov.plan_web(s["result"], rasteriser)
    return ov.plan_snapshot(s["detections"], s["thickness"], s["font_scale"], s["draw_labels"], rasteriser=rasteriser)


def test_fixture_declares_the_metric_rule_the_fake_rasteriser_uses():
    assert GOLD["metric"] == ref.METRIC
    assert len(SCENARIOS) == len(GOLD["scenarios"]) >= 15


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_plans_equal_the_recorded_cv2_calls(name):
    s = SCENARIOS[name]
    got = ref.as_events(plan_of(s, ref.FakeRasteriser(GOLD["metric"])))
    want = s["calls"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i, g, w)
    assert len(got) == len(want)


def test_fixture_covers_what_it_claims():
    calls = [c for s in GOLD["scenarios"] for c in s["calls"]]
    rects = [c for c in calls if c[0] == "rect"]
    texts = [c for c in calls if c[0] == "text"]
    assert any(c[1][1] < 0 for c in rects) and any(c[1][0] < 0 for c in rects)               # negative bar / box coordinates
    assert any(c[1][0] > c[2][0] for c in rects)                                               # inverted corners
    colours = {tuple(c[3]) for c in rects}
    assert set(ov.CLASS_COLORS.values()) | {ov.DEFAULT_COLOR, ov.WEB_PERSON, ov.WEB_ANIMAL, ov.WEB_OTHER} <= colours
    assert {c[6] for c in texts} == {True, False} and {c[4] for c in rects} >= {-1, 1, 2, 3}
    labels = {c[1] for c in texts}
    assert {"Northern Cardinal 0.93", "Corvus (genus) 0.61", "Bobcat 0.50", "Canidae 0.40", "dog 0.45", "Latency: 0ms", "Latency: 13ms"} <= labels
    top = SCENARIOS["snap_top_edge"]
    above = [c[2][1] < int(d["bbox"]["y1"]) for c, d in zip([c for c in top["calls"] if c[0] == "text"], top["detections"])]
    assert True in above and False in above                                                    # both label_y branches
    assert not [c for c in SCENARIOS["snap_no_labels"]["calls"] if c[0] == "text"]
    assert SCENARIOS["snap_empty"]["calls"] == [] and len(SCENARIOS["web_empty"]["calls"]) == 1


# ---- the compositor's pixel rules ------------------------------------------------------------------------------------------------------
def blank(h=40, w=50, c=3, v=7):
    return np.full((h, w, c), v, np.uint8)


def test_fill_is_inclusive_and_takes_corners_in_any_order():
    want = blank()
    want[5:11, 8:21] = (1, 2, 3)
    for corners in ((8, 5, 20, 10), (20, 10, 8, 5), (8, 10, 20, 5)):
        got = ref.composite(blank(), prims(prim(FILL, *corners, (1, 2, 3))), np.zeros(0, np.uint8))
        assert (got == want).all(), corners


@pytest.mark.parametrize("t", [1, 2, 3, 7])
def test_outline_strip_is_t_pixels_wide_with_square_corners(t):
    got = ref.composite(blank(60, 70), prims(prim(OUTLINE, 20, 15, 50, 40, (9, 9, 9), t)), np.zeros(0, np.uint8))[:, :, 0] == 9
    o, i = t // 2, (t - 1) // 2
    assert o + i + 1 == t
    want = np.zeros((60, 70), bool)
    want[15 - o:40 + o + 1, 20 - o:50 + o + 1] = True
    want[15 + i + 1:40 - i, 20 + i + 1:50 - i] = False
    assert (got == want).all()
    assert got[27].sum() == 2 * t and got[:, 35].sum() == 2 * t          # a row / a column through the middle crosses two strips
    assert got[15 - o, 20 - o] and got[40 + o, 50 + o]                     # square corners
    if t == 1:                                                             # cv2's outline: the four edges
        assert got.sum() == 2 * 31 + 2 * 26 - 4


def test_thick_outline_of_a_small_box_has_no_hole():
    got = ref.composite(blank(), prims(prim(OUTLINE, 10, 10, 13, 12, (9, 9, 9), 7)), np.zeros(0, np.uint8))[:, :, 0] == 9
    want = np.zeros((40, 50), bool)
    want[7:16, 7:17] = True
    assert (got == want).all()


def test_blend_endpoints_and_rounding():
    m = np.array([[0, 255, 128, 1, 254]], np.uint8)
    bg = blank(1, 5, 3, 100)
    got = ref.composite(bg, prims(prim(MASK, 0, 0, 5, 1, (200, 0, 100))), m.reshape(-1))
    assert got[0, 0].tolist() == [100, 100, 100] and got[0, 1].tolist() == [200, 0, 100]
    for x, a in enumerate(m[0].tolist()):
        assert got[0, x].tolist() == [(100 * (255 - a) + c * a + 127) // 255 for c in (200, 0, 100)]


def test_order_matters_and_later_primitives_win():
    a, b = prim(FILL, 0, 0, 20, 20, (1, 1, 1)), prim(FILL, 10, 10, 30, 30, (2, 2, 2))
    ab = ref.composite(blank(), prims(a, b), np.zeros(0, np.uint8))
    ba = ref.composite(blank(), prims(b, a), np.zeros(0, np.uint8))
    assert ab[15, 15, 0] == 2 and ba[15, 15, 0] == 1 and ab[5, 5, 0] == 1 and ab[25, 25, 0] == 2


def test_clipping_on_every_side_and_wholly_outside():
    m = np.full(6 * 4, 255, np.uint8)
    got = ref.composite(blank(), prims(prim(FILL, -5, -5, 2, 2, (1, 1, 1)), prim(FILL, 45, 35, 90, 90, (2, 2, 2)), prim(OUTLINE, -3, 10, 60, 20, (3, 3, 3), 3),
                                       prim(MASK, 48, 38, 6, 4, (4, 4, 4)), prim(MASK, -4, 30, 6, 4, (5, 5, 5)), prim(FILL, 50, 0, 60, 10, (6, 6, 6)),
                                       prim(FILL, 0, -9, 10, -1, (6, 6, 6)), prim(MASK, 0, 40, 6, 4, (6, 6, 6))), m)[:, :, 0]
    assert (got[:3, :3] == 1).all() and got[3, 3] == 7 and (got[35:, 45:48] == 2).all()
    assert (got[9:12, :] == 3).all() and (got[19:22, :] == 3).all() and (got[12:19, :] == 7).all()
    assert (got[38:, 48:] == 4).all() and (got[30:34, :2] == 5).all() and got[30, 2] == 7
    assert not (got == 6).any()


def test_one_channel_frames_take_the_first_colour_value():
    got = ref.composite(blank(10, 10, 1), prims(prim(FILL, 1, 1, 3, 3, (50, 60, 70)), prim(MASK, 5, 5, 1, 1, (200, 1, 2))), np.array([255], np.uint8))
    assert got.shape == (10, 10, 1) and got[2, 2, 0] == 50 and got[5, 5, 0] == 200
    assert ref.composite(np.full((4, 4), 3, np.uint8), prims(), np.zeros(0, np.uint8)).shape == (4, 4, 1)


def test_tiles_touched_counts_an_outline_as_its_strips():
    tile = (16, 64)
    assert ref.tiles_touched(prims(), (100, 300, 3), tile) == 0
    assert ref.tiles_touched(prims(prim(FILL, 0, 0, 299, 99)), (100, 300, 3), tile) == 7 * 5
    assert ref.tiles_touched(prims(prim(OUTLINE, 0, 0, 299, 99, thickness=1)), (100, 300, 3), tile) == 7 * 5 - 5 * 3
    assert ref.tiles_touched(prims(prim(OUTLINE, 70, 20, 120, 40, thickness=1)), (100, 300, 3), tile) == 2
    assert ref.tiles_touched(prims(prim(FILL, 400, 0, 500, 10), prim(MASK, -10, -10, 5, 5)), (100, 300, 3), tile) == 0
    assert ref.tiles_touched(prims(prim(MASK, 60, 14, 8, 4)), (100, 300, 3), tile) == 4


# ---- the renderer over the restatement --------------------------------------------------------------------------------------------------
def renderer():
    return ov.OverlayRenderer(device=0, rasteriser=ref.FakeRasteriser(), backend=ref.RefBackend())


def test_renderer_leaves_a_host_frame_unchanged_with_and_without_inplace():
    r = renderer()
    s = SCENARIOS["web_top_edge"]
    frame = blank(*s["hw"])
    keep = frame.copy()
    plan = ov.plan_web(s["result"], r.rasteriser)
    out = r.draw_batch([frame], [plan])[0]
    assert (frame == keep).all() and out is not frame and (out != keep).any()
    p, m = ov.lower([plan], ov.MaskCache(ref.FakeRasteriser()))
    assert (out == ref.composite(keep, p[0], m)).all()
    assert r._backend.calls == [(1, False, False)]
    assert (r.draw_batch([frame], [plan], inplace=True)[0] == out).all() and (frame == keep).all()   # host frames are never drawn on
    assert (r.web_draw(frame, s["result"]) == out).all()


def test_ref_backend_draws_in_place_when_asked():
    frame = blank()
    out = ref.RefBackend().draw([frame], False, [prims(prim(FILL, 0, 0, 3, 3, (1, 1, 1)))], np.zeros(0, np.uint8), True)[0]
    assert out is frame and frame[0, 0, 0] == 1


def test_draw_detections_has_the_reference_call_shape():
    r = renderer()
    s = SCENARIOS["snap_species"]
    frame = blank(*s["hw"])
    out = r.draw_detections(frame, s["detections"])
    assert isinstance(out, np.ndarray) and out.shape == frame.shape and (frame == 7).all()
    p, m = ov.lower([ov.plan_snapshot(s["detections"], 3, 0.7, True, rasteriser=r.rasteriser)], r.cache)
    assert (out == ref.composite(frame, p[0], m)).all()
    gray = np.full((480, 640), 9, np.uint8)
    assert r.draw_detections(gray, s["detections"], thickness=1, draw_labels=False).shape == (480, 640)
    assert (r.draw_detections(frame, []) == frame).all()


def test_install_rebinds_the_modules_draw_detections_for_device_frames_only():
    import types
    mod = types.ModuleType("detection_processor")
    seen = []
    mod.draw_detections = lambda frame, dets, *a, **k: seen.append(len(dets)) or "original"
    r = renderer()
    ov.install(mod, r)
    ov.install(mod, r)                                                      # twice: the original is still the first one
    assert mod.draw_detections(blank(), [1, 2]) == "original" and seen == [2]

    class DeviceFrame:                                                      # what install looks at
        is_cuda = True
    calls = []
    r.draw_detections = lambda *a: calls.append(a) or "device"
    assert mod.draw_detections(DeviceFrame(), [], 2, 0.5, False) == "device" and calls[0][1:] == ([], 2, 0.5, False)


def test_mjpeg_tick_is_one_overlay_call_and_one_encode_call():
    from tests.jpeg_ref import RefBackend as JpegRef, encode
    from telescope_cam_detection_amd.jpeg import JpegEncoder
    jb = JpegRef()
    r = ov.OverlayRenderer(device=0, rasteriser=ref.FakeRasteriser(), backend=ref.RefBackend(), encoder=JpegEncoder(0, backend=jb))
    frames = [blank(48, 64), blank(40, 56, 3, 90), blank(32, 32)]
    results = [SCENARIOS["web_no_latency"]["result"], None, SCENARIOS["web_empty"]["result"]]
    got = r.mjpeg_tick(frames, results, 80)
    assert r._backend.calls == [(3, False, False)] and jb.calls == [(3, False, 80)]
    assert got[1] == encode(frames[1], 80)
    assert got[0] == encode(r.web_draw(frames[0], results[0]), 80) != encode(frames[0], 80)


def test_lower_stores_a_repeated_label_once_and_skips_empty_masks():
    cache = ov.MaskCache(ref.FakeRasteriser())
    plan = [("text", "ab", (5, 20), 0.5, (1, 2, 3), 2, False), ("text", "ab", (50, 20), 0.5, (1, 2, 3), 2, False), ("text", "", (0, 0), 0.5, (1, 2, 3), 2, False),
            ("rect", (3, 4), (1, 2), (9, 8, 7), -1), ("rect", (3, 4), (1, 2), (9, 8, 7), 3)]
    p, m = ov.lower([plan, plan[:1]], cache)
    (w, h), base = ref.text_size("ab", 0.5, 2)
    assert len(m) == w * (h + base) and len(p[0]) == 4 and len(p[1]) == 1
    assert p[0]["kind"].tolist() == [MASK, MASK, FILL, OUTLINE] and p[0]["mask_offset"].tolist()[:2] == [0, 0] and p[1]["mask_offset"][0] == 0
    assert (p[0][0]["x1"], p[0][0]["y1"], p[0][0]["x2"], p[0][0]["y2"]) == (5, 20 - h, w, h + base)
    assert p[0][3]["thickness"] == 3 and p[0][2]["bgr"].tolist() == [9, 8, 7]
    with pytest.raises(ValueError):
        ov.lower([[("rect", (0, 0), (1, 1), (0, 0, 0), 0)]], cache)


def test_mask_cache_is_an_lru():
    fr = ref.FakeRasteriser()
    c = ov.MaskCache(fr, capacity=2)
    a1 = c.get("a", 0.5, 2, False)
    assert c.get("a", 0.5, 2, False)[0] is a1[0] and (c.hits, c.misses, fr.mask_calls) == (1, 1, 1)
    c.get("b", 0.5, 2, False)
    c.get("a", 0.5, 2, False)                                               # "a" is now the most recent
    c.get("c", 0.5, 2, False)                                               # evicts "b"
    assert len(c) == 2 and fr.mask_calls == 3
    c.get("a", 0.5, 2, False)
    assert fr.mask_calls == 3
    c.get("b", 0.5, 2, False)
    assert fr.mask_calls == 4
    c.get("a", 0.5, 2, True)                                                # another key: the AA flag
    assert fr.mask_calls == 5


# ---- rasterisers ------------------------------------------------------------------------------------------------------------------------
def test_pillow_rasteriser_size_and_mask_agree_and_every_printable_character_leaves_a_mark():
    r = ov.PillowRasteriser()
    for scale, t in ((0.5, 2), (0.7, 2), (1.0, 3)):
        for text in ("cat: 0.90", "Latency: 13ms", "Corvus (genus) 0.61"):
            (w, h), base = r.size(text, scale, t)
            for aa in (False, True):
                m, dx, dy = r.mask(text, scale, t, aa)
                assert m.dtype == np.uint8 and m.shape == (h + base, w) and (dx, dy) == (0, -h)
                assert m.max() == 255 and (aa or set(np.unique(m).tolist()) <= {0, 255})
        assert r.size("ab", scale, t)[0][1] == r.size("Ay", scale, t)[0][1]                   # the height belongs to the font
        assert r.size("abcd", scale, t)[0][0] > r.size("ab", scale, t)[0][0]
    for code in range(33, 127):
        m, _, _ = r.mask(chr(code), 0.7, 2, True)
        assert m.any(), chr(code)
    assert r.mask("", 0.5, 2, False)[0].size == 0 or not r.mask("", 0.5, 2, False)[0].any()


def test_cv2_rasteriser_issues_the_expected_calls_and_crops():
    cv2 = ref.RecordingCv2()
    r = ov.Cv2Rasteriser(cv2)
    (w, h), base = ref.text_size("dog 0.81", 0.7, 2)
    assert r.size("dog 0.81", 0.7, 2) == ((w, h), base)
    m, dx, dy = r.mask("dog 0.81", 0.7, 2, True)
    pad = 4
    assert cv2.calls == [["text", "dog 0.81", [pad, pad + h], 0.7, [255, 255, 255], 2, True]]
    assert all(c[1] == cv2.FONT_HERSHEY_SIMPLEX for c in cv2.size_calls)
    # the stand-in fills the text box inset by one pixel: rows oy - h + 1 .. oy - 1, columns ox + 1 .. ox + w - 2
    assert m.shape == (h - 1, w - 2) and (m == 255).all() and (dx, dy) == (1, -h + 1)
    r.mask("dog 0.81", 0.5, 1, False)
    assert cv2.calls[-1][-1] is False and cv2.calls[-1][2] == [3, 3 + ref.text_size("dog 0.81", 0.5, 1)[0][1]]
    assert r.mask("", 0.5, 1, False)[0].size == 0


def test_default_rasteriser_falls_back_to_pillow_without_cv2():
    try:
        import cv2  # noqa: F401
        assert isinstance(ov.default_rasteriser(), ov.Cv2Rasteriser)
    except ImportError:
        assert isinstance(ov.default_rasteriser(), ov.PillowRasteriser)


def test_line8_text_through_the_cv2_rasteriser_is_cv2s_own_pixels():
    cv2 = pytest.importorskip("cv2")
    r = ov.OverlayRenderer(device=0, rasteriser=ov.Cv2Rasteriser(), backend=ref.RefBackend())
    rng = np.random.default_rng(3)
    for text, org, scale, colour, t in (("cat: 0.90", (10, 40), 0.5, (255, 255, 255), 2), ("Latency: 13ms", (10, 30), 0.7, (0, 255, 0), 2),
                                        ("clipped", (-12, 8), 0.7, (10, 20, 30), 2), ("edge", (150, 118), 1.0, (1, 2, 3), 1)):
        frame = rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)
        want = frame.copy()
        cv2.putText(want, text, org, cv2.FONT_HERSHEY_SIMPLEX, scale, colour, t)
        got = r.draw_batch([frame], [[("text", text, org, scale, colour, t, False)]])[0]
        assert (got == want).all(), text
