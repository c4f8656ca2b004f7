"""The host side of the face masks, without a GPU: the restatement (tests/face_ref.py) against values worked by hand, the blur taps
against tests/motion_ref.py and against the library's own rule, the padded rectangle, the adaptive kernel size, the layer plan
(rtd_debug_facemask_plan), every limit that needs no device, and the Python classes of telescope_cam_detection_amd/face_masker.py."""
import logging

import numpy as np
import pytest

from tests import face_ref as ref
from tests import motion_ref
from telescope_cam_detection_amd import _capi
from telescope_cam_detection_amd import face_masker as fm


def frame_of(plane, other=7):
    """an [H, W, 3] frame: `plane` in channels 0 and 1, a constant in channel 2"""
    p = np.array(plane, np.uint8)
    return np.ascontiguousarray(np.stack([p, p, np.full_like(p, other)], axis=2))


# ---- the restatement against hand-worked values ---------------------------------------------------------------------------------------
def test_blur_3x3_region_k3_by_hand():
    """taps 64 128 64; REFLECT_101 makes the edge sums 128 a + 128 b.  Row sums of the ramp (in 1/256): [3840 5120 6400], [11520 12800
    14080], [19200 20480 21760]; the column pass on them gives exact multiples of 65536, e.g. 128 (3840 + 11520) = 30 * 65536."""
    ramp = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]])
    assert (ref.blur_region(frame_of(ramp), 3)[:, :, 0] == [[30, 35, 40], [45, 50, 55], [60, 65, 70]]).all()
    spike = np.array([[0, 0, 0], [0, 255, 0], [0, 0, 0]])
    # the spike's row sums are 32640 in every column of row 1; every output is 128 * 32640 = 63.75 * 65536 -> 64
    out = ref.blur_region(frame_of(spike), 3)
    assert (out[:, :, 0] == 64).all() and (out[:, :, 2] == 7).all()


def test_blur_of_a_region_one_pixel_wide_by_hand():
    """n = 1 reflects every column onto column 0: the row sum is 256 v.  Columns [10 20 40]: (128 * 2560 + 128 * 5120) / 65536 = 15,
    (64 * 2560 + 128 * 5120 + 64 * 10240 + 32768) >> 16 = 23 (22.5 rounds up), 128 (5120 + 10240) / 65536 = 30."""
    out = ref.blur_region(frame_of([[10], [20], [40]]), 3)
    assert out[:, 0, 0].tolist() == [15, 23, 30]
    wide = ref.blur_region(frame_of([[10, 20, 40]]), 3)           # and the same along a row
    assert wide[0, :, 0].tolist() == [15, 23, 30]


def test_blur_k1_is_the_identity_and_k99_of_a_constant_is_the_constant():
    a = ref.noise(1, 9, 11)
    assert (ref.blur_region(a, 1) == a).all()
    c = np.full((5, 5, 3), 201, np.uint8)
    for k in (3, 25, 63, 65, 99):                                 # a region shorter than the radius reflects repeatedly
        assert (ref.blur_region(c, k) == 201).all()


def test_black_box_fills_both_corners_away_from_and_at_the_frame_border():
    f = np.full((10, 10, 3), 255, np.uint8)
    out = ref.apply_mask(f, [(2, 2, 3, 3)], "black_box")          # p = int(0.6) = 0: (2, 2) .. (5, 5) inclusive
    want = np.full((10, 10), 255)
    want[2:6, 2:6] = 0
    assert (out[:, :, 0] == want).all() and (out[:, :, 2] == want).all()
    out = ref.apply_mask(f, [(7, 7, 3, 3)], "black_box")          # x2 = y2 = 10 = W: the frame ends at 9
    want = np.full((10, 10), 255)
    want[7:10, 7:10] = 0
    assert (out[:, :, 1] == want).all()
    assert (f == 255).all()                                       # apply_mask works on a copy


def test_pixelate_4x4_by_the_area_rule_by_hand():
    """blocks 2: small is 2 x 2 and both scales are exactly 2: (a + b + c + d + 2) >> 2; the nearest pass repeats each 2 x 2"""
    plane = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 17]]
    assert ref.is_area2(4, 4, 2, 2)
    out = ref.apply_mask(frame_of(plane), [(0, 0, 4, 4)], "pixelate", pixelate_blocks=2)
    assert (out[:, :, 0] == [[4, 4, 6, 6], [4, 4, 6, 6], [12, 12, 14, 14], [12, 12, 14, 14]]).all()       # 16>>2 24>>2 48>>2 57>>2


def test_pixelate_6x3_by_the_linear_rule_by_hand():
    """blocks 3: small is 2 x 1, scale 3 both ways (not the area rule).  Source positions (dx + 0.5) 3 - 0.5 = 1 and 4, (0.5) 3 - 0.5 = 1,
    all with fraction 0: weights (2048, 0), so small = [v[1][1], v[1][4]] exactly ((2048 * (2048 v >> 4) >> 16) + 2) >> 2 = v; the
    nearest map is floor(x / 3)."""
    plane = np.arange(18).reshape(3, 6) * 13 + 1
    assert not ref.is_area2(6, 3, 2, 1)
    assert ref.linear_table(6, 2, True) == [(1, 2, 2048, 0), (4, 5, 2048, 0)] and ref.linear_table(3, 1, False) == [(1, 2, 2048, 0)]
    out = ref.apply_mask(frame_of(plane), [(0, 0, 6, 3)], "pixelate", pixelate_blocks=3)
    assert (out[:, :, 0] == [[plane[1, 1]] * 3 + [plane[1, 4]] * 3] * 3).all()


def test_pixelate_with_fractional_weights_by_hand_along_a_row_and_along_a_column():
    """5 -> 2 samples: positions 0.75 and 3.25: (i0, i1, w0, w1) = (0, 1, 512, 1536), (3, 4, 1536, 512).  Row [10 20 . 40 80] of a 3-row
    region (3 -> 1: row 1, fraction 0): S = 10 * 512 + 20 * 1536 = 35840, ((2048 * 2240) >> 16) = 70, (70 + 2) >> 2 = 18; S = 40 * 1536 +
    80 * 512 = 102400 -> 200 -> 50.  Nearest 2 -> 5: floor(0.4 x) = 0 0 0 1 1.  The same numbers down a column go through the vertical
    weights: ((512 * 1280) >> 16) + ((1536 * 2560) >> 16) + 2 = 72 -> 18 and 120 + 80 + 2 = 202 -> 50."""
    assert ref.linear_table(5, 2, True) == [(0, 1, 512, 1536), (3, 4, 1536, 512)] and ref.nearest_table(2, 5).tolist() == [0, 0, 0, 1, 1]
    plane = np.zeros((3, 5), int)
    plane[1] = [10, 20, 99, 40, 80]
    out = ref.pixelate_region(frame_of(plane), 2)
    assert (out[:, :, 0] == [[18, 18, 18, 50, 50]] * 3).all()
    out = ref.pixelate_region(frame_of(plane.T), 2)
    assert (out[:, :, 0] == np.array([[18, 18, 18, 50, 50]] * 3).T).all()


def test_pixelate_with_a_small_of_one_pixel():
    """blocks larger than the region: small is 1 x 1, the sample at position 1 of 3 with fraction 0: the centre pixel everywhere"""
    plane = np.arange(9).reshape(3, 3) * 20 + 3
    out = ref.apply_mask(frame_of(plane), [(0, 0, 3, 3)], "pixelate", pixelate_blocks=10)
    assert (out[:, :, 0] == plane[1, 1]).all() and (out[:, :, 2] == 7).all()
    same = ref.pixelate_region(ref.noise(3, 7, 9), 1)             # blocks 1: both resizes are copies
    assert (same == ref.noise(3, 7, 9)).all()


# ---- taps -------------------------------------------------------------------------------------------------------------------------------
def test_taps_equal_motion_refs_up_to_63_and_the_librarys_rule_for_every_odd_k():
    worst = 1.0
    for k in range(1, 100, 2):
        margins = []
        c = ref.taps(k, margins)
        if k <= motion_ref.MAX_BLUR:
            assert (c == motion_ref.taps(k)).all(), k
        assert len(c) == k and (c >= 0).all() and c.sum() == 256 and (c == c[::-1]).all(), k
        assert fm.taps(k) == c.tolist(), k                        # gauss_taps.h through rtd_debug_facemask_plan
        worst = min([worst] + margins)
    # C++ and Python agree as long as no rounding is nearer to a tie than their exp() and sums can differ (a few ulp of 256: 1e-13)
    print(f"nearest rounding to a tie over all odd k <= 99: {worst:.3e}")
    assert worst >= 3.8e-4                                        # (the figure checked when the 99-tap table was introduced)
    for k in (0, 2, 101, -3):
        with pytest.raises(ValueError):
            ref.taps(k)
        with pytest.raises(_capi.RtdError):
            fm.taps(k)


# ---- the padded rectangle and the adaptive kernel size ----------------------------------------------------------------------------------
def test_padding_and_clamping_at_all_four_edges():
    H, W = 48, 64
    assert ref.padded_rect((10, 12, 20, 30), H, W) == (6, 8, 34, 46)                # p = int(20 * 0.2) = 4
    assert ref.padded_rect((2, 20, 20, 10), H, W)[0] == 0 and ref.padded_rect((20, 1, 20, 10), H, W)[1] == 0
    assert ref.padded_rect((50, 20, 20, 10), H, W)[2] == W and ref.padded_rect((20, 30, 20, 30), H, W)[3] == H
    assert ref.padded_rect((0, 0, 64, 48), H, W) == (0, 0, 64, 48)
    assert ref.padded_rect((5, 5, 4, 4), H, W) == (5, 5, 9, 9)                      # int(0.8) = 0
    assert ref.padded_rect((5, 5, 14, 4), H, W) == (3, 3, 21, 11)                   # int(14 * 0.2) = int(2.8000000000000003) = 2
    for face in ((-100, 0, 20, 20), (70, 0, 20, 20), (0, 60, 20, 20), (0, -40, 20, 10), (3, 3, 0, 5)):
        assert ref.is_empty(ref.padded_rect(face, H, W)), face
    faces = [(10, 12, 20, 30), (2, 1, 20, 30), (50, 30, 20, 30), (-100, 0, 20, 20), (5, 5, 14, 4), (70, 0, 20, 20)]
    got = fm.plan([(H, W)], [(0, *f, fm.BLUR, 3) for f in faces])
    assert got["rects"][:3] == [ref.padded_rect(f, H, W) for f in faces[:3]] and got["rects"][4] == (3, 3, 21, 11)
    assert got["layer_of"][3] == -1 and got["layer_of"][5] == -1 and got["layer_of"][0] >= 0


def test_adaptive_k_grows_with_the_face_and_is_capped_at_99():
    H, W = 1080, 1920
    assert ref.adaptive_k(25, (0, 0, 120, 120), H, W) == 27 == fm.adaptive_k(25, 120, 120, H, W)      # int(25 * 1.0694...) = 26 -> 27
    assert ref.adaptive_k(25, (0, 0, 10, 10), H, W) == 25
    assert ref.adaptive_k(25, (0, 0, 800, 800), H, W) == 99 == fm.adaptive_k(25, 800, 800, H, W)      # int(25 * 4.08...) = 102 -> 103 -> 99
    assert ref.adaptive_k(25, (0, 0, 700, 710), H, W) == 85                                           # int(84.92...) = 84 -> 85
    assert ref.adaptive_k(3, (0, 0, 5, 7), 5, 7) == 33                                                # the face is the frame: 3 * 11


# ---- the layer plan ---------------------------------------------------------------------------------------------------------------------
def rows(frame, faces, style=fm.BLUR, k=25):
    return [(frame, *f, style, k) for f in faces]


def test_layers_keep_the_order_of_overlapping_faces_only():
    A, B, C = (10, 10, 30, 30), (30, 30, 30, 30), (150, 10, 20, 20)
    got = fm.plan([(100, 200)], rows(0, [A, B, C]))
    assert got["layers"] == 2 and got["layer_of"] == [0, 1, 0] == ref.layers([A, B, C], ["gaussian_blur"] * 3, 100, 200)
    chain = [(10, 10, 30, 30), (40, 10, 30, 30), (70, 10, 30, 30)]                # each meets only its neighbour
    got = fm.plan([(100, 200)], rows(0, chain))
    assert got["layers"] == 3 and got["layer_of"] == [0, 1, 2] == ref.layers(chain, ["gaussian_blur"] * 3, 100, 200)
    # the same three faces on three frames never wait on each other, and a face of frame 1 ignores an overlapping one of frame 0
    got = fm.plan([(100, 200)] * 3, [(i, *f, fm.BLUR, 25) for i, f in enumerate(chain)] + rows(1, [chain[0]]))
    assert got["layers"] == 2 and got["layer_of"] == [0, 0, 0, 1]
    # a black box reaches one row and column further than a blur of the same face: only it meets the neighbour that starts there
    a, b = (10, 10, 4, 4), (14, 10, 4, 4)                                           # p = 0: a is 10..14, b starts at 14
    assert fm.plan([(50, 50)], rows(0, [a, b]))["layers"] == 1
    assert fm.plan([(50, 50)], [(0, *a, fm.BLACK_BOX, 0), (0, *b, fm.BLUR, 3)])["layer_of"] == [0, 1]
    assert ref.layers([a, b], ["black_box", "gaussian_blur"], 50, 50) == [0, 1]


def test_tiles_of_a_call():
    got = fm.plan([(100, 200), (37, 223)], [(0, 0, 0, 200, 100, fm.BLUR, 3), (1, 0, 0, 223, 37, fm.PIXELATE, 10), (1, 0, 0, 10, 10, fm.BLACK_BOX, 0)])
    th, tw = got["tile"]
    assert (th, tw) == (16, 64)
    assert got["tiles"]["blur_rows"] == got["tiles"]["blur_cols"] == 4 * 7 and got["tiles"]["pix_nearest"] == 4 * 3
    assert got["tiles"]["pix_small"] == 1 and got["tiles"]["box"] == 1              # small is 22 x 3 x 3 bytes; the box 13 x 13
    assert got["layers"] == 2


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
GOOD = [(0, 10, 10, 20, 20, fm.BLUR, 25), (1, 0, 0, 3, 3, fm.PIXELATE, 2)]
BAD = {
    "frame index": (lambda s, f: f.__setitem__(1, (2,) + f[1][1:]), "face 1"),
    "negative frame index": (lambda s, f: f.__setitem__(0, (-1,) + f[0][1:]), "face 0"),
    "style": (lambda s, f: f.__setitem__(1, f[1][:5] + (3, 2)), "face 1"),
    "even k": (lambda s, f: f.__setitem__(0, f[0][:6] + (24,)), "face 0"),
    "k 101": (lambda s, f: f.__setitem__(0, f[0][:6] + (101,)), "face 0"),
    "k 0": (lambda s, f: f.__setitem__(0, f[0][:6] + (0,)), "face 0"),
    "blocks 0": (lambda s, f: f.__setitem__(1, f[1][:6] + (0,)), "face 1"),
    "side 0": (lambda s, f: s.__setitem__(1, (0, 7)), "frame 1"),
    "side 65536": (lambda s, f: s.__setitem__(0, (48, 65536)), "frame 0"),
    "2 GiB": (lambda s, f: s.__setitem__(0, (65535, 65535)), "frame 0"),
    "no frame": (lambda s, f: s.clear(), "frames per call"),
    "65 frames": (lambda s, f: s.extend([(4, 4)] * 63), "frames per call"),
    "1025 faces": (lambda s, f: f.extend([GOOD[0]] * 1023), "faces per call"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_a_limit_is_refused_as_invalid_and_names_the_face_or_frame(what):
    shapes, faces = [(48, 64), (5, 7)], list(GOOD)
    fm.plan(shapes, faces)                                        # the good call passes
    edit, names = BAD[what]
    edit(shapes, faces)
    with pytest.raises(_capi.RtdError) as ei:
        fm.plan(shapes, faces)
    assert ei.value.code == _capi.RTD_E_INVALID and names in str(ei.value), str(ei.value)


def test_null_pointers_and_the_limits_themselves_pass_or_fail_as_documented():
    L = _capi.lib()
    hw = (_capi.C.c_int32 * 2)(48, 64)
    one = (_capi.RtdFaceRect * 1)(_capi.RtdFaceRect(0, 1, 1, 5, 5, fm.BLUR, 99, 0))
    args = (None,) * 6 + (0, None)
    assert L.rtd_debug_facemask_plan(1, None, 1, one, *args) == _capi.RTD_E_INVALID
    assert L.rtd_debug_facemask_plan(1, hw, 1, None, *args) == _capi.RTD_E_INVALID
    assert b"null argument" in L.rtd_facemask_last_error(None)
    assert L.rtd_debug_facemask_plan(1, hw, 1, one, *args) == _capi.RTD_OK          # k = 99, and every output pointer may be null
    assert L.rtd_debug_facemask_plan(1, hw, 0, None, *args) == _capi.RTD_OK
    assert L.rtd_facemask_apply(None, 1, None, hw, 1, 1, one) == _capi.RTD_E_INVALID  # no handle
    L.rtd_facemask_destroy(None)
    fm.plan([(4, 4)] * 64, [(63, 0, 0, 2, 2, fm.PIXELATE, 10 ** 6)] * 1024)         # 64 frames, 1024 faces, any blocks >= 1
    assert _capi.C.sizeof(_capi.RtdFaceRect) == 32


# ---- the classes ------------------------------------------------------------------------------------------------------------------------
def no_faces(gray):
    return []


def test_constructor_parity(caplog):
    m = fm.FaceMasker(detector=no_faces)
    assert (m.detection_backend, m.mask_style, m.min_face_size, m.blur_strength, m.pixelate_blocks, m.scale_factor, m.min_neighbors) == \
        ("opencv_haar", "gaussian_blur", 30, 25, 10, 1.1, 5)
    assert fm.FaceMasker.FACE_PADDING_PERCENT == 0.2
    with caplog.at_level(logging.WARNING):
        assert fm.FaceMasker(blur_strength=24, detector=no_faces).blur_strength == 25
    assert "odd" in caplog.text
    assert fm.FaceMasker(blur_strength=31, detector=no_faces).blur_strength == 31
    for bad in (0, -3):
        with pytest.raises(ValueError, match="blur_strength must be positive"):
            fm.FaceMasker(blur_strength=bad, detector=no_faces)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert fm.FaceMasker("yolox", detector=no_faces).detection_backend == "opencv_haar"
        assert fm.FaceMasker("retina", detector=no_faces).detection_backend == "opencv_haar"
    assert "yolox" in caplog.text and "retina" in caplog.text
    try:
        import mediapipe  # noqa: F401
    except ImportError:
        assert fm.FaceMasker("mediapipe", detector=no_faces).detection_backend == "opencv_haar"      # the reference's fallback
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="detector"):
            fm.FaceMasker()


def test_styles_become_library_rows_and_an_unknown_style_is_a_gaussian_blur(caplog):
    m = fm.FaceMasker(blur_strength=25, pixelate_blocks=7, detector=no_faces)
    face = (5, 6, 120, 120)
    assert m._face_rows(2, (1080, 1920, 3), [face], "gaussian_blur") == [(2, 5, 6, 120, 120, fm.BLUR, 25)]
    assert m._face_rows(0, (1080, 1920, 3), [face], "adaptive_blur") == [(0, 5, 6, 120, 120, fm.BLUR, 27)]
    assert m._face_rows(0, (1080, 1920, 3), [face], "pixelate") == [(0, 5, 6, 120, 120, fm.PIXELATE, 7)]
    assert m._face_rows(0, (1080, 1920, 3), [face], "black_box") == [(0, 5, 6, 120, 120, fm.BLACK_BOX, 0)]
    with caplog.at_level(logging.WARNING):
        assert m._face_rows(0, (1080, 1920, 3), [face], "mosaic") == [(0, 5, 6, 120, 120, fm.BLUR, 25)]
    assert "mosaic" in caplog.text


def test_apply_mask_without_faces_is_the_frame_itself_and_bad_frames_raise():
    m = fm.FaceMasker(detector=no_faces)
    f = np.zeros((4, 5, 3), np.uint8)
    assert m.apply_mask(f, []) is f and m.apply_mask_batch([f, f], [[], []]) == [f, f]
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 1), np.uint8), np.zeros((4, 5, 3), np.float32), np.zeros((4, 10, 3), np.uint8)[:, ::2],
                [[0, 0, 0]]):
        with pytest.raises(ValueError):
            m.apply_mask(bad, [(0, 0, 2, 2)])
        with pytest.raises(ValueError):
            m.detect_faces(bad)
    with pytest.raises(ValueError):
        m.apply_mask_batch([f], [[], []])


def test_detect_faces_on_a_host_frame_hands_the_detector_cv2s_gray_plane():
    seen = {}

    def detector(gray):
        seen["gray"] = gray
        return np.array([[1, 2, 3, 4]])

    f = np.array(ref.noise(5, 6, 7))
    m = fm.FaceMasker(detector=detector)
    assert m.detect_faces(f) == [(1, 2, 3, 4)] and all(type(v) is int for v in m.detect_faces(f)[0])
    assert (seen["gray"] == motion_ref.as_gray(f)).all() and (fm.gray_plane(f) == motion_ref.as_gray(f)).all()


def test_face_masking_cache_call_by_call():
    c = fm.FaceMaskingCache(ttl_frames=2)
    assert c.ttl == 2 and c.cache == {} and c.should_detect("a") and c.get_cached_faces("a") is None
    c.increment_frame_count("a")                                  # unknown camera: nothing happens
    assert c.cache == {}
    faces = [(1, 2, 3, 4)]
    c.update_cache("a", faces)
    assert c.cache["a"] == (faces, 0) and not c.should_detect("a") and c.get_cached_faces("a") is faces and c.should_detect("b")
    c.increment_frame_count("a")
    assert not c.should_detect("a")
    c.increment_frame_count("a")
    assert c.cache["a"][1] == 2 and c.should_detect("a")
    c.update_cache("a", [])
    assert c.get_cached_faces("a") == [] and not c.should_detect("a")
    c.update_cache("b", faces)
    c.clear_cache("a")
    assert "a" not in c.cache and "b" in c.cache
    c.clear_cache("zz")
    c.clear_cache()
    assert c.cache == {} and fm.FaceMaskingCache().ttl == 5


class FakeMasker:
    def __init__(self, faces, raises=False):
        self.faces, self.raises, self.detected, self.masked = faces, raises, 0, []

    def detect_faces(self, frame):
        self.detected += 1
        if self.raises:
            raise RuntimeError("the detector broke")
        return self.faces

    def apply_mask(self, frame, faces):
        self.masked.append(list(faces))
        return ("masked", frame)


def test_mask_frame_takes_the_references_three_branches():
    frame = object()
    # 1. the cache says detect: detect, store, mask
    m, c = FakeMasker([(1, 1, 2, 2)]), fm.FaceMaskingCache(2)
    assert fm.mask_frame(m, c, frame, "a") == ("masked", frame) and m.detected == 1 and c.cache["a"] == ([(1, 1, 2, 2)], 0)
    # 2. cached faces: no detection, the frame is counted
    assert fm.mask_frame(m, c, frame, "a") == ("masked", frame) and m.detected == 1 and c.cache["a"][1] == 1
    assert fm.mask_frame(m, c, frame, "a") == ("masked", frame) and m.detected == 1 and c.cache["a"][1] == 2
    assert fm.mask_frame(m, c, frame, "a") == ("masked", frame) and m.detected == 2 and c.cache["a"][1] == 0      # the ttl ran out
    # 3. no cache: detect every frame
    assert fm.mask_frame(m, None, frame, "a") == ("masked", frame) and fm.mask_frame(m, None, frame, "a")[0] == "masked" and m.detected == 4
    # no faces: the frame itself, detected or cached
    e, c = FakeMasker([]), fm.FaceMaskingCache(2)
    assert fm.mask_frame(e, c, frame, "a") is frame and fm.mask_frame(e, c, frame, "a") is frame and e.detected == 1 and e.masked == []
    assert fm.mask_frame(e, None, frame, "a") is frame and fm.mask_frame(None, c, frame, "a") is frame


def test_mask_frame_returns_the_unmasked_frame_on_any_exception(caplog):
    frame = object()
    with caplog.at_level(logging.ERROR):
        assert fm.mask_frame(FakeMasker([], raises=True), fm.FaceMaskingCache(), frame, "cam7") is frame
    assert "cam7" in caplog.text and "the detector broke" in caplog.text

    class BadMask(FakeMasker):
        def apply_mask(self, frame, faces):
            raise ValueError("no")
    assert fm.mask_frame(BadMask([(0, 0, 1, 1)]), None, frame, "a") is frame


def test_install_keeps_host_frames_on_the_original_method():
    class Server:
        def __init__(self):
            self.face_masker, self.face_masking_cache, self.enabled = FakeMasker([(0, 0, 1, 1)]), fm.FaceMaskingCache(), True

        def _is_face_masking_enabled_for_camera(self, camera_id):
            return self.enabled

        def _apply_face_masking_to_frame(self, frame, camera_id):
            return ("original", frame)

    s = Server()
    fm.install(s)
    fm.install(Server)                                            # twice, and on the class: the original stays the original
    f = np.zeros((2, 2, 3), np.uint8)
    assert s._apply_face_masking_to_frame(f, "a") == ("original", f)


def test_all_four_styles_equal_cv2_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    H, W = 160, 224
    a = np.array(ref.noise(1200, H, W))
    faces = [(30, 20, 60, 50), (70, 50, 50, 40), (180, 120, 60, 60), (-5, -5, 30, 30), (200, 140, 40, 40)]
    for style in ref.STYLES:
        for k, blocks in ((25, 10), (9, 3), (99, 2), (3, 7)):
            want = a.copy()
            for (x, y, w, h) in faces:                          # src/face_masker.py's calls on the padded rectangle
                x1, y1, x2, y2 = ref.padded_rect((x, y, w, h), H, W)
                if style == "black_box":
                    cv2.rectangle(want, (x1, y1), (x2, y2), (0, 0, 0), -1)
                elif style == "pixelate":
                    small = cv2.resize(want[y1:y2, x1:x2], (max(1, (x2 - x1) // blocks), max(1, (y2 - y1) // blocks)), interpolation=cv2.INTER_LINEAR)
                    want[y1:y2, x1:x2] = cv2.resize(small, (x2 - x1, y2 - y1), interpolation=cv2.INTER_NEAREST)
                else:
                    kk = k if style == "gaussian_blur" else ref.adaptive_k(k, (x, y, w, h), H, W)
                    want[y1:y2, x1:x2] = cv2.GaussianBlur(want[y1:y2, x1:x2], (kk, kk), 0)
            assert (ref.apply_mask(a, faces, style, k, blocks) == want).all(), (style, k, blocks)
