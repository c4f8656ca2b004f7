"""The crop enhancement without a GPU: the numpy restatement (tests/enhance_ref.py) against its own scalar transcription, against the
fp64 definitions of the colour conversions, the CLAHE and bilateral properties, the packing rule of rtd_enhance_layout (host code of
the library) and the Stage-2 glue with stand-ins.  Where cv2 is importable the restatement is compared with it."""
import types

import numpy as np
import pytest

from tests import enhance_ref as ref
from telescope_cam_detection_amd import _capi, enhance
from telescope_cam_detection_amd.stage2 import BatchedStage2


@pytest.mark.parametrize("h,w,grid", [(16, 16, (8, 8)), (19, 23, (4, 4)), (16, 17, (8, 8))])       # 17 x 16 (w x h) with 8 x 8 is the last
def test_vectorised_equals_scalar_transcription(h, w, grid):
    for kind, params in (("noise", {}), ("ramp", {}), ("noise", {"clip_limit": 40.0, "bilateral_d": 3, "sigma_color": 10, "sigma_space": 10}),
                         ("ramp", {"clip_limit": 0.0})):
        img = ref.content(kind, h, w, seed=h * 100 + w)
        a = ref.stages(img, tile_grid_size=grid, **params)
        b = ref.scalar_enhance(img, tile_grid_size=grid, **params)
        for k in ("lab", "luts", "bgr", "out"):
            assert (a[k] == b[k]).all(), (kind, params, k, int((a[k] != b[k]).sum()))


@pytest.fixture(scope="module")
def lattice():
    g = np.arange(0, 256, 3)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)


def test_forward_lab_against_the_fp64_definition(lattice):
    got = ref.bgr_to_lab(lattice).astype(np.int64)
    want = np.clip(np.rint(ref.lab_fp64(lattice)), 0, 255).astype(np.int64)
    worst = np.abs(got - want).max(0)
    print("forward Lab max |diff| (L, a, b):", worst.tolist())
    assert (worst <= np.array([1, 3, 2])).all(), worst.tolist()
    assert ref.tables()["C"].sum(1).tolist() == [4096, 4096, 4096]


def test_inverse_lab_against_the_fp64_definition(lattice):
    lab = ref.bgr_to_lab(lattice)
    lab[:, 0] = np.random.default_rng(0).integers(0, 256, len(lab))
    got = ref.lab_to_bgr(lab).astype(np.int64)
    want = np.clip(np.rint(ref.bgr_fp64(lab)), 0, 255).astype(np.int64)
    d = np.abs(got - want)
    share = float((d > 1).any(1).mean())
    print("inverse Lab max |diff| (B, G, R):", d.max(0).tolist(), "share off by more than 1:", share)
    assert d.max() <= 3, d.max(0).tolist()
    assert share <= 1e-3, share
    assert ref.tables()["finv"].size == 8754 and ref.tables()["gi"].size == 16321


def test_clahe_one_tile_without_clipping_is_global_equalisation():
    L = ref.content("noise", 40, 56, 5)[..., 0] // 2 + 30
    got = ref.clahe(L, clip_limit=0.0, tiles_x=1, tiles_y=1)
    cdf = np.cumsum(np.bincount(L.ravel(), minlength=256))
    lut = np.clip(np.rint(cdf.astype(np.float32) * (np.float32(255.0) / np.float32(L.size))), 0, 255).astype(np.uint8)
    assert (ref.clahe_luts(L, 0.0, 1, 1)[0, 0] == lut).all()
    assert (got == lut[L]).all()


def test_clahe_constant_crop_maps_to_a_constant():
    for v in (0, 90, 255):
        for shape, grid in (((64, 64), (8, 8)), ((73, 67), (8, 8)), ((16, 16), (16, 16))):
            out = ref.clahe(np.full(shape, v, np.uint8), 2.0, *grid)
            assert (out == out[0, 0]).all(), (v, shape, grid)


def test_clahe_tile_geometry():
    assert ref.clahe_geometry(64, 64, 8, 8) == (64, 64, 8, 8)            # divides: no padding
    assert ref.clahe_geometry(73, 67, 8, 8)[2:] == (10, 9)               # 67 x 73 (w x h): tile 9 x 10
    assert ref.clahe_geometry(73, 64, 8, 8) == (80, 72, 10, 9)           # the width divides, yet it is padded by 8 because the height does not
    L = ref.content("noise", 64, 64, 1)[..., 0]
    luts = ref.clahe_luts(L, 2.0, 8, 8)
    tile = L[8:16, 16:24]                                                # tile (1, 2) is the crop's own pixels
    assert (luts[1, 2] == ref.lut_of_hist(np.bincount(tile.ravel(), minlength=256), ref.clip_of(2.0, 64), 64)).all()


def test_clahe_residual_spread():
    hist = np.zeros(256, np.int64)
    hist[7] = 1000                                                       # clip 10: clipped 990 = 3 * 256 + 222, step 1: bins 0..221 get one more
    lut = ref.lut_of_hist(hist, 10, 1000)
    flat = np.full(256, 3)
    flat[7] += 10
    flat[:222] += 1
    want = np.clip(np.rint(np.cumsum(flat).astype(np.float32) * (np.float32(255.0) / np.float32(1000))), 0, 255)
    assert (lut == want).all()
    hist[7] = 10 + 256 + 100                                             # residual 100: step 2, bins 0, 2, .., 198
    lut = ref.lut_of_hist(hist, 10, 366)
    flat = np.full(256, 1)
    flat[7] += 10
    flat[0:200:2] += 1
    assert flat.sum() == 366
    assert (lut == np.clip(np.rint(np.cumsum(flat).astype(np.float32) * (np.float32(255.0) / np.float32(366))), 0, 255)).all()


def test_bilateral_properties():
    assert len(ref.bilateral_weights(9, 75.0, 75.0)[1]) == 49
    assert ref.bilateral_weights(9, 75.0, 75.0)[0] == 4 and ref.bilateral_radius(0, 3.0) == 4 and ref.bilateral_radius(15, 1.0) == 7
    const = np.full((20, 31, 3), (12, 200, 99), np.uint8)
    assert (ref.bilateral(const) == const).all()
    img = ref.content("noise", 24, 17, 3)
    assert (ref.bilateral(img, 9, 1e-3, 75) == img).all()                # no colour but the pixel's own has any weight


def test_layout_is_host_code_of_the_library():
    rects = [(0, 0, 16, 16), (5, 7, 72, 80), (3, 3, 134, 73), (0, 0, 1920, 1080)]
    off = enhance.layout(rects)
    assert len(off) == len(rects) + 1 and off[0] == 0
    sizes = [3 * (r[2] - r[0]) * (r[3] - r[1]) for r in rects]
    for i, s in enumerate(sizes):
        assert off[i + 1] - off[i] >= s                                  # monotonic, no two crops overlap
    assert off[-1] >= sum(sizes)
    assert enhance.layout([]) == [0]
    assert enhance.layout(rects[1:3])[1] == off[2] - off[1]              # position independent: a chunk of a long list lies as the list says
    for bad in ((0, 0, 15, 16), (0, 0, 16, 15), (-1, 0, 20, 20), (10, 10, 5, 40)):
        with pytest.raises(_capi.RtdError) as ei:
            enhance.layout([rects[0], bad])
        assert ei.value.code == _capi.RTD_E_INVALID
    offsets = (np.zeros(2, np.int64) - 7)
    import ctypes as C
    rc = (C.c_int32 * 4)(0, 0, 15, 16)
    assert _capi.lib().rtd_enhance_layout(1, rc, offsets.ctypes.data_as(C.POINTER(C.c_int64))) == _capi.RTD_E_INVALID


def fake_image_enhancer(method="clahe", grid=(8, 8), d=9, sigma_space=75):
    return types.SimpleNamespace(method=method, clahe_clip_limit=2.0, clahe_tile_grid_size=grid, bilateral_d=d, bilateral_sigma_color=75,
                                 bilateral_sigma_space=sigma_space)


def test_from_reference_refuses_what_the_library_cannot_stand_in_for():
    CE = enhance.CropEnhancer
    assert CE.from_reference(None, 64) is None
    assert CE.from_reference(fake_image_enhancer("realesrgan"), 64) is None
    assert CE.from_reference(fake_image_enhancer("none"), 64) is None
    assert CE.from_reference(fake_image_enhancer(grid=(32, 32)), 64) is None
    assert CE.from_reference(fake_image_enhancer(grid=(8, 17)), 64) is None
    assert CE.from_reference(fake_image_enhancer(d=17), 64) is None
    assert CE.from_reference(fake_image_enhancer(d=0, sigma_space=75), 64) is None        # radius rint(112.5)
    assert CE.from_reference(fake_image_enhancer(), 8) is None
    assert enhance.within_limits((16, 16), 15, 75) and enhance.within_limits((1, 1), 3, 75) and enhance.within_limits((8, 8), 0, 3.0)


class _Pipeline:
    """the attributes BatchedStage2 reads, with an enhancer and the reference's own per-detection method"""

    def __init__(self, enhancer):
        self.enable_species_classification = True
        self.class_id_to_category = {14: "bird"}
        self.species_classifiers = {"bird": object()}
        self.min_crop_size = 64
        self.crop_padding_percent = 20
        self.rejected_taxonomic_levels = []
        self.time_of_day_top_k = 5
        self.time_of_day_penalty = 0.3
        self.enhancer = enhancer
        self.calls = []

    def process_detections(self, frame, dets):
        self.calls.append((frame, dets))
        return [dict(d, species="per-detection path") for d in dets]


def test_default_keeps_the_fallback_for_pipelines_with_an_enhancer():
    p = _Pipeline(fake_image_enhancer())
    s2 = BatchedStage2(p, batcher=object())
    assert s2.enhancer is None
    dets = [{"class_id": 14, "bbox": {"x1": 0, "y1": 0, "x2": 100, "y2": 100}}]
    out = s2.process_batch(["frame0", "frame1"], [dets, []])
    assert [len(o) for o in out] == [1, 0] and out[0][0]["species"] == "per-detection path"
    assert [c[0] for c in p.calls] == ["frame0", "frame1"]
    # "auto" with an enhancer the library cannot stand in for: the same fallback, and nothing touches the GPU
    for ie in (fake_image_enhancer("realesrgan"), fake_image_enhancer(grid=(32, 32))):
        p = _Pipeline(ie)
        s2 = BatchedStage2(p, batcher=object(), enhancer="auto")
        assert s2.enhancer is None
        assert s2.process_batch(["f"], [dets])[0][0]["species"] == "per-detection path"
    p = _Pipeline(fake_image_enhancer())
    p.min_crop_size = 8
    assert BatchedStage2(p, batcher=object(), enhancer="auto").enhancer is None
    with pytest.raises(ValueError):
        BatchedStage2(p, batcher=object(), enhancer="clahe")


def test_a_given_enhancer_takes_the_batched_path_and_books_its_time():
    from collections import deque

    from tests.standins import StandInSpeciesClassifier

    class FakeEnhancer:
        def last_call_ms(self):
            return 6.0

    class FakeBatcher:
        def __init__(self):
            self.seen = []

        def preprocess_batch(self, frames, rects_per_frame, enhancer=None):
            import torch
            self.seen.append((enhancer, [list(r) for r in rects_per_frame]))
            n = sum(len(r) for r in rects_per_frame)
            return torch.zeros((n, 3, 32, 32))

    import torch
    p = _Pipeline(fake_image_enhancer())
    p.species_classifiers = {"bird": StandInSpeciesClassifier(input_size=32, device="cpu")}
    p.enhancement_times = deque(maxlen=1000)
    fe, fb = FakeEnhancer(), FakeBatcher()
    s2 = BatchedStage2(p, batcher=fb, enhancer=fe)
    frames = [torch.zeros((200, 300, 3), dtype=torch.uint8), torch.zeros((240, 320, 3), dtype=torch.uint8)]
    dets = [[{"class_id": 14, "bbox": {"x1": 10, "y1": 10, "x2": 110, "y2": 120}}, {"class_id": 14, "bbox": {"x1": 50, "y1": 20, "x2": 150, "y2": 190}}],
            [{"class_id": 14, "bbox": {"x1": 0, "y1": 0, "x2": 100, "y2": 100}}]]
    out = s2.process_batch(frames, dets)
    assert not p.calls and len(fb.seen) == 1 and fb.seen[0][0] is fe and [len(r) for r in fb.seen[0][1]] == [2, 1]
    assert all("species" in d and d["stage2_category"] == "bird" for per in out for d in per)
    assert list(p.enhancement_times) == [2.0, 2.0, 2.0]


def test_matches_cv2_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    for kind, h, w in (("noise", 64, 64), ("ramp", 73, 67), ("noise", 73, 64), ("ramp", 70, 131)):
        img = ref.content(kind, h, w, 9)
        st = ref.stages(img)
        lab = cv2.cvtColor(img, cv2.COLOR_BGR2LAB)
        d = np.abs(lab.astype(int) - st["lab"].astype(int)).reshape(-1, 3).max(0)
        assert (d <= np.array([1, 3, 2])).all(), d
        theirs = cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(np.ascontiguousarray(st["lab"][..., 0]))
        assert (theirs == ref.clahe(st["lab"][..., 0], 2.0, 8, 8)).all()                       # the same L plane: exact
        lab2 = st["lab"].copy()
        lab2[..., 0] = theirs
        assert np.abs(cv2.cvtColor(lab2, cv2.COLOR_LAB2BGR).astype(int) - st["bgr"].astype(int)).max() <= 3
        assert np.abs(cv2.bilateralFilter(st["bgr"], 9, 75, 75).astype(int) - st["out"].astype(int)).max() <= 3
