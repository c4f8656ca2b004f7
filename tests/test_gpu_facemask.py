"""The face masks on the MI355X (csrc/facemask.hip): every comparison is exact equality with the numpy restatement (tests/face_ref.py),
on seeded noise frames (smooth content hides an off-by-one tap).  Frames are 1 x 1, 5 x 7, 37 x 223 (odd 3 W) and 160 x 224; regions are
the smallest that reach each path of the kernels - shorter than the radius, one tile, one tile and one more pixel each way, clipped at
each corner, the whole frame - for every style, kernel size and block count.  The frames of a call lie in one buffer, at addresses of
every alignment, with guard bytes everywhere else: a byte outside the padded rectangles that changes fails the comparison.  Then the
order of overlapping faces, mixed batches, the Python class (copies, numpy frames, stream order), the gray plane, the limits, the handle
scaffold and the chain ingest -> mask -> overlay -> JPEG."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import face_ref as ref
from tests import motion_ref
from telescope_cam_detection_amd import _capi
from telescope_cam_detection_amd import face_masker as fm

pytestmark = pytest.mark.gpu

GUARD = 0xA5
TH, TW = fm.plan([(1, 1)], [])["tile"]                      # host arithmetic (rtd_debug_facemask_plan): no GPU is touched at import
H, W = 160, 224
KS = [1, 3, 7, 9, 25, 63, 65, 99]
STYLE_OF = {fm.BLUR: "gaussian_blur", fm.PIXELATE: "pixelate", fm.BLACK_BOX: "black_box"}


@pytest.fixture(scope="module")
def be():
    b = fm.DeviceBackend(0)
    yield b
    b.close()


def face_for(x1, y1, rw, rh, H, W):
    """a face whose padded rectangle on an H x W frame is exactly [x1, x1 + rw) x [y1, y1 + rh)"""
    for w in range(1, 2 * W + 2):
        p = int(w * 0.2)
        for x in ([x1 + p] if x1 > 0 else range(p + 1)):
            if min(W, x + w + p) != x1 + rw:
                continue
            for y in ([y1 + p] if y1 > 0 else range(p + 1)):
                for h in range(1, 2 * H + 2):
                    if ref.padded_rect((x, y, w, h), H, W) == (x1, y1, x1 + rw, y1 + rh):
                        return (x, y, w, h)
    raise AssertionError(f"no face pads to {(x1, y1, rw, rh)} on {H} x {W}")


def want_of(frames, rows):
    """the reference's loop: the faces one after another, each on the output of the one before"""
    out = [np.array(f) for f in frames]
    for (i, x, y, w, h, style, param) in rows:
        ref.apply_face(out[i], (x, y, w, h), STYLE_OF[style], blur_strength=param, pixelate_blocks=param)
    return out


class Frames:
    """the frames of a call in one device buffer, frame i at an address = skews[i] mod 4, guard bytes everywhere else"""

    def __init__(self, frames, skews=None):
        self.shapes, self.offs, at = [f.shape for f in frames], [], 64
        for i, f in enumerate(frames):
            at = (at + 3) // 4 * 4 + (skews[i] if skews else i % 4)
            self.offs.append(at)
            at += f.size + 32
        host = np.full(at + 64, GUARD, np.uint8)
        for f, o in zip(frames, self.offs):
            host[o:o + f.size] = f.reshape(-1)
        self.buf = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()

    def ptrs(self):
        return [self.buf.data_ptr() + o for o in self.offs]

    def check(self, want):
        got = self.buf.cpu().numpy()
        rest = np.ones(got.size, bool)
        for i, (s, o) in enumerate(zip(self.shapes, self.offs)):
            g = got[o:o + want[i].size].reshape(s)
            assert (g == want[i]).all(), (i, s, np.argwhere(g != want[i])[:4].tolist())
            rest[o:o + want[i].size] = False
        assert (got[rest] == GUARD).all(), "a byte outside the frames was written"


def run(be, frames, rows, skews=None):
    """one call on device frames in a guarded buffer, compared whole with the sequential restatement; returns the masked frames"""
    want = want_of(frames, rows)
    held = Frames(frames, skews)
    rc = be.apply_raw(held.ptrs(), held.shapes, True, rows)
    assert rc == _capi.RTD_OK, (rc, be._fn("last_error")(be._h))
    held.check(want)
    return want


def params(style):
    return [25, 99] if style == fm.BLUR else [1, 2, 3, 10, 1000] if style == fm.PIXELATE else [0]


REGIONS = {                                                  # on the 160 x 224 frame: x1, y1, rw, rh
    "shorter than the radius, clipped bottom right": (W - 5, H - 5, 5, 5),
    "one tile, clipped top left": (0, 0, TW, TH),
    "one tile and a column, clipped top right": (W - TW - 1, 0, TW + 1, TH),
    "one tile and a row, clipped bottom left": (0, H - TH - 1, TW, TH + 1),
    "one tile and one more each way, clipped bottom right": (W - TW - 1, H - TH - 1, TW + 1, TH + 1),
    "inside, many tiles": (37, 21, 3 * TW - 7, 4 * TH + 3),
    "the whole frame": (0, 0, W, H),
}


@pytest.mark.parametrize("style", [fm.BLUR, fm.PIXELATE, fm.BLACK_BOX], ids=["blur", "pixelate", "black_box"])
@pytest.mark.parametrize("region", sorted(REGIONS))
def test_every_region_class_with_this_style(be, style, region):
    x1, y1, rw, rh = REGIONS[region]
    face = face_for(x1, y1, rw, rh, H, W)
    for k, param in enumerate(params(style)):
        frame = ref.noise(100 + k, H, W)
        masked = run(be, [frame], [(0, *face, style, param)], skews=[k % 4])
        if not (style == fm.PIXELATE and param == 1):         # (blocks = 1 is the identity)
            assert (masked[0] != frame).any()


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (37, 223), (5, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_and_odd_frames_with_every_style_and_parameter(be, hw):
    """the face is the frame, a corner of it, and (where the frame has room) a region inside it; 5 x 5 with k = 25 and k = 99 is the
    region shorter than the radius as a frame of its own"""
    h, w = hw
    faces = [(0, 0, w, h), (w - 2, h - 2, 4, 4), (-3, -3, 5, 5)] + ([(w // 3, h // 3, 3, 2)] if h >= 5 else [])
    rows, frames = [], []
    for style in (fm.BLUR, fm.PIXELATE, fm.BLACK_BOX):
        for param in (KS if style == fm.BLUR else params(style)):
            for face in faces:
                frames.append(ref.noise(len(frames), h, w))
                rows.append((len(frames) - 1, *face, style, param))
    for i in range(0, len(frames), fm.MAX_FRAMES):
        part = [(r[0] - i,) + r[1:] for r in rows[i:i + fm.MAX_FRAMES]]
        run(be, frames[i:i + fm.MAX_FRAMES], part)


def test_every_kernel_size_on_a_region_with_halos_inside_and_outside_the_region(be):
    """3 x 2 tiles and a bit: the halo of an inner tile is other tiles' pixels, that of an outer one is reflected"""
    face = face_for(11, 7, 2 * TW + 9, 3 * TH + 5, H, W)
    frames = [ref.noise(200 + k, H, W) for k in KS]
    run(be, frames, [(i, *face, fm.BLUR, k) for i, k in enumerate(KS)])
    narrow = [(0, 30, 3, 60), (100, 3, 90, 3)]              # 3 x 60 pixels (no padding), and 126 x 24 from a 3-row face at the top
    run(be, frames[:2], [(i, *narrow[i], fm.BLUR, 99) for i in range(2)] + [(i, *narrow[1 - i], fm.PIXELATE, 7) for i in range(2)])


def test_two_overlapping_faces_in_both_orders_give_different_bytes(be):
    frame = ref.noise(300, H, W)
    a, b = (40, 40, 50, 40), (70, 60, 50, 40)
    for sa, pa, sb, pb in ((fm.BLUR, 25, fm.BLUR, 9), (fm.BLUR, 25, fm.PIXELATE, 10), (fm.BLACK_BOX, 0, fm.BLUR, 63), (fm.PIXELATE, 3, fm.BLACK_BOX, 0)):
        ab = run(be, [frame], [(0, *a, sa, pa), (0, *b, sb, pb)])[0]
        ba = run(be, [frame], [(0, *b, sb, pb), (0, *a, sa, pa)])[0]
        assert (ab != ba).any()
    # a chain of three (three layers), and the same face twice (the second blurs the first's output)
    run(be, [frame], [(0, 10, 10, 40, 40, fm.BLUR, 25), (0, 50, 20, 40, 40, fm.PIXELATE, 5), (0, 90, 30, 40, 40, fm.BLUR, 7)])
    twice = run(be, [frame], [(0, *a, fm.BLUR, 25)] * 2)[0]
    assert (twice != run(be, [frame], [(0, *a, fm.BLUR, 25)])[0]).any()
    assert fm.plan([frame.shape], [(0, *a, fm.BLUR, 25)] * 2)["layers"] == 2


def test_three_frames_of_different_sizes_with_0_1_and_4_faces_and_all_four_styles_in_one_call(be):
    frames = [ref.noise(400, 37, 223), ref.noise(401, 5, 7), ref.noise(402, H, W)]
    masker = fm.FaceMasker(blur_strength=25, pixelate_blocks=10, detector=lambda g: [])
    faces = [(10, 10, 60, 50), (100, 20, 50, 60), (60, 70, 70, 60), (150, 100, 90, 90)]      # the third meets the first two
    styles = ["gaussian_blur", "pixelate", "adaptive_blur", "black_box"]
    rows = masker._face_rows(1, frames[1].shape, [(1, 1, 3, 2)], "pixelate")
    for f, s in zip(faces, styles):
        rows += masker._face_rows(2, frames[2].shape, [f], s)
    assert rows[3][5:] == (fm.BLUR, ref.adaptive_k(25, faces[2], H, W)) and rows[3][6] != 25
    want = run(be, frames, rows, skews=[1, 2, 3])
    assert (want[0] == frames[0]).all()
    whole = ref.apply_mask(frames[2], faces, styles, 25, 10)    # face_ref's own loop, with the styles by name
    assert (want[2] == whole).all()


def test_1024_faces_of_one_pixel(be):
    frame = ref.noise(500, 37, 223)
    rows = [(0, (7 * i) % 223, (i // 32), 1, 1, i % 3, [3, 1, 0][i % 3]) for i in range(1024)]
    want = run(be, [frame], rows)
    assert (want[0] != frame).any()
    assert be.apply_raw([1], [(37, 223, 3)], True, rows + rows[:1]) == _capi.RTD_E_INVALID


# ---- the class --------------------------------------------------------------------------------------------------------------------------
FACES = [(30, 20, 60, 50), (70, 50, 50, 40), (180, 120, 60, 60)]


@pytest.mark.parametrize("style", ref.STYLES)
def test_apply_mask_returns_a_new_tensor_leaves_its_input_and_numpy_frames_give_the_same_bytes(style):
    m = fm.FaceMasker(mask_style=style, blur_strength=25, pixelate_blocks=10, device=0, detector=lambda g: FACES)
    a = np.array(ref.noise(600, H, W))
    want = ref.apply_mask(a, FACES, style, 25, 10)
    dev = torch.from_numpy(a).cuda()
    got = m.apply_mask(dev, FACES)
    assert got is not dev and got.data_ptr() != dev.data_ptr() and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3)
    assert (got.cpu().numpy() == want).all() and (dev.cpu().numpy() == a).all()
    host = m.apply_mask(a, FACES)
    assert isinstance(host, np.ndarray) and host is not a and (host == want).all() and (a == ref.noise(600, H, W)).all()
    masked, faces = m.detect_and_mask(dev)
    assert faces == FACES and (masked.cpu().numpy() == want).all()
    other = ref.STYLES[(ref.STYLES.index(style) + 1) % 4]       # the per-call override
    assert (m.apply_mask(dev, FACES, mask_style=other).cpu().numpy() == ref.apply_mask(a, FACES, other, 25, 10)).all()
    assert m.apply_mask(dev, []) is dev
    with pytest.raises(ValueError):
        m.apply_mask(dev[:, ::2], FACES)
    with pytest.raises(ValueError):
        m.apply_mask(dev.float(), FACES)
    m.close()


def test_apply_mask_batch_is_one_call_for_a_ticks_cameras():
    m = fm.FaceMasker(mask_style="gaussian_blur", device=0, detector=lambda g: [])
    frames = [np.array(ref.noise(700 + i, h, w)) for i, (h, w) in enumerate([(H, W), (37, 223), (64, 48)])]
    per = [FACES[:2], [], [(10, 10, 20, 20)]]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    got = m.apply_mask_batch(dev, per)
    assert got[1] is dev[1] and got[0] is not dev[0]
    for g, f, faces in zip(got, frames, per):
        assert (g.cpu().numpy() == ref.apply_mask(f, faces, "gaussian_blur", 25)).all()
    host = m.apply_mask_batch(frames, per, mask_style="pixelate")
    assert host[1] is frames[1] and all((h == ref.apply_mask(f, faces, "pixelate", 25, 10)).all() for h, f, faces in zip(host, frames, per))
    with pytest.raises(ValueError):
        m.apply_mask_batch([dev[0], frames[1]], per[:2])
    many = [(3 * (i % 70), 2 * (i // 70), 1, 1) for i in range(1100)]      # more faces than one call takes: two calls, in order
    assert (m.apply_mask(dev[0], many, "black_box").cpu().numpy() == ref.apply_mask(frames[0], many, "black_box")).all()
    m.close()


def test_a_frame_written_on_a_side_stream_just_before_the_call():
    m = fm.FaceMasker(device=0, detector=lambda g: [])
    a = np.array(ref.noise(800, H, W))
    src = torch.from_numpy(a).pin_memory()
    frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)                       # the write below is still pending when the calls are made
        frame.copy_(src, non_blocking=True)
        got = m.apply_mask(frame, FACES)                    # ordered after `side`, torch's current stream here
        gray = m._backend(frame).gray(frame)
    assert (got.cpu().numpy() == ref.apply_mask(a, FACES, "gaussian_blur", 25)).all()
    assert (gray == motion_ref.as_gray(a)).all()
    torch.cuda.synchronize()
    m.close()


@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (5, 7), (37, 223), (H, W)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_gray_plane_equals_the_restatement_at_every_alignment(be, hw):
    h, w = hw
    a = ref.noise(900, h, w)
    for skew in range(4):
        held = Frames([a], skews=[skew])
        out = np.full(h * w + 16, GUARD, np.uint8)
        rc = be._L.rtd_facemask_gray(be._h, C.c_void_p(held.ptrs()[0]), h, w, C.c_void_p(out.ctypes.data + 8))
        assert rc == _capi.RTD_OK, be._fn("last_error")(be._h)
        assert (out[8:8 + h * w].reshape(h, w) == motion_ref.as_gray(a)).all() and (out[:8] == GUARD).all() and (out[8 + h * w:] == GUARD).all()
        held.check([a])                                     # the frame and the bytes around it stay as they were


def test_detect_faces_on_a_device_frame_hands_the_detector_the_gray_plane():
    seen = []
    m = fm.FaceMasker(device=0, detector=lambda g: seen.append(g) or [(1, 2, 3, 4)])
    a = np.array(ref.noise(901, 37, 223))
    assert m.detect_faces(torch.from_numpy(a).cuda()) == [(1, 2, 3, 4)]
    assert isinstance(seen[0], np.ndarray) and seen[0].dtype == np.uint8 and (seen[0] == motion_ref.as_gray(a)).all()
    m.close()


# ---- limits and the scaffold --------------------------------------------------------------------------------------------------------------
def test_a_refused_call_names_its_face_and_writes_nothing_and_the_handle_goes_on(be):
    frames = [ref.noise(1000, 48, 64), ref.noise(1001, 5, 7)]
    good = [(0, 10, 10, 20, 20, fm.BLUR, 25), (1, 0, 0, 3, 3, fm.PIXELATE, 2)]
    held = Frames(frames)
    for rows, names in (([good[0], (1, 0, 0, 3, 3, fm.BLUR, 4)], b"face 1"), ([(2,) + good[0][1:], good[1]], b"face 0"),
                        ([good[0], (1, 0, 0, 3, 3, 7, 2)], b"face 1"), ([good[0], (1, 0, 0, 3, 3, fm.PIXELATE, 0)], b"face 1")):
        assert be.apply_raw(held.ptrs(), held.shapes, True, rows) == _capi.RTD_E_INVALID
        assert names in be._fn("last_error")(be._h)
    assert be.apply_raw([held.ptrs()[0], None], held.shapes, True, good) == _capi.RTD_E_INVALID and b"frame 1" in be._fn("last_error")(be._h)
    assert be.apply_raw(held.ptrs(), [(48, 64, 3), (0, 7, 3)], True, good) == _capi.RTD_E_INVALID
    assert be.apply_raw(held.ptrs(), held.shapes, True, good, n=0) == _capi.RTD_E_INVALID
    assert be._L.rtd_facemask_apply(be._h, 2, None, (C.c_int32 * 4)(48, 64, 5, 7), 1, 0, None) == _capi.RTD_E_INVALID
    assert be._L.rtd_facemask_gray(be._h, None, 4, 4, None) == _capi.RTD_E_INVALID
    held.check(frames)                                      # none of the refused calls wrote
    assert be.apply_raw(held.ptrs(), held.shapes, True, [(0, 500, 10, 20, 20, fm.BLUR, 3)]) == _capi.RTD_OK      # an empty rectangle is skipped
    assert be.apply_raw(held.ptrs(), held.shapes, True, []) == _capi.RTD_OK
    held.check(frames)
    assert be.apply_raw(held.ptrs(), held.shapes, True, good) == _capi.RTD_OK
    held.check(want_of(frames, good))


def test_create_refused_create_wait_stream_and_close_as_the_scaffold_promises():
    L = _capi.lib()
    h = C.c_void_p(0xDEAD)
    assert L.rtd_facemask_create(torch.cuda.device_count(), C.byref(h)) == _capi.RTD_E_INVALID and h.value is None
    assert b"no such device" in L.rtd_facemask_last_error(None)
    assert L.rtd_facemask_create(0, None) == _capi.RTD_E_INVALID
    with pytest.raises(_capi.RtdError, match="no such device"):
        fm.DeviceBackend(torch.cuda.device_count())
    b = fm.DeviceBackend(0)
    try:
        assert b._h.value and (L.rtd_facemask_last_error(b._h) or b"") == b""
        b.wait_stream(0)
        frame = ref.noise(1100, 48, 64)
        rows = [(0, 10, 10, 20, 20, fm.BLUR, 25), (0, 20, 20, 20, 20, fm.PIXELATE, 4)]
        first = run(b, [frame], rows)[0].tobytes()
        assert b.apply_raw([1], [frame.shape], True, [(0, 10, 10, 20, 20, fm.BLUR, 24)]) == _capi.RTD_E_INVALID
        assert b"face 0" in L.rtd_facemask_last_error(b._h)
        assert run(b, [frame], rows)[0].tobytes() == first
    finally:
        b.close()
    assert not b._h.value
    b.close()                                               # closing twice is harmless
    L.rtd_facemask_destroy(None)


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
def test_ingest_mask_frame_overlay_and_jpeg_give_the_masked_frames_jpeg():
    from tests import jpeg_ref, overlay_ref, yuv_ref
    from telescope_cam_detection_amd import ingest, overlay as ov

    planes = yuv_ref.scene_planes(7, H, W)
    bgr = yuv_ref.planes_to_bgr(*planes)
    ing = ingest.FrameIngest(0)
    frame = ing.to_bgr([yuv_ref.pack(*planes, layout="nv12")[0].tobytes()], [(H, W)])[0]
    calls = []
    masker = fm.FaceMasker(mask_style="gaussian_blur", device=0, detector=lambda g: calls.append(g) or FACES[:2])
    cache = fm.FaceMaskingCache(ttl_frames=5)
    want = ref.apply_mask(bgr, FACES[:2], "gaussian_blur", 25)
    r = ov.OverlayRenderer(device=0, rasteriser=overlay_ref.FakeRasteriser())
    result = [x for x in overlay_ref.load_golden()["scenarios"] if x["name"] == "web_top_edge"][0]["result"]
    p, msk = ov.lower([ov.plan_web(result, r.rasteriser)], r.cache)
    jpegs = [jpeg_ref.encode(want, 90), jpeg_ref.encode(overlay_ref.composite(want, p[0], msk), 90)]
    try:
        for tick in range(2):                               # the second tick reuses the cached faces: one detection in all
            masked = fm.mask_frame(masker, cache, frame, "c1")
            assert masked.is_cuda and masked is not frame and (masked.cpu().numpy() == want).all()
            assert r.mjpeg_tick([masked, masked], [None, result], 90) == jpegs
        assert len(calls) == 1 and (calls[0] == motion_ref.as_gray(bgr)).all() and cache.cache["c1"][1] == 1
        assert (frame.cpu().numpy() == bgr).all()           # the camera's frame stays unmasked

        class Server:                                       # the reference's method behind install(): a device frame stays on the device
            face_masker, face_masking_cache = masker, fm.FaceMaskingCache()

            def _is_face_masking_enabled_for_camera(self, camera_id):
                return camera_id != "off"

            def _apply_face_masking_to_frame(self, f, camera_id):
                raise AssertionError("only host frames go to the original method")

        fm.install(Server)
        s = Server()
        assert (s._apply_face_masking_to_frame(frame, "c2").cpu().numpy() == want).all() and s._apply_face_masking_to_frame(frame, "off") is frame
    finally:
        r.close()
        ing.close()
        masker.close()

