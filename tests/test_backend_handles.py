"""The handle scaffold the seven handles share - the detector engine and the six stand-alone back ends (csrc/backend.h, _capi.Handle):
what a refused create returns and leaves behind, where its message is kept (one string per handle type and per thread), and - on the
GPU - one create / call / refused call / call / close round of every handle against the restatement its own GPU test uses.

The first five tests need no GPU: a bad parameter is refused before any HIP call, and a device that does not exist is refused with
RTD_E_INVALID where a GPU is present and with RTD_E_HIP (no device at all) where none is.  (rtd_create itself never touches the device:
the engine meets a missing one in rtd_load_weights, on the GPU below.)"""
import ctypes as C
import threading

import numpy as np
import pytest

from telescope_cam_detection_amd import _capi

BACKENDS = ("motion", "mog2", "jpeg", "overlay", "enhance", "esrgan")
HANDLES = BACKENDS + ("engine",)
NO_DEVICE = 10 ** 6
_BLOB = {}


def esrgan_blob():
    """a well-formed one-block weight blob (rtd_esrgan_create checks the blob before it looks at the device)"""
    if "b" not in _BLOB:
        from tests import esrgan_ref
        from telescope_cam_detection_amd import esrgan
        _BLOB["b"] = esrgan.load_state(esrgan_ref.synth_state(1, 0), 1)
    return _BLOB["b"]


def enhance_params(tiles_x=8):
    p = _capi.RtdEnhanceParams()
    p.struct_size = C.sizeof(_capi.RtdEnhanceParams)
    p.clip_limit, p.tiles_x, p.tiles_y, p.bilateral_d, p.sigma_color, p.sigma_space = 2.0, tiles_x, 8, 9, 75.0, 75.0
    return p


def esrgan_config(device, num_block=1):
    c = _capi.RtdEsrganConfig()
    c.struct_size = C.sizeof(_capi.RtdEsrganConfig)
    c.device, c.precision, c.num_feat, c.num_grow_ch, c.num_block, c.tile, c.tile_pad = device, _capi.PREC_F16X3, 64, 32, num_block, 0, 10
    return c


def engine_config(device, bad=False):
    from telescope_cam_detection_amd.arch import ARCHS
    return _capi.make_config(ARCHS["tiny"], device, _capi.PREC_FP32, 1, (641 if bad else 160, 160), False)


def raw_create(name, device, bad=False):
    """rtd_<name>_create (the engine's: rtd_create) as it is, with valid parameters or with the handle's one bad parameter: (return
    code, handle value)"""
    L = _capi.lib()
    h = C.c_void_p(0xDEAD)                                  # a refused create must overwrite this with NULL
    if name == "motion":
        rc = L.rtd_motion_create(device, 4 if bad else 21, C.byref(h))
    elif name == "mog2":
        rc = L.rtd_mog2_create(device, 0 if bad else 500, 16.0, 1, C.byref(h))
    elif name == "jpeg":
        rc = L.rtd_jpeg_create(device, C.byref(h))
    elif name == "overlay":
        rc = L.rtd_overlay_create(device, C.byref(h))
    elif name == "enhance":
        rc = L.rtd_enhance_create(device, C.byref(enhance_params(17 if bad else 8)), C.byref(h))
    elif name == "engine":
        rc = L.rtd_create(C.byref(engine_config(device, bad)), C.byref(h))
    else:
        if bad:
            rc = L.rtd_esrgan_create(C.byref(esrgan_config(device, 0)), None, 0, C.byref(h))
        else:
            blob = esrgan_blob()
            rc = L.rtd_esrgan_create(C.byref(esrgan_config(device)), (C.c_char * len(blob)).from_buffer_copy(blob), len(blob), C.byref(h))
    return rc, h.value


def create_error(name) -> bytes:
    return getattr(_capi.lib(), "rtd_last_error" if name == "engine" else f"rtd_{name}_last_error")(None) or b""


BAD = {"motion": b"blur_size must be odd", "mog2": b"history must be >= 1", "enhance": b"tile grid must be 1..16", "esrgan": b"num_block must be 1..32",
       "engine": b"multiple of 32"}


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_bad_parameter_is_refused_as_invalid_with_its_message(name):
    rc, h = raw_create(name, 0, bad=True)
    assert rc == _capi.RTD_E_INVALID and h is None
    assert BAD[name] in create_error(name), create_error(name)


@pytest.mark.parametrize("name", BACKENDS)
def test_a_device_that_does_not_exist_is_refused(name):
    import torch
    rc, h = raw_create(name, NO_DEVICE)
    assert rc == (_capi.RTD_E_INVALID if torch.cuda.is_available() else _capi.RTD_E_HIP), (rc, create_error(name))
    assert h is None and len(create_error(name)) > 0


def in_thread(fn):
    out = {}
    t = threading.Thread(target=lambda: out.setdefault("v", fn()))
    t.start()
    t.join()
    return out["v"]


def test_every_back_end_keeps_its_own_create_message():
    def body():                                             # a fresh thread: nothing has failed in it yet
        rc, h = raw_create("jpeg", NO_DEVICE)
        return rc, h, create_error("jpeg"), create_error("overlay")
    rc, h, jpeg_msg, overlay_msg = in_thread(body)
    assert rc != _capi.RTD_OK and h is None and len(jpeg_msg) > 0
    assert overlay_msg == b""


def test_the_create_message_belongs_to_the_thread_that_failed():
    rc, _ = raw_create("motion", 0, bad=True)
    assert rc == _capi.RTD_E_INVALID
    mine = create_error("motion")
    assert BAD["motion"] in mine
    assert in_thread(lambda: create_error("motion")) == b""
    assert create_error("motion") == mine


def test_the_engines_create_message_is_its_own_and_its_threads():
    rc, h = raw_create("engine", 0, bad=True)               # input size 641
    assert rc == _capi.RTD_E_INVALID and h is None
    mine = create_error("engine")
    assert BAD["engine"] in mine

    def body():                                             # a fresh thread: empty; and the jpeg back end's refusal goes to its own string
        before = create_error("engine")
        rc, h = raw_create("jpeg", NO_DEVICE)
        return before, rc, create_error("jpeg"), create_error("engine")
    before, rc, jpeg_msg, engine_msg = in_thread(body)
    assert before == b"" and rc != _capi.RTD_OK and len(jpeg_msg) > 0 and engine_msg == b""
    assert in_thread(lambda: (raw_create("engine", 0, bad=True), create_error("jpeg"))[1]) == b""
    assert create_error("engine") == mine


# ---- on the GPU: one round per handle ------------------------------------------------------------------------------------------
def frames16(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (16, 16, 3), dtype=np.uint8) for _ in range(2)]


class MotionRound:
    """a reset, a first frame (-1) and a second frame's motion area against tests/motion_ref.py"""

    def __init__(self, device):
        from tests import motion_ref
        from telescope_cam_detection_amd import motion
        self.be = motion.DeviceBackend(device, 21)
        self.f = frames16(1)
        ref = motion_ref.RefBackend(21)
        self.want = [ref.check([f], False, [0], 25)[0] for f in self.f]
        assert self.want[0] == -1 and self.want[1] >= 0

    def valid(self):
        self.be.reset(-1)
        got = [self.be.check([f], False, [0], 25)[0] for f in self.f]
        assert got == self.want
        return self.be.state(0, (16, 16)).tobytes()

    def refused(self):
        L = self.be._L
        return L.rtd_motion_check(self.be._h, 1, (C.c_void_p * 1)(None), (C.c_int32 * 3)(16, 16, 3), 0, (C.c_int32 * 1)(0), 25, (C.c_int64 * 1)())


class Mog2Round:
    """a new model, then two frames with one box each against tests/mog2_ref.py"""

    def __init__(self, device):
        from tests import mog2_ref
        from telescope_cam_detection_amd import motion_filter
        self.be = motion_filter.DeviceBackend(device, 500, 16, True)
        self.f = frames16(2)
        ref = mog2_ref.RefBackend(500, 16, True)
        self.box = (2, 3, 13, 12)
        self.want = [ref.apply(f, False, [self.box], 21) for f in self.f]

    def valid(self):
        self.be.configure(500, 16, True)
        got = [self.be.apply(f, False, [self.box], 21) for f in self.f]
        assert got == self.want
        return self.be.fg_bits(1, (16, 16)).tobytes()

    def refused(self):
        L = self.be._L
        return L.rtd_mog2_apply(self.be._h, None, (C.c_int32 * 3)(16, 16, 3), 0, 1, (C.c_int32 * 4)(*self.box), 21, (C.c_int64 * 1)())


class JpegRound:
    def __init__(self, device):
        from tests import jpeg_ref
        from telescope_cam_detection_amd import jpeg
        self.be = jpeg.DeviceBackend(device)
        self.f = frames16(3)[0]
        self.want = jpeg_ref.encode(self.f, 90)

    def valid(self):
        got = self.be.encode([self.f], False, 90)
        assert got == [self.want]
        return got[0]

    def refused(self):
        return self.be.encode_raw([None], [self.f.shape], False, 90, np.empty(4096, np.uint8))[0]


class OverlayRound:
    def __init__(self, device):
        from tests import overlay_ref as ref
        from telescope_cam_detection_amd import overlay
        self.be = overlay.DeviceBackend(device)
        self.f = frames16(4)[0]
        self.masks = np.arange(64, dtype=np.uint8) * 4
        self.prims = ref.prims(ref.prim(ref.FILL, 1, 2, 9, 6, (10, 20, 30)), ref.prim(ref.OUTLINE, 3, 3, 14, 13, (200, 100, 50), 2),
                               ref.prim(ref.MASK, 4, 5, 8, 8, (255, 255, 255)))
        self.want = ref.composite(self.f, self.prims, self.masks)

    def valid(self):
        got = self.be.draw([self.f], False, [self.prims], self.masks, False)[0].cpu().numpy()
        assert (got == self.want).all()
        return got.tobytes()

    def refused(self):
        import torch
        out = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
        return self.be.draw_raw([None], [self.f.shape], False, [self.prims], self.masks, [out.data_ptr()])


class CropRound:
    """one 16 x 16 crop of a 32 x 32 device frame"""
    RECT = (9, 7, 25, 23)

    def __init__(self):
        import torch
        self.frame_np = np.random.default_rng(5).integers(0, 256, (32, 32, 3), dtype=np.uint8)
        self.frame = torch.from_numpy(self.frame_np).cuda()
        x1, y1, x2, y2 = self.RECT
        self.crop = np.ascontiguousarray(self.frame_np[y1:y2, x1:x2])

    def refused(self):
        import torch
        out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        return self.call(self.be._h, 1, (C.c_void_p * 1)(None), (C.c_int32 * 2)(32, 32), (C.c_int32 * 4)(*self.RECT), C.c_void_p(out.data_ptr()),
                         out.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))


class EnhanceRound(CropRound):
    def __init__(self, device):
        from tests import enhance_ref
        from telescope_cam_detection_amd import enhance
        super().__init__()
        self.be = enhance.CropEnhancer(device=device)
        self.call = _capi.lib().rtd_enhance_crops
        self.want = enhance_ref.enhance(self.crop)

    def valid(self):
        buf, offsets, shapes = self.be.enhance([self.frame], [[self.RECT]])
        got = buf[:16 * 16 * 3].view(16, 16, 3).cpu().numpy()
        assert shapes == [(16, 16)] and offsets[0] == 0 and (got == self.want).all()
        return got.tobytes()


class EsrganRound(CropRound):
    """the gate of tests/test_gpu_esrgan.py: no byte off by more than 1 from the fp64 restatement, and no larger a share of differing
    bytes than plain fp16 (the reference's own half mode) has on the same crop - computed here, on the CPU, from the restatement"""

    def __init__(self, device):
        import torch
        from tests import esrgan_ref as ref
        from telescope_cam_detection_amd import esrgan
        super().__init__()
        sd = ref.synth_state(1, 0)
        self.be = esrgan.CropUpscaler(esrgan_blob(), num_block=1, tile=0, device=device)
        self.call = _capi.lib().rtd_esrgan_upscale
        self.want = ref.to_bytes(ref.upscale_float(sd, self.crop, torch.float64, 0, 10))
        half = ref.to_bytes(ref.upscale_float(sd, self.crop, torch.float16, 0, 10).double())
        self.share = float((half != self.want).mean())

    def valid(self):
        buf, offsets, shapes = self.be.upscale([self.frame], [[self.RECT]])
        got = buf[:64 * 64 * 3].view(64, 64, 3).cpu().numpy()
        d = np.abs(got.astype(np.int16) - self.want.astype(np.int16))
        share = float((d != 0).mean())
        print(f"esrgan 16x16: worst byte {int(d.max())}, differing bytes {share:.2e} (fp16 on the same crop {self.share:.2e})")
        assert shapes == [(64, 64)] and d.max() <= 1 and share <= self.share
        return got.tobytes()


class EngineRound:
    """the fp32 engine on t_tiny_160 (the smallest case there is: its two 160 x 160 frames in one call, as the parity test runs it),
    held to everything tests/test_gpu_parity.py::test_fp32_engine_matches_oracle_and_golden asks of that case"""

    def __init__(self, device):
        from tests import test_gpu_parity as parity
        self.parity = parity
        self.case = c = parity.fp32_case("t_tiny_160")
        self.be = parity.make_engine(c["arch"], c["w"], c["frames"], c["input_size"], "fp32")

    def valid(self):
        return b"".join(a.tobytes() for a in self.parity.check_fp32_engine(self.be, self.case))

    def refused(self):
        """one frame more than max_batch; the refusal is counted on the handle"""
        be = self.be
        n, ptrs, hw, keep = be._frame_args((self.case["frames"] * 2)[:be.max_batch + 1], False)
        assert n == be.max_batch + 1
        out = np.zeros(n * be.num_queries * 4, np.float32)
        rc = be._L.rtd_infer_raw(be._h, n, ptrs, hw, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data)
        st = be.stats()
        assert st["failed_calls"] == 1 and st["last_error_code"] == _capi.RTD_E_INVALID, st
        return rc

    def missing_device(self, device):
        """the engine meets its device in rtd_load_weights: the constructor raises and leaves no open handle"""
        from telescope_cam_detection_amd.weights import fold_weights, pack_blob
        c = self.case
        eng = _capi.Engine.__new__(_capi.Engine)
        with pytest.raises(_capi.RtdError, match="no such device") as ei:
            eng.__init__(c["arch"], pack_blob(fold_weights(c["arch"], c["w"])), device=device, precision=_capi.PREC_FP32, max_batch=len(c["frames"]),
                         input_size=c["input_size"], use_graph=False)
        assert ei.value.code == _capi.RTD_E_INVALID and not eng._h.value


ROUNDS = {"motion": MotionRound, "mog2": Mog2Round, "jpeg": JpegRound, "overlay": OverlayRound, "enhance": EnhanceRound, "esrgan": EsrganRound,
          "engine": EngineRound}


@pytest.mark.gpu
@pytest.mark.parametrize("name", HANDLES)
def test_create_call_refused_call_call_close(name):
    import torch
    if name != "engine":
        rc, h = raw_create(name, torch.cuda.device_count())
        assert rc == _capi.RTD_E_INVALID and h is None and b"no such device" in create_error(name)
    r = ROUNDS[name](0)
    try:
        be = r.be
        assert be._h.value
        if name == "engine":
            r.missing_device(torch.cuda.device_count())
        if name in ("motion", "mog2", "jpeg", "overlay", "engine"):
            be.wait_stream(0)                               # (raises unless RTD_OK)
        first = r.valid()
        assert r.refused() == _capi.RTD_E_INVALID
        assert len(be._fn("last_error")(be._h) or b"") > 0
        assert r.valid() == first
    finally:
        r.be.close()
    assert not r.be._h.value
