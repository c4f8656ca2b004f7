"""The Real-ESRGAN x4 upscaler on the MI355X (csrc/esrgan.hip) against the fp64 restatement (tests/esrgan_ref.py).

Gates, for the f16x3 and the fp32 engine alike, from tests/golden/esrgan_yardstick.json (what plain fp16 - the reference's own
`realesrgan_half=True` mode - costs against fp64 on the same case):
  1. float output: max |delta| <= one quarter of the recorded fp16 error of the case (of the stage, for the stage-by-stage test);
  2. bytes: no byte off by more than 1, and the share of differing bytes <= the recorded fp16 share of the case.
The shapes are the smallest at which each path can go wrong: 19 x 27 (odd, not a tile multiple, tile kernels), 128 x 128 (the direct
64 -> 64 pair kernel takes the layer), 40 x 33 with tile 16 / pad 4 (3 x 3 ragged tiles with interior and edge pads)."""
import ctypes as C
import json
import os
import types
from collections import deque

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import enhance_ref
from tests import esrgan_ref as ref
from tests.standins import StandInPipeline
from telescope_cam_detection_amd import _capi, enhance, esrgan
from telescope_cam_detection_amd.stage2 import BatchedStage2, CropBatcher, crop_rect, format_predictions, normalised_bbox

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARD = json.load(open(os.path.join(ROOT, "tests", "golden", "esrgan_yardstick.json")))["cases"]
ENGINES = ("f16x3", "fp32")

_REF, _UP = {}, {}


def reference(name):
    """the fp64 restatement of a yardstick case, computed once: (state, crop, float output [4h, 4w, 3] RGB, bytes, stages of the last tile)"""
    if name not in _REF:
        sd, crop, tile, pad = ref.case_inputs(name)
        st = {}
        out = ref.upscale_float(sd, crop, torch.float64, tile, pad, st)
        assert 0 < float(out.min()) and float(out.max()) < 1, "the restatement's own output must hold no clamped value"
        _REF[name] = (sd, crop, out.permute(1, 2, 0).numpy(), ref.to_bytes(out), {k: v.numpy() for k, v in st.items()})
    return _REF[name]


def upscaler(num_block, precision, tile=0, tile_pad=10, sd=None, key=None):
    k = (num_block, precision, tile, tile_pad, key)
    if k not in _UP:
        _UP[k] = esrgan.CropUpscaler(sd if sd is not None else ref.synth_state(num_block, 0), num_block=num_block, precision=precision, tile=tile,
                                     tile_pad=tile_pad)
    return _UP[k]


@pytest.fixture(scope="module", autouse=True)
def _close_upscalers():
    yield
    for u in _UP.values():
        u.close()
    _UP.clear()
    _capi.debug_option("reset", 0)


def crop_bytes(buf, offsets, shapes, i):
    h, w = shapes[i]
    return buf[offsets[i]:offsets[i] + h * w * 3].view(h, w, 3).cpu().numpy()


def gate2(got, want, share, what):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    s = float((d != 0).mean())
    print(f"{what}: worst byte {int(d.max())}, differing bytes {s:.2e} (fp16 yardstick {share:.2e})")
    assert d.max() <= 1 and s <= share, (what, int(d.max()), s, share)


def gate1(got, want, fp16_err, what):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: max |delta| {err:.3e} (gate {fp16_err / 4:.3e} = fp16 yardstick {fp16_err:.3e} / 4)")
    assert np.isfinite(got).all() and err <= fp16_err / 4, (what, err, fp16_err / 4)
    return err


# ------------------------------------------------------------------------------------------------------------ LeakyReLU epilogue
def _quant(x, dtype):
    """the values the kernel sees for an fp32 array stored in `dtype`, and their device storage"""
    if dtype == _capi.DT_F32:
        return x, torch.from_numpy(x).cuda()
    if dtype == _capi.DT_BF16:
        q = torch.from_numpy(x).to(torch.bfloat16)
        return q.float().numpy(), q.cuda()
    s = _capi.to_split(x)
    return _capi.from_split(s), torch.from_numpy(s.view(np.int16)).cuda()


def _unquant(t, dtype):
    if dtype == _capi.DT_F32:
        return t.cpu().numpy()
    if dtype == _capi.DT_BF16:
        return t.float().cpu().numpy()
    return _capi.from_split(t.cpu().numpy().view(np.uint16))


# relative to max |y|, against fp64 on the values the kernel sees.  fp32: K <= 1728 products accumulated in fp32 (<= sqrt(K) 2^-24
# typical, K 2^-24 = 1e-4 worst) -> 2e-5, the bound tests/test_gpu_ops.py holds the pair kernels to; pairs: the same bound (2^-22 operands,
# the dropped lo * lo term, one hi + lo rounding of the output); bf16: the filter is rounded to bf16 by the library (2^-9 relative per
# weight, random signs: 2^-9 / sqrt(K) of the sum's scale) and the output is rounded to bf16 once (2^-9 of |y|) -> 2^-8.
CONV_TOL = {_capi.DT_F32: 2e-5, _capi.DT_F16X2: 2e-5, _capi.DT_BF16: 2.0 ** -8}
# (dtype -> dispatch variants): every conv family launch_conv can choose for these shapes
# ("ws": the LDS-DMA tile kernel; bf16 takes it at any size through its two options, fp32 from 512 tiles on - the 256 x 256 case)
VARIANTS = {_capi.DT_F32: ("auto", "reg"), _capi.DT_BF16: ("auto", "reg", "ws"), _capi.DT_F16X2: ("auto", "tiled", "tiled2")}


def _set_variant(v):
    _capi.debug_option("reset", 0)
    if v == "reg":
        _capi.debug_option("conv_mode", 1)                     # the register-staged tile kernel only
    elif v == "ws":
        _capi.debug_option("glds_min_blocks", 1)
        _capi.debug_option("glds_min_n", 64)
    elif v in ("tiled", "tiled2"):                              # fixed tiles only (no direct 3x3 / flexible kernels): 4-stage, then 2-stage
        _capi.debug_option("split_flex", 0)
        _capi.debug_option("split_wsq", 0)
        _capi.debug_option("conv_reg", 0)
        _capi.debug_option("split_ws2_min_blocks", (1 << 30) if v == "tiled" else 1)


LRELU_CASES = {
    # name: (H, W, buffer channels, Cin (prefix), Cout, output channel offset (None: a second buffer), residual)
    "96to32_slice_19x27": (19, 27, 192, 96, 32, 96, False),
    "192to64_res_19x27": (19, 27, 192, 192, 64, None, True),
    "64to64_128x128": (128, 128, 64, 64, 64, None, False),
    "64to64_res_40x40": (40, 40, 64, 64, 64, None, True),
    "64to64_256x256": (256, 256, 64, 64, 64, None, False),       # fp32 only: the smallest map its LDS-DMA tile kernel takes (512 tiles)
}
DTYPE_IDS = {_capi.DT_BF16: "bf16", _capi.DT_F32: "fp32", _capi.DT_F16X2: "f16x2"}
LRELU_PARAMS = [(c, d) for c in LRELU_CASES for d in DTYPE_IDS if c != "64to64_256x256" or d == _capi.DT_F32]


@pytest.mark.parametrize("case,dtype", LRELU_PARAMS, ids=[f"{c}-{DTYPE_IDS[d]}" for c, d in LRELU_PARAMS])
def test_lrelu_epilogue_on_views(case, dtype):
    H, W, CB, Cin, Cout, c_off, with_res = LRELU_CASES[case]
    L = _capi.lib()
    g = torch.Generator().manual_seed(100 + list(LRELU_CASES).index(case))
    x = torch.randn(1, H, W, CB, generator=g).numpy()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / (Cin * 9)) ** 0.5)
    b = (torch.randn(Cout, generator=g) * 0.1)
    es = 2 if dtype == _capi.DT_BF16 else 4                    # bytes per channel of a view's pointer arithmetic
    xq, xd = _quant(x, dtype)
    wq = w if dtype == _capi.DT_F32 else torch.from_numpy(_quant(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().numpy(), dtype)[0]).reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    xin = torch.from_numpy(xq[..., :Cin]).permute(0, 3, 1, 2).double()
    y = F.conv2d(xin, wq.double(), b.double(), padding=1)
    if with_res:
        y = y + torch.from_numpy(xq[..., :Cout]).permute(0, 3, 1, 2).double()       # RES_PRE: the block input, added before the activation
    y = F.leaky_relu(y, 0.2)
    assert (y > 0).any() and (y < 0).any()
    y = y.permute(0, 2, 3, 1).numpy()
    wd = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().cuda()
    bd = b.cuda()
    for variant in (("auto",) if case == "64to64_256x256" else VARIANTS[dtype]):
        _set_variant(variant)
        try:
            if c_off is None:
                CY = 192 if CB == 192 else Cout
                _, yd = _quant(np.full((1, H, W, CY), 7.0, np.float32), dtype)
                ybase, ldy = yd.data_ptr(), CY
            else:
                xd = _quant(x, dtype)[1]
                yd, ybase, ldy = xd, xd.data_ptr() + c_off * es, CB
            rc = L.rtd_op_conv_view(dtype, xd.data_ptr(), CB, wd.data_ptr(), bd.data_ptr(), xd.data_ptr() if with_res else None, CB, ybase, ldy,
                                    1, H, W, Cin, Cout, 3, 1, 1, _capi.ACT["lrelu"], 1 if with_res else 0)
            assert rc == _capi.RTD_OK, (L.rtd_last_error(None) or b"").decode()
        finally:
            _capi.debug_option("reset", 0)
        full = _unquant(yd, dtype)
        o = 0 if c_off is None else c_off
        got = full[..., o:o + Cout]
        err = float(np.abs(got - y).max() / np.abs(y).max())
        print(f"lrelu {case} dtype {dtype} {variant}: max err / max |y| {err:.2e}")
        assert np.isfinite(got).all() and err <= CONV_TOL[dtype], (case, dtype, variant, err)
        keep = np.ones(full.shape[-1], bool)
        keep[o:o + Cout] = False                                  # a slice is written and nothing beside it
        assert np.array_equal(full[..., keep], (xq if c_off is not None else np.full_like(full, 7.0))[..., keep]), (case, dtype, variant)


def test_plain_conv_entry_point_takes_act_4():
    L = _capi.lib()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 12, 12, 32, generator=g)
    w = torch.randn(32, 32, 3, 3, generator=g) * 0.06
    b = torch.randn(32, generator=g) * 0.1
    y = F.leaky_relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1), 0.2).permute(0, 2, 3, 1)
    yd = torch.zeros(1, 12, 12, 32, device="cuda")
    xd, wd, bd = x.cuda(), w.permute(0, 2, 3, 1).reshape(32, -1).contiguous().cuda(), b.cuda()
    rc = L.rtd_op_conv(_capi.DT_F32, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, yd.data_ptr(), 1, 12, 12, 32, 32, 3, 3, 1, 1, 4, 0, 1)
    assert rc == _capi.RTD_OK
    assert (y < 0).any() and float((yd.cpu().double() - y).abs().max() / y.abs().max()) <= 2e-5


# ------------------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("engine", ENGINES)
def test_stage_by_stage(engine):
    name = ref.STAGE_CASE
    sd, crop, out, want_bytes, stages = reference(name)
    up = upscaler(1, engine)
    frame = torch.from_numpy(crop).cuda()
    buf, offsets, shapes = up.upscale([frame], [[(0, 0, crop.shape[1], crop.shape[0])]])
    got = up.debug_tensor("ingest")
    want = ref.ingest(crop, torch.float32)[0].permute(1, 2, 0).numpy()          # float32(v) / 255, RGB
    if engine == "f16x3":                                          # ... in the trunk's storage type: the hi + lo pair nearest to it
        padded = np.zeros(want.shape[:2] + (32,), np.float32)
        padded[..., :3] = want
        want = _capi.from_split(_capi.to_split(padded))[..., :3]
    assert got.shape == (19, 27, 32) and np.array_equal(got[..., :3], want) and not got[..., 3:].any()
    rec = YARD[name]["fp16"]["stages"]
    for st in ref.stage_names(1):
        g = up.debug_tensor(st)
        w = stages[st]
        assert g.shape[:2] == w.shape[:2] and g.shape[2] in (w.shape[2], 32), (st, g.shape, w.shape)
        gate1(g[..., :w.shape[2]], w, rec[st], f"{engine} stage {st}")
    gate2(crop_bytes(buf, offsets, shapes, 0), want_bytes, YARD[name]["fp16"]["byte_share"], f"{engine} {name} bytes")
    with pytest.raises(_capi.RtdError):
        up.debug_tensor("body.1")


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["b2_19x27", "b23_32x32"])
def test_whole_network(name, engine):
    sd, crop, out, want_bytes, _ = reference(name)
    up = upscaler(ref.CASES[name]["num_block"], engine)
    h, w = crop.shape[:2]
    frame = torch.from_numpy(crop).cuda()
    buf, offsets, shapes = up.upscale([frame], [[(0, 0, w, h)]])
    assert shapes == [(4 * h, 4 * w)] and offsets == [0, (4 * h * 4 * w * 3 + 255) // 256 * 256]
    gate2(crop_bytes(buf, offsets, shapes, 0), want_bytes, YARD[name]["fp16"]["byte_share"], f"{engine} {name} bytes")
    last = up.debug_tensor("last")
    assert last.shape == (4 * h, 4 * w, 32) and not last[..., 3:].any()
    gate1(last[..., :3], out, YARD[name]["fp16"]["max_abs"], f"{engine} {name} float output")
    assert up.last_call_ms() > 0


@pytest.mark.parametrize("engine", ENGINES)
def test_tiles(engine):
    name = "b1_40x33_t16p4"
    sd, crop, out, want_bytes, _ = reference(name)
    share = YARD[name]["fp16"]["byte_share"]
    frame = torch.from_numpy(crop).cuda()
    rect = [[(0, 0, 33, 40)]]
    up = upscaler(1, engine, tile=16, tile_pad=4)
    buf, offsets, shapes = up.upscale([frame], rect)
    tiled = crop_bytes(buf, offsets, shapes, 0)
    gate2(tiled, want_bytes, share, f"{engine} 3 x 3 tiles")
    last = up.debug_tensor("last")                                  # the last tile: core 8 x 1, input 12 x 5
    assert last.shape == (4 * 12, 4 * 5, 32)
    gate1(last[..., :3], reference(name)[4]["last"], YARD[name]["fp16"]["max_abs"], f"{engine} last tile, float output")
    one_pass = ref.to_bytes(ref.upscale_float(sd, crop, torch.float64, 0))
    buf0, off0, shp0 = upscaler(1, engine, tile=0).upscale([frame], rect)
    whole = crop_bytes(buf0, off0, shp0, 0)
    gate2(whole, one_pass, share, f"{engine} tile 0")
    bufb, offb, shpb = upscaler(1, engine, tile=64, tile_pad=10).upscale([frame], rect)
    assert np.array_equal(crop_bytes(bufb, offb, shpb, 0), whole)   # a tile that holds the crop is the one-pass flow, bit for bit


def raw_call(up, frames, rects, out, out_cap=None, n=None):
    k = len(rects)
    ptrs = (C.c_void_p * max(k, 1))(*[f.data_ptr() for f in frames])
    hw = (C.c_int32 * max(2 * k, 1))(*[int(v) for f in frames for v in f.shape[:2]])
    rc = (C.c_int32 * max(4 * k, 1))(*[int(v) for r in rects for v in r])
    return _capi.lib().rtd_esrgan_upscale(up._h, k if n is None else n, ptrs, hw, rc, C.c_void_p(out.data_ptr()), out.numel() if out_cap is None else out_cap,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("engine", ENGINES)
def test_geometry_three_crops_of_two_frames(engine):
    a, b = "b1_19x27", "b1_24x20"
    crop_a, bytes_a = reference(a)[1], reference(a)[3]
    crop_b, bytes_b = reference(b)[1], reference(b)[3]
    big = ref.random_crop(60, 70, 77)                               # a noise frame: a read outside the rectangle shows
    big[7:7 + 19, 5:5 + 27] = crop_a
    big[30:30 + 24, 40:40 + 20] = crop_b
    frames = [torch.from_numpy(big).cuda(), torch.from_numpy(crop_b).cuda()]
    rects = [(5, 7, 32, 26), (40, 30, 60, 54), (0, 0, 20, 24)]       # at an offset, at another, and a crop that is its whole frame
    offsets = esrgan.layout(rects)
    sizes = [76 * 108 * 3, 96 * 80 * 3, 96 * 80 * 3]
    assert any(o + s < n for o, s, n in zip(offsets, sizes, offsets[1:]))     # there are bytes between the crops
    out = torch.full((offsets[-1] + 512,), 0xAB, dtype=torch.uint8, device="cuda")
    up = upscaler(1, engine)
    assert raw_call(up, [frames[0], frames[0], frames[1]], rects, out) == _capi.RTD_OK
    torch.cuda.synchronize()
    arena = up.arena_bytes()
    assert arena > 0
    o = out.cpu().numpy()
    for i, (want, case) in enumerate(((bytes_a, a), (bytes_b, b), (bytes_b, b))):
        got = o[offsets[i]:offsets[i] + sizes[i]].reshape(want.shape)
        gate2(got, want, YARD[case]["fp16"]["byte_share"], f"{engine} crop {i}")
        assert (o[offsets[i] + sizes[i]:offsets[i + 1]] == 0xAB).all(), i
    assert (o[offsets[-1]:] == 0xAB).all()
    first = o.copy()
    out.fill_(0xAB)
    assert raw_call(up, [frames[0], frames[0], frames[1]], rects, out) == _capi.RTD_OK       # the same shapes again: nothing is allocated
    torch.cuda.synchronize()
    assert up.arena_bytes() == arena and np.array_equal(out.cpu().numpy(), first)
    assert (frames[0].cpu().numpy() == big).all()                   # the frames are only read


def test_clamp_path():
    name = "b1_24x20"
    sd, crop = reference(name)[:2]
    sd = dict(sd)
    sd["conv_last.bias"] = sd["conv_last.bias"] + torch.tensor([0.6, -0.6, 0.0])     # R clamps at 1, G at 0, B stays inside
    want_f = ref.upscale_float(sd, crop, torch.float64, 0)
    assert float(want_f[0].min()) > 1 and float(want_f[1].max()) < 0
    want = ref.to_bytes(want_f)
    for engine in ENGINES:
        up = upscaler(1, engine, sd=sd, key="clamp")
        buf, offsets, shapes = up.upscale([torch.from_numpy(crop).cuda()], [[(0, 0, 20, 24)]])
        got = crop_bytes(buf, offsets, shapes, 0)
        assert (got[..., 2] == 255).all() and (got[..., 1] == 0).all() and 0 < got[..., 0].min() and got[..., 0].max() < 255
        gate2(got, want, YARD[name]["fp16"]["byte_share"], f"{engine} clamped")


def test_limits_are_refused_and_leave_the_output_untouched():
    up = upscaler(1, "f16x3")
    frame = torch.from_numpy(ref.random_crop(40, 50, 9)).cuda()
    wide = torch.from_numpy(ref.random_crop(8, 600, 10)).cuda()
    out = torch.full((1 << 20,), 0xAB, dtype=torch.uint8, device="cuda")
    good = (4, 4, 20, 16)
    need = esrgan.layout([good])[-1]
    cases = {"7 px wide": (frame, [(0, 0, 7, 30)]), "7 px high": (frame, [(0, 0, 30, 7)]), "right of its frame": (frame, [(30, 0, 51, 30)]),
             "below its frame": (frame, [(0, 20, 30, 41)]), "negative corner": (frame, [(-1, 0, 30, 30)]), "second crop bad": (frame, [good, (0, 0, 7, 30)]),
             "tile 0 with a 600-pixel side": (wide, [(0, 0, 600, 8)])}
    for what, (f, rects) in cases.items():
        assert raw_call(up, [f] * len(rects), rects, out) == _capi.RTD_E_INVALID, what
        assert _capi.lib().rtd_esrgan_last_error(up._h)
    assert raw_call(up, [frame], [good], out, out_cap=need - 1) == _capi.RTD_E_INVALID
    assert raw_call(up, [frame], [good], out, n=0) == _capi.RTD_E_INVALID
    assert raw_call(up, [frame] * 65, [good] * 65, out) == _capi.RTD_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    tiled = upscaler(1, "f16x3", tile=512, tile_pad=10)
    assert raw_call(tiled, [wide], [(0, 0, 600, 8)], out) == _capi.RTD_OK               # with tiles a 600-pixel side is fine (2 tiles)
    torch.cuda.synchronize()
    assert not bool((out[:32 * 2400 * 3] == 0xAB).all())
    blob = esrgan.load_state(ref.synth_state(1, 0))
    for bad in (dict(precision="bf16"), dict(tile=8), dict(tile_pad=33)):
        with pytest.raises(_capi.RtdError) as ei:
            esrgan.CropUpscaler(blob, num_block=1, **bad)
        assert ei.value.code == _capi.RTD_E_INVALID, bad


def test_stream_order_needs_no_synchronisation():
    up = upscaler(1, "f16x3")
    base = torch.from_numpy(np.random.default_rng(80).integers(0, 200, (40, 50, 3), dtype=np.uint8)).cuda()
    rects = [[(3, 5, 30, 24)]]
    buf, offsets, shapes = up.upscale([base + 37], rects)
    want = buf.to(torch.int32).sum()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    frame = torch.zeros_like(base)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(37):                                          # the producer: the frame is complete only when the stream has run all of it
            frame += 1
        frame += base
        buf2, _, _ = up.upscale([frame], rects)                      # rtd_esrgan_upscale follows on s ...
        got = buf2.to(torch.int32).sum()                             # ... and a torch op on its output follows it, no sync between
    s.synchronize()
    assert torch.equal(got, want) and torch.equal(buf2, buf)


# ------------------------------------------------------------------------------------------------------------ the chain
ENH = dict(clip_limit=2.0, tile_grid_size=(8, 8), bilateral_d=9, sigma_color=75, sigma_space=75)


@pytest.fixture(scope="module")
def chain():
    ue = esrgan.UpscalingEnhancer(upscaler(1, "f16x3", tile=512, tile_pad=10), enhance.CropEnhancer())
    yield ue
    ue.crop_enhancer.close()


def test_upscaling_enhancer_chain(chain):
    name = "b1_24x20"
    crop, want4 = reference(name)[1], reference(name)[3]
    big = ref.random_crop(50, 60, 5)
    big[10:34, 30:50] = crop
    buf, offsets, shapes = chain.enhance([torch.from_numpy(big).cuda()], [[(30, 10, 50, 34)]])
    assert shapes == [(96, 80)]
    up4 = crop_bytes(*chain.last_upscaled, 0)
    gate2(up4, want4, YARD[name]["fp16"]["byte_share"], "chain: the 4x image")
    final = crop_bytes(buf, offsets, shapes, 0)
    assert np.array_equal(final, enhance_ref.stages(up4, **ENH)["out"])            # the CLAHE + bilateral stage is bit-exact on the device's 4x bytes
    assert chain.last_call_ms() > 0


def test_batcher_with_the_chain_equals_the_batcher_on_reference_enhanced_images(chain):
    batcher = CropBatcher(input_size=96, min_crop_size=16)
    frames_np = [ref.random_crop(50, 60, 11), ref.random_crop(30, 34, 12)]
    rects = [[(2, 3, 30, 27), (35, 20, 59, 50)], [(0, 0, 34, 30)]]
    frames = [torch.from_numpy(f).cuda() for f in frames_np]
    got = batcher.preprocess_batch(frames, rects, enhancer=chain)
    up4 = [crop_bytes(*chain.last_upscaled, i) for i in range(3)]
    enhanced = [enhance_ref.stages(u, **ENH)["out"] for u in up4]
    want = batcher.preprocess_batch([torch.from_numpy(c).cuda() for c in enhanced], [[(0, 0, c.shape[1], c.shape[0])] for c in enhanced])
    assert got.shape == (3, 3, 96, 96) and torch.equal(got, want)
    assert not torch.equal(got, batcher.preprocess_batch(frames, rects))


def test_batched_stage2_with_the_chain_equals_a_per_detection_loop(chain):
    p = StandInPipeline(min_crop_size=16)
    p.enhancer = types.SimpleNamespace(method="realesrgan")
    p.enhancement_times = deque(maxlen=1000)
    p.process_detections = lambda *a: pytest.fail("the per-detection fallback ran")
    batcher = CropBatcher(input_size=96, min_crop_size=p.min_crop_size, crop_padding_percent=p.crop_padding_percent)
    assert BatchedStage2(p, batcher=batcher, enhancer="auto").enhancer is None      # "auto" stays as it was for this method
    s2 = BatchedStage2(p, batcher=batcher, enhancer=chain)
    rng = np.random.default_rng(90)
    frames_np = [rng.integers(0, 256, (80, 100, 3), dtype=np.uint8), rng.integers(0, 256, (60, 64, 3), dtype=np.uint8)]
    boxes = [[(14, 10.5, 12.2, 34.9, 40.0), (15, 50, 10, 90, 45), (14, 0, 0, 10, 10), (2, 20, 20, 60, 60)],
             [(21, 8, 9, 40, 44), (14, 30, 20, 63, 59.5)]]
    dets = [[{"class_id": c, "class_name": "x", "confidence": 0.9, "bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}} for c, x1, y1, x2, y2 in per]
            for per in boxes]
    want = [[dict(d, bbox=dict(d["bbox"])) for d in per] for per in dets]
    got = s2.process_batch([torch.from_numpy(f).cuda() for f in frames_np], dets)

    n_crops = 0
    for f, per in zip(frames_np, want):                               # one detection at a time: upscaled alone, enhanced on the CPU
        for d in per:
            d["bbox"] = normalised_bbox(d["bbox"])
            category = p.class_id_to_category.get(d["class_id"])
            if category not in p.species_classifiers:
                d["species"], d["species_confidence"] = None, 0.0
                continue
            rect = crop_rect(d["bbox"], f.shape[:2], p.min_crop_size, p.crop_padding_percent)
            if rect is None:
                s2._set(d, None, 0.0, category, None)
                continue
            x1, y1, x2, y2 = rect
            one = np.ascontiguousarray(f[y1:y2, x1:x2])
            b4 = chain.upscaler.upscale([torch.from_numpy(one).cuda()], [[(0, 0, x2 - x1, y2 - y1)]])
            crop = enhance_ref.stages(crop_bytes(*b4, 0), **ENH)["out"]
            x = s2.batcher.preprocess_batch([torch.from_numpy(crop).cuda()], [[(0, 0, crop.shape[1], crop.shape[0])]])
            clf = p.species_classifiers[category]
            with torch.no_grad():
                probs = torch.softmax(clf.model(x), dim=1).float().cpu()
            s2._conclude(d, category, format_predictions(clf, probs[0], 1))
            n_crops += 1
    assert n_crops >= 3 and len(p.enhancement_times) == n_crops and all(t > 0 for t in p.enhancement_times)
    for g_per, w_per in zip(got, want):
        assert len(g_per) == len(w_per)
        for g, w in zip(g_per, w_per):
            assert set(g) == set(w) and g["bbox"] == w["bbox"] and g["class_id"] == w["class_id"]
            for k in ("species", "taxonomic_level", "stage2_category"):
                assert g.get(k) == w.get(k), (k, g, w)
            # the same input bytes; a batched and a single-row forward of the fp32 stand-in net may sum in another order
            assert g["species_confidence"] == pytest.approx(w["species_confidence"], rel=1e-4, abs=1e-6)
