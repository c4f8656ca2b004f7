"""Host side of the Real-ESRGAN upscaler: the restatement's own flow (tests/esrgan_ref.py), the checkpoint key rule, the library's
layout arithmetic and its refusals that need no device, `UpscalingEnhancer.from_reference`, the recorded yardstick and the export lists."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import esrgan_ref as ref
from telescope_cam_detection_amd import _capi, enhance, esrgan
from telescope_cam_detection_amd.weights import unpack_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK = os.path.join(ROOT, "tests", "golden", "esrgan_yardstick.json")


@pytest.fixture(scope="module")
def b1():
    return ref.synth_state(1, 0)


def test_tile_flow_equals_a_hand_written_loop(b1):
    crop = ref.random_crop(40, 33, 4)
    got = ref.upscale_float(b1, crop, torch.float64, tile=16, tile_pad=4)
    x = ref.ingest(crop, torch.float64)
    want = torch.zeros_like(got)
    tiles = 0
    with torch.no_grad():
        for y0 in (0, 16, 32):
            for x0 in (0, 16, 32):
                y1, x1 = min(y0 + 16, 40), min(x0 + 16, 33)
                iy0, iy1, ix0, ix1 = max(y0 - 4, 0), min(y1 + 4, 40), max(x0 - 4, 0), min(x1 + 4, 33)
                o = ref.rrdbnet(b1, x[:, :, iy0:iy1, ix0:ix1])[0]
                want[:, 4 * y0:4 * y1, 4 * x0:4 * x1] = o[:, 4 * (y0 - iy0):4 * (y0 - iy0) + 4 * (y1 - y0), 4 * (x0 - ix0):4 * (x0 - ix0) + 4 * (x1 - x0)]
                tiles += 1
    assert tiles == 9 and len(ref.tile_list(40, 33, 16, 4)) == 9
    assert torch.equal(got, want)
    one = ref.upscale_float(b1, crop, torch.float64, tile=0)
    assert not torch.equal(got, one)                              # a 4-pixel pad does not cover the receptive field: the tiles are visible
    assert ((got - one).abs().max()) < 0.05


def test_a_tile_that_holds_the_crop_is_the_one_pass_flow(b1):
    crop = ref.random_crop(19, 27, 3)
    one = ref.upscale_float(b1, crop, torch.float64, tile=0)
    assert torch.equal(ref.upscale_float(b1, crop, torch.float64, tile=27, tile_pad=10), one)
    assert torch.equal(ref.upscale_float(b1, crop, torch.float64, tile=512, tile_pad=0), one)
    assert one.shape == (3, 76, 108)
    b = ref.to_bytes(one)
    assert b.shape == (76, 108, 3) and b.dtype == np.uint8
    assert 0 < one.min() and one.max() < 1


def test_ingest_and_rounding_rules():
    crop = np.arange(8 * 8 * 3, dtype=np.uint8).reshape(8, 8, 3)
    x = ref.ingest(crop, torch.float32)
    assert x.shape == (1, 3, 8, 8) and x[0, 0, 0, 0] == np.float32(2) / np.float32(255) and x[0, 2, 0, 1] == np.float32(3) / np.float32(255)
    f = torch.tensor([0.4 / 255, 1.6 / 255, 2.4 / 255, -1.0, 2.0, 0.999]).double().view(1, 2, 3).repeat(3, 1, 1)
    b = ref.to_bytes(f)
    assert b[..., 0].tolist() == [[0, 2, 2], [0, 255, 255]]     # rounded to nearest, clamped
    assert ref.to_bytes(torch.full((3, 1, 1), 0.5).double())[0, 0, 0] == 128 and ref.to_bytes(torch.full((3, 1, 1), 0.1).double())[0, 0, 0] == 26   # 127.5 -> 128 (even), 25.5 -> 26 (even)


def test_key_rule_and_load_state_errors(b1):
    other = {k: v + 1 for k, v in b1.items()}
    blob = esrgan.load_state({"params": other, "params_ema": b1})
    got = unpack_blob(blob)
    assert set(got) == set(b1) and all(np.array_equal(got[k], b1[k].numpy()) for k in b1)
    assert np.array_equal(unpack_blob(esrgan.load_state({"params": other}))["conv_hr.bias"], other["conv_hr.bias"].numpy())
    assert np.array_equal(unpack_blob(esrgan.load_state(b1))["conv_hr.bias"], b1["conv_hr.bias"].numpy())       # a bare state dict
    assert esrgan.num_blocks_of(b1) == 1 and esrgan.num_blocks_of(ref.synth_state(2)) == 2
    assert [n for n, _, _ in esrgan.conv_table(2)] == [n for n, _, _ in ref.conv_names(2)] and len(esrgan.conv_table(23)) == 351
    missing = dict(b1)
    del missing["body.0.rdb2.conv3.bias"]
    bad_shape = dict(b1, **{"conv_up1.weight": b1["conv_up1.weight"][:, :32]})
    for sd, name in ((missing, "body.0.rdb2.conv3.bias"), (bad_shape, "conv_up1.weight"), ({}, "body.0.rdb1.conv1.weight")):
        with pytest.raises(_capi.RtdError) as ei:
            esrgan.load_state(sd)
        assert ei.value.code == _capi.RTD_E_WEIGHTS and name in str(ei.value)
    with pytest.raises(_capi.RtdError) as ei:
        esrgan.load_state(b1, num_block=2)                         # asked for more blocks than the file holds
    assert ei.value.code == _capi.RTD_E_WEIGHTS and "body.1.rdb1.conv1.weight" in str(ei.value)


def test_a_checkpoint_file_loads_by_the_key_rule(tmp_path, b1):
    path = tmp_path / "x4.pth"
    torch.save({"params_ema": b1, "params": {k: v * 0 for k, v in b1.items()}}, path)
    assert esrgan.load_state(path) == esrgan.load_state(b1)


def test_layout_is_host_code_of_the_library():
    rects = [(0, 0, 8, 8), (5, 7, 45, 40), (3, 3, 134, 73), (0, 0, 1080, 640)]
    off = esrgan.layout(rects)
    assert len(off) == len(rects) + 1 and off[0] == 0 and all(o % 256 == 0 for o in off)
    sizes = [3 * 16 * (r[2] - r[0]) * (r[3] - r[1]) for r in rects]
    for i, s in enumerate(sizes):
        assert 0 <= off[i + 1] - off[i] - s < 256                   # tight rows, padded to the next multiple of 256
    assert esrgan.layout([]) == [0]
    assert esrgan.layout(rects[1:3])[1] == off[2] - off[1]
    assert esrgan.layout([(0, 0, 4096, 4096)])[1] == 16384 * 16384 * 3
    for bad in ((0, 0, 7, 16), (0, 0, 16, 7), (-1, 0, 20, 20), (10, 10, 5, 40), (0, 0, 4097, 8)):
        with pytest.raises(_capi.RtdError) as ei:
            esrgan.layout([rects[0], bad])
        assert ei.value.code == _capi.RTD_E_INVALID
    offsets = np.zeros(2, np.int64) - 7
    rc = (C.c_int32 * 4)(0, 0, 7, 16)
    assert _capi.lib().rtd_esrgan_layout(1, rc, offsets.ctypes.data_as(C.POINTER(C.c_int64))) == _capi.RTD_E_INVALID


def test_create_refuses_bad_configs_and_blobs_before_it_needs_a_device(b1):
    blob = esrgan.load_state(b1)

    def create(blob=blob, **kw):
        args = dict(num_block=1, precision="f16x3", tile=512, tile_pad=10)
        args.update(kw)
        with pytest.raises(_capi.RtdError) as ei:
            esrgan.CropUpscaler(blob, **args)
        return ei.value

    for kw in (dict(precision="bf16"), dict(tile=8), dict(tile=513), dict(tile_pad=33), dict(tile_pad=-1), dict(num_block=0), dict(num_block=33)):
        assert create(**kw).code == _capi.RTD_E_INVALID, kw
    assert "bf16" in str(create(precision="bf16"))
    e = create(num_block=2)
    assert e.code == _capi.RTD_E_WEIGHTS and "body.1.rdb1.conv1.weight" in str(e)
    assert create(blob=blob[:100]).code == _capi.RTD_E_WEIGHTS
    assert create(blob=b"XXXX" + blob[4:]).code == _capi.RTD_E_WEIGHTS
    for value, prec, what in ((float("nan"), "fp32", "NaN"), (float("inf"), "f16x3", "NaN"), (70000.0, "f16x3", "65504")):
        sd = dict(b1, **{"body.0.rdb3.conv2.weight": b1["body.0.rdb3.conv2.weight"].clone()})
        sd["body.0.rdb3.conv2.weight"][3, 5, 1, 1] = value
        e = create(blob=esrgan.load_state(sd), precision=prec)
        assert e.code == _capi.RTD_E_WEIGHTS and "body.0.rdb3.conv2.weight" in str(e) and what in str(e), (value, str(e))


def fake_image_enhancer(path, method="realesrgan", scale=4, grid=(8, 8), d=9, sigma_space=75):
    return types.SimpleNamespace(method=method, realesrgan_model_path=path, realesrgan_scale=scale, realesrgan_tile=512, realesrgan_tile_pad=10,
                                 clahe_clip_limit=2.0, clahe_tile_grid_size=grid, bilateral_d=d, bilateral_sigma_color=75, bilateral_sigma_space=sigma_space)


def test_from_reference_refuses_what_the_library_cannot_stand_in_for(tmp_path, b1):
    path = str(tmp_path / "x4.pth")
    torch.save({"params_ema": b1}, path)
    UE = esrgan.UpscalingEnhancer
    assert UE.from_reference(None, 64) is None
    assert UE.from_reference(fake_image_enhancer(path, method="clahe"), 64) is None
    assert UE.from_reference(fake_image_enhancer(path, method="none"), 64) is None
    assert UE.from_reference(fake_image_enhancer(path, scale=2), 64) is None
    assert UE.from_reference(fake_image_enhancer(None), 64) is None
    assert UE.from_reference(fake_image_enhancer(str(tmp_path / "absent.pth")), 64) is None
    assert UE.from_reference(fake_image_enhancer(path, grid=(32, 32)), 64) is None
    assert UE.from_reference(fake_image_enhancer(path, d=17), 64) is None
    assert UE.from_reference(fake_image_enhancer(path), 8) is None
    # ... and the existing entry points stay as they were for this method
    assert enhance.CropEnhancer.from_reference(fake_image_enhancer(path), 64) is None


def test_the_yardstick_file_reproduces():
    rec = json.load(open(YARDSTICK))["cases"]
    assert set(rec) == set(ref.CASES)
    for name, c in ref.CASES.items():
        for k, v in c.items():
            assert rec[name][k] == v, (name, k)
        lo, hi = rec[name]["range"]
        assert 0 < lo < hi < 1, name                                 # no clamped value: clamping cannot hide an error
        assert rec[name]["fp32"]["max_abs"] < 1e-6 < rec[name]["fp16"]["max_abs"] < 2e-3 and rec[name]["fp16"]["worst_byte"] == 1
    assert set(rec[ref.STAGE_CASE]["fp16"]["stages"]) == set(ref.stage_names(1))
    for name in ("b2_19x27", ref.STAGE_CASE):                     # the small cases are recomputed; the 23-block fp16 run takes most of a minute
        got = ref.measure_case(name)
        assert got["range"] == pytest.approx(rec[name]["range"], rel=1e-9)
        for key in ("fp32", "fp16"):
            # the fp64 run is deterministic; a low-precision run may sum in another order on another CPU: a factor of 1.5
            assert rec[name][key]["max_abs"] / 1.5 <= got[key]["max_abs"] <= rec[name][key]["max_abs"] * 1.5, (name, key, got[key], rec[name][key])
        assert got["fp16"]["byte_share"] == pytest.approx(rec[name]["fp16"]["byte_share"], rel=0.5)


def test_export_lists_match_the_headers():
    lib = _capi.lib()
    for fname, exports in (("rtdetr_mi355.h", _capi.EXPORTS), ("rtdetr_mi355_test.h", _capi.TEST_EXPORTS)):
        code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", fname)).read(), flags=re.S)
        declared = set(re.findall(r"\b(rtd_[a-z0-9_]+)\s*\(", code)) - {"rtd_engine"}
        assert declared == set(exports), (fname, declared ^ set(exports))
    for sym in ("rtd_esrgan_create", "rtd_esrgan_layout", "rtd_esrgan_upscale", "rtd_esrgan_arena_bytes", "rtd_esrgan_last_error", "rtd_esrgan_destroy"):
        assert sym in _capi.EXPORTS and hasattr(lib, sym)
    for sym in ("rtd_debug_esrgan_tensor", "rtd_op_conv_view", "rtd_bench_conv_act"):
        assert sym in _capi.TEST_EXPORTS and hasattr(lib, sym)
    assert _capi.ACT["lrelu"] == 4


def test_matches_realesrgan_where_it_is_installed(b1, tmp_path):
    pytest.importorskip("realesrgan")
    pytest.importorskip("basicsr")
    from basicsr.archs.rrdbnet_arch import RRDBNet
    from realesrgan import RealESRGANer

    path = str(tmp_path / "x4.pth")
    torch.save({"params_ema": b1}, path)
    model = RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=1, num_grow_ch=32, scale=4)
    assert [k for k, _ in model.named_parameters()] == list(b1)
    crop = ref.random_crop(40, 33, 4)
    for tile, pad in ((0, 10), (16, 4)):
        up = RealESRGANer(scale=4, model_path=path, model=model, tile=tile, tile_pad=pad, pre_pad=0, half=False, device="cpu")
        out, _ = up.enhance(crop, outscale=4)
        want = ref.enhance(b1, crop, torch.float32, tile, pad)
        assert np.abs(out.astype(np.int16) - want.astype(np.int16)).max() <= 1 and (out != want).mean() < 1e-3
