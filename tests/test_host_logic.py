"""CPU: host-side logic - load-time folding against the oracle, blob round trip, C-ABI export list,
the drop-in class's failure behaviour without a GPU, and the N>1 collate path on gloo (world_size 2)."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rtdetr_oracle as orc
from telescope_cam_detection_amd.arch import ARCHS, arch_from_config_path
from telescope_cam_detection_amd.weights import fold_weights, pack_blob, synth_weights, unpack_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_bn_and_repvgg_match_unfused_oracle():
    """what `.deploy()` does at load time (src/rtdetr_detector.py:164-165): conv+BN and RepVGG 3x3+1x1 folded."""
    arch = ARCHS["tiny"]
    w = synth_weights(arch, 3)
    f = fold_weights(arch, w)
    x = torch.randn(2, arch.enc_dim * 2, 12, 10)
    # CSP c12 = [c1 | c2] of the un-fused oracle
    ref1 = orc.conv_bn(w, "enc.fpn.0.c1", x, act="silu")
    ref2 = orc.conv_bn(w, "enc.fpn.0.c2", x, act="silu")
    got = F.silu(F.conv2d(x, f["enc.fpn.0.c12.w"].permute(0, 3, 1, 2), f["enc.fpn.0.c12.b"]))
    h = arch.csp_hidden
    torch.testing.assert_close(got[:, :h], ref1, atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(got[:, h:], ref2, atol=2e-5, rtol=1e-5)
    # RepVGG: 3x3 + 1x1 branches -> one 3x3
    y = torch.randn(2, h, 9, 7)
    ref = F.silu(orc.conv_bn(w, "enc.fpn.0.rep0.k3", y, padding=1) + orc.conv_bn(w, "enc.fpn.0.rep0.k1", y, padding=0))
    got = F.silu(F.conv2d(y, f["enc.fpn.0.rep0.w"].permute(0, 3, 1, 2), f["enc.fpn.0.rep0.b"], padding=1))
    torch.testing.assert_close(got, ref, atol=2e-5, rtol=1e-5)
    # stem conv: input channels padded 3 -> 8 with zeros
    assert f["backbone.stem.0.w"].shape[-1] == 8 and float(f["backbone.stem.0.w"][..., 3:].abs().max()) == 0.0
    # fused sibling GEMMs keep row order
    assert torch.equal(f["dec.l0.ca.offaw.w"][: w["dec.l0.ca.off.w"].shape[0]], w["dec.l0.ca.off.w"])
    assert torch.equal(f["dec.vp_all.w"][arch.d_model:2 * arch.d_model], w["dec.l1.ca.vp.w"])
    assert f["dec.qpos.0.w"].shape[1] == 8


def test_blob_roundtrip_and_alignment():
    arch = ARCHS["tinyb"]
    f = fold_weights(arch, synth_weights(arch, 5))
    blob = pack_blob(f)
    back = unpack_blob(blob)
    assert set(back) == set(f)
    for k, v in f.items():
        np.testing.assert_array_equal(back[k], v.numpy())
    with pytest.raises(AssertionError):
        unpack_blob(b"XXXX" + blob[4:])


def test_arch_from_config_path():
    assert arch_from_config_path("RT-DETR/rtdetrv2_pytorch/configs/rtdetrv2/rtdetrv2_r18vd_120e_coco.yml").name == "r18"
    assert arch_from_config_path("configs/rtdetrv2/rtdetrv2_r50vd_6x_coco.yml").name == "r50"
    assert arch_from_config_path("configs/rtdetrv2/rtdetrv2_r101vd_6x_coco.yml").name == "r101"
    with pytest.raises(ValueError):
        arch_from_config_path("yolox_s.py")
    assert ARCHS["r50"].level_shapes(640, 640) == [(80, 80), (40, 40), (20, 20)]
    assert ARCHS["r101"].level_shapes(1280, 1280) == [(160, 160), (80, 80), (40, 40)]


def test_library_loads_and_exports_every_declared_symbol():
    """no compute calls without a GPU: dlopen + symbol table only"""
    from telescope_cam_detection_amd import _capi
    lib = _capi.lib()
    for fname, exports in (("rtdetr_mi355.h", _capi.EXPORTS), ("rtdetr_mi355_test.h", _capi.TEST_EXPORTS)):
        header = open(os.path.join(ROOT, "include", fname)).read()
        code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)           # comments mention functions of the other header
        declared = set(re.findall(r"\b(rtd_[a-z0-9_]+)\s*\(", code))
        declared -= {"rtd_engine"}
        assert declared == set(exports), (fname, declared ^ set(exports))
        for sym in declared:
            assert hasattr(lib, sym), sym
    # the product header is the reference-facing list plus the pipelined calls: no kernel-level / debug entry point in it
    assert not any(s.startswith(("rtd_op_", "rtd_bench_", "rtd_debug_", "rtd_profile")) for s in _capi.EXPORTS)
    assert lib.rtd_version().startswith(b"mi355-rtdetr")
    # argument validation happens before any HIP call
    cfg = _capi.make_config(ARCHS["r18"], 0, _capi.PREC_BF16, 8, (641, 640), True)
    h = ctypes.c_void_p()
    assert lib.rtd_create(ctypes.byref(cfg), ctypes.byref(h)) == _capi.RTD_E_INVALID
    assert b"multiple of 32" in lib.rtd_last_error(None)
    cfg = _capi.make_config(ARCHS["r18"], 0, _capi.PREC_BF16, 8, (640, 640), True)
    cfg.struct_size = 12
    assert lib.rtd_create(ctypes.byref(cfg), ctypes.byref(h)) == _capi.RTD_E_INVALID
    cfg = _capi.make_config(ARCHS["r18"], 0, _capi.PREC_BF16, 8, (640, 640), True, profile=7)   # RTD_PROFILE_* is 0 or 1
    assert lib.rtd_create(ctypes.byref(cfg), ctypes.byref(h)) == _capi.RTD_E_INVALID
    assert _capi.make_config(ARCHS["r18"], 0, _capi.PREC_BF16, 8, (640, 640), True).profile == _capi.PROFILE_LATENCY
    assert lib.rtd_debug_option(b"no_such_option", 1) == _capi.RTD_E_INVALID


@pytest.mark.parametrize("changes,why", [
    (dict(num_queries=0), "num_queries <= 1024"), (dict(num_queries=1025), "num_queries <= 1024"), (dict(num_classes=82), r"num_classes % 4 == 0"),
    (dict(n_points=0), r"n_points must be in \[1,8\]"), (dict(n_points=9), r"n_points must be in \[1,8\]"),
    (dict(dec_heads=4), "decoder head dim must be 32"), (dict(dec_heads=16), "decoder head dim must be 32"),
    (dict(dec_heads=3), "decoder head dim must be 32"),
])
def test_rtd_create_refuses_head_shapes_outside_its_range(changes, why):
    """rtd_create validates before any HIP call: the decoder-head shapes next to the accepted range (num_queries 1..1024,
    num_classes % 4 == 0, n_points 1..8, head dim 32) are RTD_E_INVALID with the reason - and the shapes at the ends of the range pass the
    same checks (tests/test_gpu_head_configs.py runs them)"""
    from dataclasses import replace
    from telescope_cam_detection_amd import _capi
    lib = _capi.lib()
    cfg = _capi.cfg_for(replace(ARCHS["r18"], **changes), input_size=(320, 320))
    h = ctypes.c_void_p()
    rc = lib.rtd_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == _capi.RTD_E_INVALID and not h.value
    assert re.search(why, lib.rtd_last_error(None).decode()), lib.rtd_last_error(None)


def test_maxpool_refuses_what_its_deleted_kernels_took():
    """bf16 and pair tensors are pooled in 2 x 2 output patches of whole 16-byte chunks only (every plan rtd_create admits has even pooled
    extents and C % 8 == 0): an odd pooled extent or a partial chunk is an RtdError from the launcher's checks, before any launch
    (the placeholder pointers are never read)"""
    from telescope_cam_detection_amd import _capi
    lib = _capi.lib()
    p = ctypes.c_void_p(4096)
    for dt, C_ in ((_capi.DT_BF16, 64), (_capi.DT_F16X2, 64)):
        rc = lib.rtd_op_pool(0, dt, p, p, 1, 6, 6, C_, C_, C_)                      # 6 x 6 -> 3 x 3
        assert rc == _capi.RTD_E_INVALID
        with pytest.raises(_capi.RtdError, match="even pooled extents"):
            _capi._raise(rc, None)
    rc = lib.rtd_op_pool(0, _capi.DT_BF16, p, p, 1, 8, 8, 12, 12, 12)                # C % 8 != 0
    assert rc == _capi.RTD_E_INVALID
    with pytest.raises(_capi.RtdError, match="16-byte channel chunks"):
        _capi._raise(rc, None)


def test_decoder_op_entry_points_refuse_bad_shapes_before_any_device_work():
    """the kernel-level entry points of the selection / decoder glue validate their shapes first: RTD_E_INVALID with the reason, and the
    placeholder pointers (aligned, never read) are not touched - no HIP call is made, so this holds without a GPU"""
    from telescope_cam_detection_amd import _capi
    lib = _capi.lib()
    p = ctypes.c_void_p(4096)
    lv = (ctypes.c_int32 * 6)(4, 4, 2, 2, 1, 1)

    def refused(rc, why):
        assert rc == _capi.RTD_E_INVALID
        with pytest.raises(_capi.RtdError, match=why):
            _capi._raise(rc, None)

    for direction in (0, 1, 2):
        refused(lib.rtd_op_split_convert(direction, p, p, 5, 48, 64, 64), "32-channel groups")      # C % 32 != 0
    refused(lib.rtd_op_split_convert(3, p, p, 5, 32, 32, 32), "direction")
    refused(lib.rtd_op_select_score(p, 320, p, p, p, p, p, 1, 16, 80, 320), "256-wide rows")       # a score width other than 256
    refused(lib.rtd_op_select_score(p, 128, p, p, p, p, p, 1, 16, 80, 128), "256-wide rows")
    refused(lib.rtd_op_msdeform_view(_capi.DT_F32, p, 768, 513, p, p, p, 1, 4, 8, 32, 3, 4, lv, 0.5), "leaves the value row")   # coff + 256 > ld
    refused(lib.rtd_op_msdeform_view(_capi.DT_F32, p, 256, 256, p, p, p, 1, 4, 8, 32, 3, 4, lv, 0.5), "leaves the value row")
    refused(lib.rtd_op_msdeform_view(_capi.DT_F32, p, 768, 0, p, p, p, 1, 4, 8, 16, 3, 4, lv, 0.5), "head dim must be 32")      # hd != 32
    refused(lib.rtd_op_postprocess(p, p, p, 1, 300, 80, 100, 1, p), "K == Q")
    refused(lib.rtd_op_postprocess(p, p, p, 1, 300, 110, 300, 1, p), "one-launch form does not take this shape")   # Q * C > 32768 keys


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_detector_fails_loudly_without_gpu():
    """the product path has no CPU fallback: load_model() -> False (never raises), detect() -> [] (reference :248-250)"""
    from telescope_cam_detection_amd.rtdetr_detector import RTDETRDetector
    det = RTDETRDetector(config_path="tiny", model_path="synthetic:tiny:1", device="cuda:0", input_size=(160, 160))
    assert det.load_model(max_retries=1) is False
    assert det.model is None
    assert det.detect(np.zeros((160, 160, 3), np.uint8)) == []
    assert det.detect_batch([np.zeros((160, 160, 3), np.uint8)] * 2) == [[], []]
    cpu = RTDETRDetector(config_path="tiny", model_path="synthetic:tiny:1", device="cpu", input_size=(160, 160))
    assert cpu.load_model(max_retries=1) is False          # "cpu" is not a device this detector can use
    assert det.is_wildlife_relevant(21) and det.get_class_category(14) == "bird"


def test_block_to_detections_matches_reference_row_loop():
    from telescope_cam_detection_amd.shard import block_to_detections
    rng = np.random.default_rng(0)
    Q = 40
    labels = rng.integers(0, 80, Q)
    scores = np.sort(rng.uniform(0, 1, Q).astype(np.float32))[::-1]
    boxes = rng.uniform(0, 640, (Q, 4)).astype(np.float32)
    block = np.concatenate([labels[:, None].astype(np.float32), scores[:, None], boxes], 1)[None]
    for wl in (True, False):
        assert block_to_detections(block, 0.3, wl)[0] == orc.format_detections(labels, boxes, scores, 0.3, wl)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _collate_worker(rank, world, port, q):
    import torch.distributed as dist
    from telescope_cam_detection_amd.shard import cameras_of_rank, collate_blocks
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cams = cameras_of_rank(4, rank, world)                   # 4 cameras over 2 ranks
    block = torch.stack([torch.full((5, 6), float(10 * k)) + torch.arange(6) for k in cams])   # [2, Q=5, 6]
    out = collate_blocks(block)
    dist.barrier()
    q.put((rank, cams, out.numpy()))
    dist.destroy_process_group()


def test_collate_detections_world_size_2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_collate_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == [0, 2] and res[1][1] == [1, 3]
    for rank, cams, out in res:
        assert out.shape == (2, 2, 5, 6)
        for r in range(2):
            for j, k in enumerate([r, r + 2]):               # camera k lives on rank k % 2
                np.testing.assert_array_equal(out[r, j], np.full((5, 6), 10.0 * k) + np.arange(6))


def test_bench_self_launch_forms_a_world_of_two_on_gloo():
    """`python bench.py --gpus 2` with no torch.distributed environment must start its own ranks: the parent
    touches no GPU and spawns `torch.distributed.run`; --launch-selftest swaps the GPU work for a gloo all-gather of the rank ids."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-selftest"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                        # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["world"] == 2 and out["ranks"] == [0, 1] and out["gpus"] == 2


def test_bench_options_and_output_dump(tmp_path, monkeypatch):
    """a plain bench.py run leaves the side measurements to --full; --dump-outputs writes float32 .npy files, and outputs that exceed the
    size limit together keep the same seeded sample of their elements on every run"""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.full is False and a.dump_outputs == "" and a.steps == 5 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", str(tmp_path), "--profile-out", "p.json"])
    assert a.full is True and a.dump_outputs == str(tmp_path)
    for bad in (["--profile-out", "p.json"], ["--steps", "0"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    small = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    big = np.random.default_rng(3).standard_normal((64, 1000))
    bench.write_outputs(str(tmp_path / "a"), {"small": small, "big": big})
    assert np.load(tmp_path / "a" / "small.npy").dtype == np.float32
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "big.npy"), big.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100_000)
    for d in ("b", "c"):
        bench.write_outputs(str(tmp_path / d), {"small": small, "big": big})
    s = np.load(tmp_path / "b" / "small.npy")
    np.testing.assert_array_equal(s, small.astype(np.float32))                   # under its share: whole
    b = np.load(tmp_path / "b" / "big.npy")
    assert b.dtype == np.float32 and b.ndim == 1 and s.nbytes + b.nbytes <= 100_000 and b.size == 50_000 // 4
    np.testing.assert_array_equal(b, np.load(tmp_path / "c" / "big.npy"))
    assert np.isin(b, big.astype(np.float32)).all()


class _FakeEngine:
    """stands in for _capi.Engine on a box without a GPU: records what the detector asks for"""
    max_batch, num_queries = 4, 5

    def __init__(self):
        self.calls = []

    def infer(self, frames, conf, wildlife_only, on_device=False):
        from telescope_cam_detection_amd import _capi
        self.calls.append((len(frames), conf, wildlife_only, on_device))
        row = np.zeros(1, dtype=_capi.DET_DTYPE)
        row["class_id"], row["score"], row["x1"], row["y1"], row["x2"], row["y2"] = 16, 0.9, 1.0, 2.0, 11.5, 22.25
        return [row for _ in frames]


def test_detector_survives_the_callers_degrade_writes():
    """src/inference_engine_yolox.py:726-748 writes `detector.input_size`, `detector.device = "cpu"` and calls
    `detector.model.to("cpu")` inside a try: the first two must not re-route an engine that stays on its GPU, the third raises
    (caught and logged by the caller).  detect / detect_batch keep working afterwards."""
    from telescope_cam_detection_amd.rtdetr_detector import RTDETRDetector, _DeviceModel
    det = RTDETRDetector(config_path="r18", model_path="synthetic:r18:0", device="cuda:3", input_size=(640, 640))
    assert det.precision == "f16x3"                       # the default engine is the one held to the reference tolerance
    eng = _FakeEngine()
    det.model, det._dev_index, det._engine_input_size = _DeviceModel(eng, "cuda:3"), 3, (640, 640)
    # --- the caller's _apply_degradation, verbatim in effect ---
    det.input_size = (480, 480)
    if hasattr(det, "exp") and det.exp is not None:
        det.exp.test_size = (480, 480)
    det.device = "cpu"
    moved = True
    try:
        det.model.to("cpu")
    except Exception:
        moved = False
    assert moved is False                                   # no CPU path: the caller logs "Failed to move model to CPU"
    # --- and keeps calling the detector ---
    frame = np.zeros((64, 64, 3), np.uint8)
    got = det.detect(frame)
    assert got == [{"class_id": 16, "class_name": "dog", "confidence": pytest.approx(0.9), "bbox": {"x1": 1.0, "y1": 2.0, "x2": 11.5, "y2": 22.25, "area": 212}}]
    assert len(det.detect_batch([frame] * 6)) == 6          # 6 frames over max_batch 4 -> two device batches
    assert [c[0] for c in eng.calls] == [1, 4, 2]
    assert det._dev_index == 3 and det._engine_input_size == (640, 640)
    # settings writes of update_settings (:678, :684) take effect on the next call
    det.conf_threshold = 0.5
    det.nms_threshold = 0.45
    det.detect(frame)
    assert eng.calls[-1][1] == 0.5


def test_oom_return_code_becomes_torch_cuda_out_of_memory_error():
    """RTD_E_OOM is the one code the shim re-raises as torch.cuda.OutOfMemoryError - the only exception the caller's recovery path
    reacts to (src/inference_engine_yolox.py:607); every other code is a plain RuntimeError subclass (caught by :625-627)."""
    from telescope_cam_detection_amd import _capi
    with pytest.raises(torch.cuda.OutOfMemoryError):
        _capi._raise(_capi.RTD_E_OOM, None)
    with pytest.raises(_capi.RtdError) as ei:
        _capi._raise(_capi.RTD_E_HIP, None)
    assert not isinstance(ei.value, torch.cuda.OutOfMemoryError) and ei.value.code == _capi.RTD_E_HIP
    assert _capi.precision_code("f16x3") == _capi.PREC_F16X3 and _capi.precision_code("fp32") == _capi.PREC_FP32
    with pytest.raises(ValueError):
        _capi.precision_code("int8")


def test_split_layout_host_mirror_roundtrip():
    """_capi.to_split / from_split mirror csrc/common.h's F16X2 layout: 32-channel groups [32 hi | 32 lo] of fp16; hi + lo is within
    2^-22 of x in relative terms or 2^-25 in absolute terms (the lo half goes subnormal below |x| = 2^-3), and saturates at +-65504"""
    from telescope_cam_detection_amd import _capi
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, 5, 96)) * np.exp(rng.uniform(-8, 8, (3, 5, 96)))).astype(np.float32)
    s = _capi.to_split(x)
    assert s.shape == (3, 5, 192) and s.dtype == np.uint16
    y = _capi.from_split(s)
    assert np.all(np.abs(y - x) <= np.maximum(np.abs(x) * 2.0 ** -22, 2.0 ** -25))
    hi = s.reshape(3, 5, 3, 2, 32)[..., 0, :].copy().view(np.float16).astype(np.float32).reshape(3, 5, 96)
    assert np.all(np.abs(hi - x) <= np.maximum(np.abs(x) * 2.0 ** -11, 2.0 ** -25))   # the hi half alone is the fp16 rounding of x
    big = np.full((1, 32), 1.0e6, np.float32)
    assert np.all(_capi.from_split(_capi.to_split(big)) == 65504.0) and np.all(_capi.from_split(_capi.to_split(-big)) == -65504.0)
    z = np.zeros((2, 64), np.float32)
    assert np.array_equal(_capi.from_split(_capi.to_split(z)), z)


def test_the_library_never_captures_a_stream_and_the_package_never_wraps_its_stream():
    """VERDICT r3 item 1, kept true by construction: (a) no `torch.cuda.ExternalStream` anywhere in the product, the bench or the tests
    (torch and RCCL never see the engine's stream; ordering goes through rtd_wait_stream / rtd_signal_stream), (b) no stream capture in
    the library's sources (graphs are built node by node), (c) every kernel launch of the library goes through rtd_launch, the one place
    that turns a launch into a graph node."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    py = glob.glob(os.path.join(root, "telescope_cam_detection_amd", "*.py")) + glob.glob(os.path.join(root, "tests", "*.py")) + [os.path.join(root, "bench.py")]
    me = os.path.abspath(__file__)
    for f in py:
        if os.path.abspath(f) == me:
            continue
        src = open(f).read()
        assert "ExternalStream(" not in src, f
    csrc = glob.glob(os.path.join(root, "telescope_cam_detection_amd", "csrc", "*"))
    assert csrc
    for f in csrc:
        src = open(f).read()
        code = re.sub(r"//[^\n]*", "", src)                       # comments may talk about it
        assert "hipStreamBeginCapture" not in code and "hipStreamEndCapture" not in code, f
        if f.endswith(".hip"):
            assert "hipLaunchKernelGGL" not in code and "<<<" not in code, f
        if os.path.basename(f) in ("ops.hip", "conv_igemm.hip", "decoder.hip"):
            # the files that hold the plan ops' launchers contain no other stream call - a hipMem*Async / hipEventRecord inside a
            # launcher would run once on the live stream while the graph is BUILT and be missing from every replay (build_exec only counts
            # rtd_launch calls).  Memsets / copies live in engine.hip, outside the plan ops.
            for call in ("hipMemsetAsync", "hipMemcpyAsync", "hipMemcpy2DAsync", "hipEventRecord", "hipStreamWaitEvent", "hipLaunchHostFunc"):
                assert call not in code, (f, call)
    common = open(os.path.join(root, "telescope_cam_detection_amd", "csrc", "common.h")).read()
    assert common.count("hipLaunchKernelGGL(") == 1 and "hipGraphAddKernelNode" in common


def test_packed_blob_cache_is_keyed_by_source_and_survives_a_torn_file(tmp_path, monkeypatch):
    """the ranks of a node fold a checkpoint once.  Same (variant, source) -> the cached bytes, bit for bit; another
    seed or a touched file -> another key; a torn cache file is rebuilt, not trusted; RTD_BLOB_CACHE=0 switches the cache off."""
    from telescope_cam_detection_amd import weights as W
    monkeypatch.setenv("RTD_BLOB_CACHE", str(tmp_path))
    arch = ARCHS["tiny"]
    calls = []

    def make(seed):
        def f():
            calls.append(seed)
            return W.synth_weights(arch, seed)
        return f
    a = W.cached_blob(arch, "synthetic:tiny:1", make(1))
    b = W.cached_blob(arch, "synthetic:tiny:1", make(1))
    assert a == b == W.pack_blob(W.fold_weights(arch, W.synth_weights(arch, 1))) and calls == [1]
    c = W.cached_blob(arch, "synthetic:tiny:2", make(2))
    assert c != a and calls == [1, 2] and len(list(tmp_path.glob("*.rtdw"))) == 2
    path = tmp_path / (W.blob_cache_key(arch, "synthetic:tiny:1") + ".rtdw")
    path.write_bytes(a[: len(a) // 2])                                  # a torn write
    assert W.cached_blob(arch, "synthetic:tiny:1", make(1)) == a and calls == [1, 2, 1]
    f = tmp_path / "ckpt.pth"
    f.write_bytes(b"x")
    k1 = W.blob_cache_key(arch, str(f))
    f.write_bytes(b"xy")
    assert W.blob_cache_key(arch, str(f)) != k1 != W.blob_cache_key(ARCHS["tinyb"], str(f))
    monkeypatch.setenv("RTD_BLOB_CACHE", "0")
    assert W.cached_blob(arch, "synthetic:tiny:1", make(1)) == a and calls[-1] == 1 and len(calls) == 4


def test_two_rank_launch_and_gather_rehearsal_on_cpu():
    """The launch + rendezvous + gather of tests/shard_ws2_child.py (the GPU box runs it with real engines) rehearsed here without a GPU:
    torch.distributed.run on 127.0.0.1 with a port of our choosing, gloo, camera k -> rank k mod 2."""
    from tests.test_rccl_collate import run_two_ranks
    out = run_two_ranks({"SHARD_DRY": "1"}, 240)
    assert out["world"] == 2 and out["dry"] is True and out["bit_exact"] is True and out["cameras"] == {"0": [0, 2], "1": [1, 3]}
