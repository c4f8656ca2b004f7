"""bench.py as the driver runs it - `python bench.py --gpus 1 --steps K --warmup W`, plain (the timed steps only, and what they computed
under --dump-outputs) and with --full, every side leg switched on - must finish and print ONE JSON line with the contract's fields (a
NameError in the CPU-baseline leg once survived a whole round because nothing ran that leg before the driver did).  Also a second, lean
line for the two_stage workload and the collate step (world-size-1 RCCL group)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_bench(*args, timeout=600):
    env = dict(os.environ, RTD_CPU_THREADS=os.environ.get("RTD_CPU_THREADS", "16"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_default_command_prints_the_contract_line_with_every_leg():
    d = run_bench("--gpus", "1", "--steps", "10", "--warmup", "3", "--full")
    assert d["metric"] == "frames_per_sec" and d["unit"] == "frames/s" and d["n_gpus"] == 1 and d["steps"] == 10 and d["warmup"] == 3
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and d["dtype"] == "f16x3"
    assert d["value"] > 500 and abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) / d["value"] < 1e-3
    assert "RT-DETR-R50 640x640 bs=8" in d["config"]["workload"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 2500 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert 0.03 < rf["frac"] < 0.4
    # the committed PMC / rocprofv3 summaries must belong to THESE kernel sources (tools/refresh_profiles.sh + commit_profiles.sh after the
    # last kernel change of a round): bench.py attaches them only when their csrc stamp matches
    assert rf["traffic"] is not None and rf["traffic"] > 10 and "avg_launch_us_rocprofv3" in rf and "mfma_busy_frac_pmc" in rf, rf
    assert abs(rf["avg_launch_us_rocprofv3"] - rf["avg_launch_us"]) / rf["avg_launch_us"] < 0.15      # HIP-event and rocprofv3 durations agree
    assert d["hbm"]["gbytes_per_step_pmc"] > 5
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "frames/s" and "sample" in cb
    assert d["cpu_baseline_r18_bs1"]["p50"] > 0 and d["cpu_baseline_r18_bs1"]["kind"] == "port"
    assert d["p50_ms_per_frame_bs1"] < 10.0                              # the north star's latency target
    assert d["rccl_ranks"] == 0 and "detect_host_ms" in d and "multi_stream" in d and "bf16_engine" in d


def test_two_stage_and_collate_lines(tmp_path):
    lean = ("--steps", "10", "--warmup", "3", "--multi-streams", "0", "--no-bf16-line", "--no-cpu-baseline", "--no-latency", "--no-detect-host", "--no-mfma-probe")
    d = run_bench("--workload", "two_stage", "--dump-outputs", str(tmp_path), *lean)
    assert d["config"]["stage2"]["crops_per_step"] == 16 and "asynchronous" in d["config"]["stage2"]["timed"] and d["value"] > 500
    crops = np.load(tmp_path / "crops.npy")                              # the last step's Stage-2 classifier input
    assert crops.dtype == np.float32 and crops.shape == (16, 3, 336, 336) and np.isfinite(crops).all() and crops.std() > 0
    d = run_bench("--collate", "--batch", "1", "--full", *lean)          # BASELINE configs[3]'s per-rank shape at N = 1
    assert d["rccl_ranks"] == 1 and d["collate"]["bytes_per_rank"] == 300 * 6 * 4 and d["collate"]["rccl_ranks"] == 1
    assert "bs=1/GPU" in d["config"]["workload"]


def test_plain_command_times_the_steps_only_and_dumps_what_they_computed(tmp_path):
    """the plain command: the contract line and nothing that takes a run of its own; --dump-outputs writes the last timed step's result
    block, which is what the same engine answers for the same frames (bench.py's camera group 0: noise_frame(2000 + i))"""
    import torch

    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.arch import ARCHS
    from telescope_cam_detection_amd.synth import noise_frame
    from telescope_cam_detection_amd.weights import cached_blob, synth_weights

    d = run_bench("--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path), timeout=300)
    assert d["metric"] == "frames_per_sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f16x3"
    assert d["steps"] == 7 and d["warmup"] == 2 and d["value"] > 500 and abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) / d["value"] < 1e-3
    for side in ("roofline", "kernel_families_ms", "p50_ms_per_frame_bs1", "multi_stream", "bf16_engine", "detect_host_ms", "cpu_baseline",
                 "cpu_baseline_r18_bs1", "collate", "hbm"):
        assert side not in d, side
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("labels", "scores", "boxes")}
    assert sorted(os.listdir(tmp_path)) == ["boxes.npy", "labels.npy", "scores.npy"]
    assert got["labels"].shape == (8, 300) and got["scores"].shape == (8, 300) and got["boxes"].shape == (8, 300, 4)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    arch = ARCHS["r50"]
    assert (got["labels"] == np.round(got["labels"])).all() and got["labels"].min() >= 0 and got["labels"].max() < arch.num_classes
    blob = cached_blob(arch, "synthetic:r50:0", lambda: synth_weights(arch, 0))
    eng = _capi.Engine(arch, blob, device=0, precision=_capi.PREC_F16X3, max_batch=8, input_size=(640, 640), use_graph=True)
    try:
        frames = [torch.from_numpy(noise_frame(2000 + i, 640, 640)).cuda() for i in range(8)]
        labels, boxes, scores = eng.infer_raw(frames, on_device=True)
    finally:
        eng.close()
    np.testing.assert_allclose(np.sort(got["scores"], axis=1), np.sort(scores, axis=1), atol=1e-3)
