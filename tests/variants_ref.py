"""The case tables of the r50vd_m and sp1 / sp2 / sp3 variants, shared by tests/test_variants_host.py, tests/test_gpu_variants.py and
oracle/make_golden.py --search, which found the seeds: every case's data meets tests.util.well_posed, and nothing else was looked at."""
import json
import os
from dataclasses import replace

from oracle.make_golden import CASES
from telescope_cam_detection_amd.arch import ARCHS
from telescope_cam_detection_amd.synth import noise_frame, scene_frame
from tests.engine_checks import FUSED, PER_OP
from tests.util import GOLDEN_DIR, load_case, reference_runs, weights_for

# the HF fixtures of these variants (rows of oracle.make_golden.CASES)
POINTS_CASES = [n for n in CASES if n[0] in "pm"]

# engine cases: two 320 x 320 frames (one scene, one noise) as in tests/test_gpu_head_configs.py: 2100 memory tokens, 300 queries in 19
# row tiles, the last with 12 rows.  name -> (Arch, (weight seed, scene seed, noise seed), decoder path)
SIZE = (320, 320)
ENGINE_CASES = {
    "r18_sp2": (ARCHS["r18_sp2"], (0, 5, 6), FUSED),
    "r18_sp3": (ARCHS["r18_sp3"], (0, 5, 6), FUSED),
    "r18_dsp_np2": (replace(ARCHS["r18_dsp"], n_points=2), (0, 7, 8), FUSED),      # (frame seeds 5 / 6: a tap flips inside the fp32 oracle)
    "r18_dsp_np3": (replace(ARCHS["r18_dsp"], n_points=3), (0, 9, 10), FUSED),     # (5 / 6: the same; 7 / 8: a post cut gap of 3e-6)
    "r18_sp1": (ARCHS["r18_sp1"], (0, 5, 6), PER_OP),
}
FUSED_ENGINE_CASES = [n for n, c in ENGINE_CASES.items() if c[2] == FUSED]


def yardstick():
    with open(os.path.join(GOLDEN_DIR, "points_yardstick.json")) as fh:
        return json.load(fh)


def engine_data(name):
    arch, (wseed, sseed, nseed), path = ENGINE_CASES[name]
    d = reference_runs(name, arch, weights_for(arch, wseed), [scene_frame(sseed, *SIZE), noise_frame(nseed, *SIZE)], SIZE)
    d["decoder"] = path
    return d


def fixture_data(name):
    arch, wseed, input_size, frames, g = load_case(name)
    d = reference_runs(name, arch, weights_for(arch, wseed), frames, input_size)
    d.setdefault("g", g)
    d["decoder"] = FUSED if 2 <= arch.n_points <= 4 else PER_OP
    return d
