"""The r50vd_m and sp1 / sp2 / sp3 variants, shared by tools/make_points_golden.py (which writes the fixtures and searched the seeds) and by
tests/test_variants_host.py and tests/test_gpu_variants.py: the case tables, the oracle runs of a case (computed once per session and
never changed) and the three conditions under which a case's data is well posed (tests/test_gpu_head_configs.py,
test_reference_is_well_posed): the fp32 oracle selects the fp64 oracle's tokens, all its rows match at 1e-3 / 1e-2 px, and both top-Q
cuts are at least 10 x wider than the fp32 oracle's own error there.  The seeds of every case were searched on the CPU for those three
conditions and nothing else (tools/make_points_golden.py --search) and are part of the tables."""
import contextlib
import json
import os
from dataclasses import replace

import numpy as np
import torch

from oracle import rtdetr_oracle as orc
from telescope_cam_detection_amd.arch import ARCHS
from telescope_cam_detection_amd.synth import make_frame, noise_frame, scene_frame
from tests.dsp_ref import discrete_oracle
from tests.util import match_detections, to64, weights_for

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YARDSTICK = "points_yardstick.json"

# HF fixtures: name -> (arch, weight seed, input size (H, W), [(frame seed, frame H, frame W)], frame kind), the layout of
# oracle.make_golden.CASES.  160 x 224: 20 x 28 + 10 x 14 + 5 x 7 = 735 memory tokens for 300 queries; the second frame goes through
# the resampler.
POINTS_CASES = {
    "p1_r18sp1_160x224": ("r18_sp1", 0, (160, 224), [(6100, 160, 224), (6101, 200, 150)], "scene"),
    "p2_r18sp2_160x224": ("r18_sp2", 0, (160, 224), [(6100, 160, 224), (6101, 200, 150)], "scene"),
    "p3_r18sp3_160x224": ("r18_sp3", 0, (160, 224), [(6100, 160, 224), (6101, 200, 150)], "scene"),
    "m1_r50m_160x224": ("r50_m", 0, (160, 224), [(6100, 160, 224), (6101, 200, 150)], "scene"),
}

# engine cases: two 320 x 320 frames (one scene, one noise) as in tests/test_gpu_head_configs.py: 2100 memory tokens, 300 queries in 19
# row tiles, the last with 12 rows.  name -> (Arch, (weight seed, scene seed, noise seed), decoder path)
FUSED, PER_OP = "fused", "per-op"
SIZE = (320, 320)
ENGINE_CASES = {
    "r18_sp2": (ARCHS["r18_sp2"], (0, 5, 6), FUSED),
    "r18_sp3": (ARCHS["r18_sp3"], (0, 5, 6), FUSED),
    "r18_dsp_np2": (replace(ARCHS["r18_dsp"], n_points=2), (0, 7, 8), FUSED),      # (frame seeds 5 / 6: a tap flips inside the fp32 oracle)
    "r18_dsp_np3": (replace(ARCHS["r18_dsp"], n_points=3), (0, 9, 10), FUSED),     # (5 / 6: the same; 7 / 8: a post cut gap of 3e-6)
    "r18_sp1": (ARCHS["r18_sp1"], (0, 5, 6), PER_OP),
}
FUSED_ENGINE_CASES = [n for n, c in ENGINE_CASES.items() if c[2] == FUSED]


def threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))


def sampler_of(arch):
    """the oracle samples as the arch says inside this block (oracle/rtdetr_oracle.py itself is bilinear only)"""
    return discrete_oracle() if arch.dec_method == "discrete" else contextlib.nullcontext()


def yardstick():
    with open(os.path.join(GOLDEN_DIR, YARDSTICK)) as fh:
        return json.load(fh)


def load_points_case(name):
    """(arch, weight seed, input size, frames, npz) of a p* / m* fixture: tests.util.load_case for these files"""
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    wseed, ih, iw, n = (int(v) for v in g["meta"])
    frames = [make_frame(str(g["kind"]), int(s), int(h), int(w)) for s, h, w in g["frames"]]
    assert (wseed, (ih, iw), [tuple(int(v) for v in f) for f in g["frames"]]) == (POINTS_CASES[name][1], POINTS_CASES[name][2], POINTS_CASES[name][3])
    return ARCHS[POINTS_CASES[name][0]], wseed, (ih, iw), frames, g


def oracle_runs(name, arch, w, frames, input_size):
    """a case's fp32 and fp64 oracle runs in the layout of tests.test_gpu_head_configs.head_data (check_fp32_engine and x3_check read it)"""
    threads()
    xs, sizes = zip(*[orc.preprocess(f, input_size) for f in frames])
    x = torch.cat(xs, 0)
    col32, col64 = {}, {}
    with torch.no_grad(), sampler_of(arch):
        out32 = orc.model_forward(arch, w, x, list(sizes), collect=col32)
        w64, x64 = to64(w, x)
        out64 = orc.model_forward(arch, w64, x64, list(sizes), collect=col64)
    col64["input"] = x64
    return dict(name=name, arch=arch, w=w, frames=frames, sizes=list(sizes), x=x, input_size=input_size,
                out32=[t.numpy() for t in out32], out64=[t.numpy() for t in out64], col32=col32, col=col64)


_DATA = {}


def engine_data(name):
    if name not in _DATA:
        arch, (wseed, sseed, nseed), path = ENGINE_CASES[name]
        d = oracle_runs(name, arch, weights_for(arch, wseed), [scene_frame(sseed, *SIZE), noise_frame(nseed, *SIZE)], SIZE)
        d["decoder"] = path
        _DATA[name] = d
    return _DATA[name]


def fixture_data(name):
    if name not in _DATA:
        arch, wseed, input_size, frames, g = load_points_case(name)
        d = oracle_runs(name, arch, weights_for(arch, wseed), frames, input_size)
        d["g"], d["decoder"] = g, (FUSED if 2 <= arch.n_points <= 4 else PER_OP)
        _DATA[name] = d
    return _DATA[name]


def cut_gap(values, Q):
    v = np.sort(np.asarray(values, np.float64).ravel())[::-1]
    return float(v[Q - 1] - v[Q])


def by_token(topk_b, rows_b):
    return np.asarray(rows_b)[np.argsort(np.asarray(topk_b), kind="stable")]


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def well_posed(d, verbose=True):
    """the three conditions of test_reference_is_well_posed on a case's oracle runs -> (ok, [reason, ...]); prints every figure"""
    name, Q, c32, c64 = d["name"], d["arch"].num_queries, d["col32"], d["col"]
    (l32, b32, s32), (l64, b64, s64) = d["out32"], d["out64"]
    tk32, tk64 = c32["topk"].numpy(), c64["topk"].numpy()
    mx32, mx64 = c32["enc_cls_max"].numpy().astype(np.float64), c64["enc_cls_max"].numpy()
    e_sel = float(np.abs(mx32 - mx64).max())
    bad = []
    for b in range(len(d["frames"])):
        if set(tk32[b].tolist()) != set(tk64[b].tolist()):
            bad.append(f"[{b}] the fp32 oracle selects other tokens than the fp64 oracle")
            continue
        m, n, ws, wb = match_detections(l64[b], b64[b], s64[b], l32[b], b32[b], s32[b], 1e-3, 1e-2)
        if not m == n == Q:
            bad.append(f"[{b}] fp32 oracle rows matched {m}/{n}")
        sc32, sc64 = sig(by_token(tk32[b], c32["logits"][b].numpy())), sig(by_token(tk64[b], c64["logits"][b].numpy()))
        e_post = float(np.abs(sc32 - sc64).max())
        g_sel, g_post = cut_gap(mx64[b], Q), cut_gap(sc64, Q)
        if verbose:
            print(f"{name}[{b}] fp32 vs fp64 oracle: matched {m}/{n} worst dscore={ws:.2e} dbox={wb:.2e}px; selection cut gap {g_sel:.2e} "
                  f"(fp32 err {e_sel:.2e}), post cut gap {g_post:.2e} (err {e_post:.2e})")
        if g_sel < 10 * e_sel:
            bad.append(f"[{b}] selection cut gap {g_sel:.2e} < 10 x {e_sel:.2e}")
        if g_post < 10 * e_post:
            bad.append(f"[{b}] post cut gap {g_post:.2e} < 10 x {e_post:.2e}")
    return not bad, bad
