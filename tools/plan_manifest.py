"""What the plan builder (csrc/engine.hip) produces for a fixed list of small cases, as JSON: per case the ordered launches of
`rtd_profile` (name, kernel, flops, bytes), the arena size, the node count of the built hipGraph and the SHA-256 of the result block
after one forward.  tests/test_gpu_plan_manifest.py compares a fresh record of each case with tests/golden/plan_manifest.json, so a
change to the builder that moves an allocation, reorders a launch or alters a launch argument shows up as a named difference.

    python tools/plan_manifest.py --out tests/golden/plan_manifest.json      (needs the MI355X; only when the plan is MEANT to change)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WEIGHT_SEED = 3
R50_SIZE = (512, 768)
# r50 f16x3 bs 1 once more per set of rtd_debug_option switches (and once with the throughput profile): the un-fused paths of the builder
R50_VARIANTS = {
    "throughput": {},
    "dec_fused=0": {"dec_fused": 0},
    "arena_reuse=0": {"arena_reuse": 0},
    "side_stream=0": {"side_stream": 0},
    "sc_fold=0,c1_fuse=0,up_fold=0": {"sc_fold": 0, "c1_fuse": 0, "up_fold": 0},
    "stem_fused_split=0,stem_pool_fuse=0,avg_fuse=0": {"stem_fused_split": 0, "stem_pool_fuse": 0, "avg_fuse": 0},
    "post_fused=0,sel_fused=0": {"post_fused": 0, "sel_fused": 0},
}


def cases():
    """[(key, arch name, (h, w), batch, precision, throughput profile?, {option: value})] - the smallest set that reaches every branch
    of the builder: bottleneck and basic blocks, op-by-op and fused AIFI / decoder / selection, the pair AIFI, the shortcut fold, the c1
    fuse inside and across stages, the fused average and its unwritten stage output, the stem fusions and each switch's other side."""
    out = []

    def add(aname, size, bs, prec, variant="", opts=None):
        key = f"{aname}-{size[0]}x{size[1]}-bs{bs}-{prec}" + (f"-{variant}" if variant else "")
        out.append((key, aname, size, bs, prec, variant == "throughput", dict(opts or {})))

    for prec in ("bf16", "fp32"):
        add("tiny", (160, 224), 1, prec)
    add("tinyc", (160, 224), 2, "f16x3")
    for prec in ("bf16", "fp32", "f16x3"):
        add("r18", (320, 320), 1, prec)
    for bs in (1, 2):
        for prec in ("f16x3", "bf16"):
            add("r50", R50_SIZE, bs, prec)
    for variant, opts in R50_VARIANTS.items():
        add("r50", R50_SIZE, 1, "f16x3", variant, opts)
    return out


_BLOBS = {}


def _blob(arch):
    from telescope_cam_detection_amd.weights import fold_weights, pack_blob
    from tests.util import weights_for
    if arch.name not in _BLOBS:
        _BLOBS[arch.name] = pack_blob(fold_weights(arch, weights_for(arch, WEIGHT_SEED)))
    return _BLOBS[arch.name]


def record(case) -> dict:
    """One engine with synthetic weights, one forward (eager pass + graph replay) on seeded frames, then the profile's op list."""
    import torch

    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.arch import ARCHS
    from telescope_cam_detection_amd.shard import DevBlock
    from telescope_cam_detection_amd.synth import make_frame

    key, aname, size, bs, prec, throughput, opts = case
    arch = ARCHS[aname]
    frames = [make_frame("noise" if i % 2 else "scene", 40 + i, size[0], size[1]) for i in range(bs)]
    try:
        for name, value in opts.items():
            _capi.debug_option(name, value)
        eng = _capi.Engine(arch, _blob(arch), device=0, precision=_capi.precision_code(prec), max_batch=bs, input_size=size, use_graph=True,
                           profile=_capi.PROFILE_THROUGHPUT if throughput else _capi.PROFILE_LATENCY)
    finally:
        _capi.debug_option("reset", 0)
    try:
        eng.infer_raw(frames)
        ptr, n = eng.result_block()
        block = torch.as_tensor(DevBlock(ptr, n), device="cuda:0").cpu().numpy()
        graph_nodes = eng.stats()["graph_nodes"]
        ops = [[p["name"], p["kernel"], repr(p["flops"]), repr(p["bytes"])] for p in eng.profile(bs, reps=1)]
        return {"ops": ops, "arena_bytes": eng.arena_bytes(), "graph_nodes": graph_nodes, "result_sha256": hashlib.sha256(block.tobytes()).hexdigest()}
    finally:
        eng.close()


def first_difference(want: dict, got: dict) -> str:
    """'' when the two records agree, else one line naming the first thing that differs."""
    for i, (a, b) in enumerate(zip(want["ops"], got["ops"])):
        if a != b:
            return f"op {i}: recorded {a}, now {b}"
    if len(want["ops"]) != len(got["ops"]):
        longer, which = (want, "recorded") if len(want["ops"]) > len(got["ops"]) else (got, "new")
        return f"{len(want['ops'])} ops recorded, now {len(got['ops'])}: first extra ({which}) {longer['ops'][min(len(want['ops']), len(got['ops']))]}"
    for k in ("arena_bytes", "graph_nodes", "result_sha256"):
        if want[k] != got[k]:
            return f"{k}: recorded {want[k]}, now {got[k]} (same op list" + (": a launch argument changed)" if k == "result_sha256" else ")")
    return ""


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    doc = {}
    for case in cases():
        doc[case[0]] = record(case)
        print(case[0], len(doc[case[0]]["ops"]), "ops", doc[case[0]]["arena_bytes"], "arena bytes", flush=True)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in doc.items()) + "\n}\n")   # a case per line


if __name__ == "__main__":
    main()
