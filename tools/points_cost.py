#!/usr/bin/env python3
"""What the decoder costs per layer at 2, 3 and 4 sampling points per level, fused (one dec_layer_kernel launch per layer) against per-op
(one launch per decoder op), with either sampler: HIP-event times of the plan's decoder launches (rtd_profile), all variants in ONE process
on one box in alternating rounds - boxes differ by several per cent in the clock they hold, so two runs never compare.  Modelled on
tools/dsp_cost.py.

    python tools/points_cost.py --out profiles/points_decoder.json        (R18, 640^2, bs 8, f16x3)

Counted per variant: every launch named dec.l<i>.* plus, on the fused path, dec.prologue (it computes layer 0's q | k | v, which the per-op
path does in dec.l0.sa.*); the sum over the decoder divided by its layers is the per-layer time.  The value projection of the memory
tokens is the same launch on both paths and is left out.
"""
import argparse
import json
import os
import statistics
import sys
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="2,3,4")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel and round (rtd_profile)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.arch import ARCHS
    from telescope_cam_detection_amd.synth import noise_frame
    from telescope_cam_detection_amd.weights import fold_weights, pack_blob, synth_weights

    B, S = args.batch, args.size
    frames = [noise_frame(2000 + i, S, S) for i in range(B)]       # bench.py's camera group 0
    variants = {}
    for k in (int(v) for v in args.points.split(",")):
        variants[f"np{k} bilinear"] = replace(ARCHS["r18"], n_points=k)
        variants[f"np{k} discrete"] = replace(ARCHS["r18_dsp"], n_points=k)
    engs = {}
    try:
        for tag, arch in variants.items():
            blob = pack_blob(fold_weights(arch, synth_weights(arch, 0)))
            for fused in (1, 0):
                _capi.debug_option("dec_fused", fused)          # read when the plan is built: the first call below
                e = _capi.Engine(arch, blob, 0, _capi.precision_code(args.precision), B, (S, S), use_graph=True)
                for _ in range(3):                                # real frames: the sampler's addresses depend on the data
                    e.infer_raw(frames)
                engs[(tag, "fused" if fused else "per-op")] = e
    finally:
        _capi.debug_option("reset", 0)

    def decoder_launches(e):
        return [p for p in e.profile(B, args.reps) if p["name"].startswith("dec.l") or p["name"] == "dec.prologue"]

    res = {key: [] for key in engs}
    for _ in range(args.rounds):
        for key, e in engs.items():
            e.infer_raw(frames)
            res[key].append(sum(p["ms"] for p in decoder_launches(e)) * 1e3)
    out = {"config": f"r18 {S}x{S} bs{B} {args.precision}", "rounds": args.rounds,
           "method": "alternating rounds in one process; per variant the sum of the plan's decoder launches (dec.l<i>.*, and dec.prologue on the "
                     f"fused path), HIP events, mean of {args.reps} per round, divided by the decoder's layers; median / min / max over the rounds"}
    for (tag, path), e in engs.items():
        layers = e.arch.dec_layers
        launches = decoder_launches(e)
        us = [v / layers for v in res[(tag, path)]]
        rec = {"layer_us_median": round(statistics.median(us), 1), "layer_us_min": round(min(us), 1), "layer_us_max": round(max(us), 1),
               "launches_per_step": len(launches), "layers": layers}
        if path == "fused":
            rec["dec_layer_launch_us_last_round"] = [round(p["ms"] * 1e3, 1) for p in launches]
        out.setdefault(tag, {})[path] = rec
        print(f"{tag:14s} {path:7s} {rec['layer_us_median']:7.1f} us per layer (min {rec['layer_us_min']:.1f}, max {rec['layer_us_max']:.1f}), "
              f"{len(launches)} launches per step", flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    for e in engs.values():
        e.close()


if __name__ == "__main__":
    main()
