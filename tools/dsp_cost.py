#!/usr/bin/env python3
"""What the discrete sampler costs against the bilinear one: dec_layer_kernel's HIP-event time per step (rtd_profile) and the step time
(back-to-back graph replays, host clock around a device synchronise) of two or more variants in ONE process on one box, in alternating
rounds - boxes differ by several per cent in the clock they hold, so two runs never compare.

    python tools/dsp_cost.py --archs r50,r50_dsp --out profiles/dsp_decoder.json        (640^2, bs 8, f16x3)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", default="r50,r50_dsp")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel and round (rtd_profile)")
    ap.add_argument("--steps", type=int, default=60, help="graph replays per round")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.arch import ARCHS
    from telescope_cam_detection_amd.synth import noise_frame
    from telescope_cam_detection_amd.weights import cached_blob, synth_weights

    names = args.archs.split(",")
    B, S = args.batch, args.size
    frames = [torch.from_numpy(noise_frame(2000 + i, S, S)).cuda() for i in range(B)]       # bench.py's camera group 0
    engs, prepared = {}, {}
    for n in names:
        arch = ARCHS[n]
        blob = cached_blob(arch, f"synthetic:{n}:0", lambda arch=arch: synth_weights(arch, 0))
        engs[n] = _capi.Engine(arch, blob, 0, _capi.precision_code(args.precision), B, (S, S), use_graph=True)
        prepared[n] = engs[n].make_async_args(frames)
        for _ in range(5):                                     # real frames: the sampler's addresses depend on the data
            engs[n].infer_async_prepared(prepared[n])
        engs[n].sync()
    res = {n: {"dec_layer_us": [], "dec_layer_launch_us": [], "step_ms": []} for n in names}
    for _ in range(args.rounds):
        for n in names:
            e = engs[n]
            for _ in range(3):
                e.infer_async_prepared(prepared[n])
            e.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.infer_async_prepared(prepared[n])
            e.sync()
            res[n]["step_ms"].append((time.perf_counter() - t0) * 1e3 / args.steps)
            dec = [p for p in e.profile(B, args.reps) if p["kernel"] == "dec_layer" and ".fused" in p["name"]]
            res[n]["dec_layer_us"].append(sum(p["ms"] for p in dec) * 1e3)
            res[n]["dec_layer_launch_us"].append([round(p["ms"] * 1e3, 1) for p in dec])
    out = {"config": f"{S}x{S} bs{B} {args.precision}", "rounds": args.rounds, "lib": os.environ.get("RTD_LIB_PATH", "this build"),
           "method": "alternating rounds in one process; dec_layer_us = sum of the decoder layers' dec_layer_kernel launches per step, HIP events, "
                     f"mean of {args.reps}; step_ms = {args.steps} back-to-back graph replays, host clock around a device synchronise"}
    for n in names:
        d, s = res[n]["dec_layer_us"], res[n]["step_ms"]
        out[n] = {"dec_layer_us_median": round(statistics.median(d), 1), "dec_layer_us_min": round(min(d), 1), "dec_layer_us_max": round(max(d), 1),
                  "step_ms_median": round(statistics.median(s), 4), "step_ms_min": round(min(s), 4), "step_ms_max": round(max(s), 4),
                  "dec_layer_launch_us_last_round": res[n]["dec_layer_launch_us"][-1]}
        print(f"{n:10s} dec_layer {out[n]['dec_layer_us_median']:7.1f} us/step (min {min(d):.1f}, max {max(d):.1f})   step "
              f"{out[n]['step_ms_median']:.4f} ms (min {min(s):.4f}, max {max(s):.4f})", flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    for e in engs.values():
        e.close()


if __name__ == "__main__":
    main()
