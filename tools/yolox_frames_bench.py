"""Benchmark of the YOLOX uint8 front end (rtd_yolox_net_run_frames, csrc/yolox_net.hip yolox_focus_u8): yolox-s at 640 x 640 on the
f16x3 engine with seeded weights, from one and eight 1920 x 1080 or 2560 x 1440 BGR frames, device-resident or host numpy.

    python tools/yolox_frames_bench.py calls [--rounds 5] [--per 10] [--out profiles/yolox_frames_bench.json]
        per workload, alternating the two sides round by round in one process: the path before the fused front end -
        torch.cat([YOLOXDetector.preprocess(f) for f in frames]) + rtd_yolox_net_run - and YoloxNetwork.run_frames, each between HIP
        events on torch's stream, `per` calls back to back per round, median and range over the rounds after a warm-up.  The head rows of
        the two are compared first (the scale factors 1.6875, 3, 2.25 and 4 are dyadic, so the two inputs are the same numbers).
    rocprofv3 --kernel-trace --stats -d DIR -o yf --output-format csv -- python tools/yolox_frames_bench.py run --workload dev_1080p_b8 --calls 20
        the run to profile (one workload per run, so that a kernel's average belongs to one shape)
    python tools/yolox_frames_bench.py kernel --workload dev_1080p_b8 --stats DIR/yf_kernel_stats.csv [--out profiles/yolox_frames_bench.json]
        the front-end kernel's time in that run against the bytes it must move: the source frames read once + the Focus map written
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 640
HBM_PEAK_GBS = 8000.0
SHAPES = {"1080p": (1080, 1920), "1440p": (1440, 2560)}
WORKLOADS = {f"{src}_{res}_b{n}": (src, res, n) for src in ("dev", "host") for res in SHAPES for n in (1, 8)}


def make(workload):
    import torch

    from telescope_cam_detection_amd.synth import noise_frame
    from telescope_cam_detection_amd.yolox_detector import YOLOXDetector
    from telescope_cam_detection_amd.yolox_network import YoloxNetwork
    from tests import yolox_net_ref as ref
    src, res, n = WORKLOADS[workload]
    h, w = SHAPES[res]
    net = YoloxNetwork(ref.synth_state("yolox-s", 80, 1), "yolox-s", max_batch=8, precision="f16x3", input_size=(SIZE, SIZE))
    frames = [noise_frame(300 + i, h, w) for i in range(n)]
    if src == "dev":
        frames = [torch.from_numpy(f).cuda() for f in frames]
    pre = YOLOXDetector(device="cuda:0", input_size=(SIZE, SIZE), frontend="torch")          # only its preprocess() is used
    return net, frames, pre


def must_move(workload):
    """bytes the front-end kernel cannot avoid: every frame byte read once, every Focus group (32 channels x 4 bytes in either storage) written"""
    _, res, n = WORKLOADS[workload]
    h, w = SHAPES[res]
    return n * (h * w * 3 + (SIZE // 2) * (SIZE // 2) * 32 * 4)


def merge(path, update):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    for k, v in update.items():
        doc.setdefault(k, {}).update(v)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def summary(v):
    s = sorted(v)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "rounds": len(s)}


def one_round(call, per):
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(per):
        call()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) / per


def cmd_calls(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    res = {}
    for name in WORKLOADS:
        net, frames, pre = make(name)
        try:
            def parent():
                with torch.no_grad():
                    return net(torch.cat([pre.preprocess(f) for f in frames], dim=0))

            def fused():
                return net.run_frames(frames)

            for _ in range(3):
                want, got = parent(), fused()
            torch.cuda.synchronize()
            err = float((got - want).abs().max())
            t = {"parent": [], "fused": []}
            for _ in range(a.rounds):                                    # alternating: both sides see the same box at the same time
                t["parent"].append(one_round(parent, a.per))
                t["fused"].append(one_round(fused, a.per))
            src, shape, n = WORKLOADS[name]
            r = {"frames": n, "frame": list(SHAPES[shape]), "source": "device uint8 tensors" if src == "dev" else "host numpy uint8", "input": [SIZE, SIZE],
                 "precision": "f16x3", "calls_per_round": a.per, "max_abs_delta_between_the_sides": err,
                 "preprocess_cat_rtd_yolox_net_run": summary(t["parent"]), "run_frames": summary(t["fused"])}
            r["ratio_parent_over_fused"] = round(r["preprocess_cat_rtd_yolox_net_run"]["median_ms"] / r["run_frames"]["median_ms"], 3)
            res[name] = r
            print(json.dumps({name: r}), flush=True)
        finally:
            net.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    import torch
    net, frames, _ = make(a.workload)
    try:
        for _ in range(a.calls):
            net.run_frames(frames)
        torch.cuda.synchronize()
        print(json.dumps({"workload": a.workload, "calls": a.calls}))
    finally:
        net.close()


def cmd_kernel(a):
    found = None
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            if "yolox_focus_u8" in r.get("Name", ""):
                found = r
    if found is None:
        raise SystemExit("no yolox_focus_u8 kernel in " + a.stats)
    avg_us = float(found["AverageNs"]) / 1e3
    b = must_move(a.workload)
    out = {"kernel": found["Name"][:100], "calls": int(found["Calls"]), "avg_us": round(avg_us, 2), "must_move_bytes": b,
           "achieved_gbytes_per_s": round(b / avg_us / 1e3, 1), "share_of_hbm_peak": round(b / avg_us / 1e3 / HBM_PEAK_GBS, 3), "hbm_peak_gbytes_per_s": HBM_PEAK_GBS}
    print(json.dumps({a.workload: out}, indent=1))
    merge(a.out, {"kernel": {a.workload: out}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernel"])
    ap.add_argument("--workload", choices=list(WORKLOADS), default="dev_1080p_b8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "yolox_frames_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernel": cmd_kernel}[a.cmd](a)


if __name__ == "__main__":
    main()
