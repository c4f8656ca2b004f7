"""Benchmark of the Stage-2 crop enhancement (rtd_enhance_crops, csrc/enhance.hip) on two workloads:
    crops8   8 crops of 256 x 256, one out of each of 8 1080p BGR device frames (synth.scene_frame)
    full     one crop that is a whole 1080p frame

    python tools/enhance_bench.py calls [--calls 50] [--out profiles/enhance_bench.json]
        per workload: the whole enhance() call (three launches; HIP events around it on torch's stream, and the host clock around call +
        synchronise: medians of five rounds, the per-round lists kept), and for scale the unchanged crop-resize launch
        (rtd_crop_resize_batch to 336 x 336) on the same crops, timed the same way
    rocprofv3 --kernel-trace --stats -d DIR -o enh --output-format csv -- python tools/enhance_bench.py run --workload crops8 --calls 20
        the run to profile (one workload per run, so that a kernel's average belongs to one shape)
    python tools/enhance_bench.py kernels --workload crops8 --stats DIR/enh_kernel_stats.csv [--out profiles/enhance_bench.json]
        the three kernel times from that file against the bytes each launch must move (crop read once + crop written once)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1080, 1920
HBM_PEAK_GBS = 8000.0            # MI355X HBM3E peak
WORKLOADS = {"crops8": (8, [(800, 400, 1056, 656)]), "full": (1, [(0, 0, W, H)])}


def scene(workload):
    import torch

    from telescope_cam_detection_amd.synth import scene_frame
    n, rects = WORKLOADS[workload]
    frames = [torch.from_numpy(scene_frame(40 + i, H, W)).cuda() for i in range(n)]
    torch.cuda.synchronize()
    return frames, [list(rects) for _ in range(n)]


def crop_bytes(workload):
    n, rects = WORKLOADS[workload]
    return n * sum(3 * (r[2] - r[0]) * (r[3] - r[1]) for r in rects)


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


def med(v):
    return round(sorted(v)[len(v) // 2], 4)


def cmd_calls(a):
    import torch

    from telescope_cam_detection_amd.enhance import CropEnhancer
    from telescope_cam_detection_amd.stage2 import CropBatcher
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    e = CropEnhancer()
    batcher = CropBatcher(min_crop_size=16)
    res = {}
    for name in WORKLOADS:
        frames, rects = scene(name)

        def device_ms(fn, calls):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(calls):
                fn()
            ev1.record()
            ev1.synchronize()
            return ev0.elapsed_time(ev1) / calls

        def host_ms(fn, calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / calls * 1e3

        enh = lambda: e.enhance(frames, rects)
        rsz = lambda: batcher.preprocess_batch(frames, rects)
        both = lambda: batcher.preprocess_batch(frames, rects, enhancer=e)
        for _ in range(3):
            enh(), rsz(), both()
        torch.cuda.synchronize()
        per = max(a.calls // 5, 1)
        rounds = {k: [] for k in ("enhance_device_ms", "enhance_call_and_sync_ms", "crop_resize_device_ms", "crop_resize_call_and_sync_ms",
                                  "enhance_plus_crop_resize_device_ms")}
        for _ in range(5):                    # the sides alternate so that all see the same machine load
            rounds["enhance_device_ms"].append(device_ms(enh, per))
            rounds["crop_resize_device_ms"].append(device_ms(rsz, per))
            rounds["enhance_plus_crop_resize_device_ms"].append(device_ms(both, per))
            rounds["enhance_call_and_sync_ms"].append(host_ms(enh, per))
            rounds["crop_resize_call_and_sync_ms"].append(host_ms(rsz, per))
        r = {"crops": WORKLOADS[name][0], "crop_bytes": crop_bytes(name), "params": e.params}
        for k, v in rounds.items():
            r[k] = med(v)
            r[k + "_rounds"] = [round(x, 4) for x in v]
        res[name] = r
        print(json.dumps({name: r}), flush=True)
    e.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    import torch

    from telescope_cam_detection_amd.enhance import CropEnhancer
    frames, rects = scene(a.workload)
    e = CropEnhancer()
    try:
        for _ in range(a.calls):
            e.enhance(frames, rects)
        torch.cuda.synchronize()
        print(json.dumps({"workload": a.workload, "calls": a.calls}))
    finally:
        e.close()


def cmd_kernels(a):
    b = 2 * crop_bytes(a.workload)               # every launch reads the crops once (3 B / px) and writes them once
    rows = {"bytes_per_launch": b, "us_at_hbm_peak": round(b / HBM_PEAK_GBS / 1e3, 2)}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            for k in ("enhance_lab_hist", "enhance_apply", "enhance_bilateral"):
                if k in name:
                    avg_us = float(r["AverageNs"]) / 1e3
                    gbs = b / avg_us / 1e3
                    rows[k] = {"calls": int(r["Calls"]), "avg_us": round(avg_us, 2), "gbytes_per_s": round(gbs, 1),
                               "fraction_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
    print(json.dumps({a.workload: rows}, indent=1))
    merge(a.out, {"kernels": {a.workload: rows}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels"])
    ap.add_argument("--workload", choices=list(WORKLOADS), default="crops8")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "enhance_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
