"""Benchmark of the frame ingest (rtd_ingest_convert, csrc/ingest.hip) on 8 x 1080p NV12 frames of seeded content
(tests/yuv_ref.py planes).

    python tools/ingest_bench.py calls [--calls 100] [--out profiles/ingest_bench.json]
        the whole synchronous call from host frames and from device frames (host clock around the call: medians of five rounds, the
        per-round lists kept); alternating with them in the same process the comparator the reference's capture class amounts to,
        `torch.from_numpy(bgr).to(device)` for the same 8 frames as bgr24 plus a synchronise, and a torch device-to-device copy that
        moves the kernel's byte count (the bandwidth yardstick, timed with events and with the host clock).
    rocprofv3 --kernel-trace --stats -d DIR -o ing --output-format csv -- python tools/ingest_bench.py run --calls 20
        the run to profile (a run of its own: tracing slows the host); device frames, so nothing but the kernel and the table upload
    python tools/ingest_bench.py kernels --stats DIR/ing_kernel_stats.csv [--out profiles/ingest_bench.json]
        kernel time from that file against the bytes of the shapes: 1.5 read + 3 written per pixel

The resize stage (rtd_ingest_convert_resize), 8 NV12 frames to 1280 x 720, `--case area` (2560 x 1440, the 2 x 2 mean) or `--case linear`
(1920 x 1080, the tables); written to profiles/ingest_resize_bench.json:

    python tools/ingest_bench.py resize-calls [--calls 100]
        per case the fused call from device and from host frames, the call that also writes the native frames (convert kernel, then
        the BGR resize kernel), and alternating with them the yardstick: rtd_ingest_convert of the same native frames
    rocprofv3 --kernel-trace --stats -d DIR -o rs --output-format csv -- python tools/ingest_bench.py resize-run --case area --calls 20
        the run to profile, one case per run: yardstick, fused and native calls on device frames
    python tools/ingest_bench.py resize-kernels --case area --stats DIR/rs_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N = 1080, 1920, 8
KERNEL_BYTES = N * H * W * 9 // 2      # 1.5 read + 3 written per pixel
HBM_PEAK_GBS = 8000.0                  # MI355X HBM3E peak


def scene():
    """(packed NV12 host frames, their BGR arrays by the restatement)"""
    from tests import yuv_ref as ref
    frames, bgr = [], []
    for i in range(N):
        Y, U, V = ref.planes(40 + i, H, W)
        frames.append(ref.pack(Y, U, V, "nv12")[0])
        bgr.append(ref.planes_to_bgr(Y, U, V))
    return frames, bgr


def merge(path, update):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.update(update)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def timed(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e3


def med(v):
    return round(sorted(v)[len(v) // 2], 3)


def setup():
    import torch

    from telescope_cam_detection_amd import ingest
    frames, bgr = scene()
    be = ingest.FrameIngest(0)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    outs = [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(N)]
    optrs = [o.data_ptr() for o in outs]
    hdesc = [ingest.tight_frame(f.ctypes.data, H, W, 0) for f in frames]
    ddesc = [ingest.tight_frame(d.data_ptr(), H, W, 0) for d in dev]
    torch.cuda.synchronize()
    return be, frames, bgr, dev, outs, optrs, hdesc, ddesc


def cmd_calls(a):
    import torch

    from telescope_cam_detection_amd import ingest
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    be, frames, bgr, dev, outs, optrs, hdesc, ddesc = setup()

    def ok(rc):
        assert rc == 0, rc

    from_host = lambda: ok(be.convert_raw(hdesc, False, optrs))
    from_dev = lambda: ok(be.convert_raw(ddesc, True, optrs))

    def comparator():
        up = [torch.from_numpy(b).to("cuda") for b in bgr]
        torch.cuda.synchronize()
        return up

    src = torch.empty(KERNEL_BYTES // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy_host_clock():
        dst.copy_(src)
        torch.cuda.synchronize()

    def copy_events(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    from_host()
    assert all((o.cpu().numpy() == b).all() for o, b in zip(outs, bgr)), "the call does not compute the restatement"
    for _ in range(3):
        from_host(), from_dev(), comparator(), copy_host_clock()
    rounds, per = 5, max(a.calls // 5, 1)
    host, devc, theirs, cp_host, cp_ev = [], [], [], [], []
    for _ in range(rounds):                   # the sides alternate so that all see the same machine load
        host.append(timed(from_host, per))
        devc.append(timed(from_dev, per))
        theirs.append(timed(comparator, max(per // 2, 1)))
        cp_host.append(timed(copy_host_clock, per))
        cp_ev.append(copy_events(per))
    r3 = lambda v: [round(x, 3) for x in v]
    res = {"frames": N, "hw": [H, W], "layout": "nv12", "tile": list(ingest.tile_hw()),
           "nv12_bytes": N * H * W * 3 // 2, "bgr_bytes": N * H * W * 3, "kernel_bytes_read_plus_written": KERNEL_BYTES,
           "convert_from_host_ms": med(host), "convert_from_host_ms_rounds": r3(host),
           "convert_from_device_ms": med(devc), "convert_from_device_ms_rounds": r3(devc),
           "comparator": "torch.from_numpy(bgr).to(device) for the same 8 frames as bgr24 (pageable memory, as the reference) + synchronize",
           "comparator_ms": med(theirs), "comparator_ms_rounds": r3(theirs),
           "copy_yardstick": "torch device-to-device copy of kernel_bytes / 2 (so that read + written equals the kernel's)",
           "copy_ms_host_clock": med(cp_host), "copy_ms_host_clock_rounds": r3(cp_host),
           "copy_ms_events": med(cp_ev), "copy_ms_events_rounds": r3(cp_ev)}
    print(json.dumps(res), flush=True)
    be.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    be, frames, bgr, dev, outs, optrs, hdesc, ddesc = setup()
    try:
        for _ in range(a.calls):
            rc = be.convert_raw(ddesc, True, optrs)
            assert rc == 0, rc
        print(json.dumps({"calls": a.calls}))
    finally:
        be.close()


def cmd_kernels(a):
    rows = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "ingest_kernel" in name:
                avg_us = float(r["AverageNs"]) / 1e3
                rows["ingest_kernel"] = {"calls": int(r["Calls"]), "avg_us": round(avg_us, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                                         "bytes_read_plus_written": KERNEL_BYTES, "gbytes_per_s": round(KERNEL_BYTES / avg_us / 1e3, 1),
                                         "share_of_hbm_peak": round(KERNEL_BYTES / avg_us / 1e3 / HBM_PEAK_GBS, 3)}
    rows["us_at_hbm_peak"] = round(KERNEL_BYTES / HBM_PEAK_GBS / 1e3, 1)
    print(json.dumps(rows, indent=1))
    merge(a.out, {"kernels": rows})


# ---- the resize stage ---------------------------------------------------------------------------------------------------------------------
RESIZE_CASES = {"area": (1440, 2560), "linear": (1080, 1920)}
OUT_HW = (720, 1280)
RESIZE_OUT = os.path.join("profiles", "ingest_resize_bench.json")


def resize_setup(case, check=True):
    import torch

    from telescope_cam_detection_amd import ingest
    from tests import resize_ref, yuv_ref
    h, w = RESIZE_CASES[case]
    frames = [yuv_ref.pack(*yuv_ref.planes(60 + i, h, w), "nv12")[0] for i in range(N)]
    be = ingest.FrameIngest(0)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    outs = [torch.empty((*OUT_HW, 3), dtype=torch.uint8, device="cuda") for _ in range(N)]
    native = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(N)]
    hdesc = [ingest.tight_frame(f.ctypes.data, h, w, 0) for f in frames]
    ddesc = [ingest.tight_frame(d.data_ptr(), h, w, 0) for d in dev]
    hw = list(OUT_HW) * N
    optrs, nptrs = [o.data_ptr() for o in outs], [o.data_ptr() for o in native]

    def ok(rc):
        assert rc == 0, (rc, be._fn("last_error")(be._h))

    calls = {"fused_from_device": lambda: ok(be.resize_raw(ddesc, True, hw, optrs)),
             "fused_from_host": lambda: ok(be.resize_raw(hdesc, False, hw, optrs)),
             "with_native_from_device": lambda: ok(be.resize_raw(ddesc, True, hw, optrs, nptrs)),
             "yardstick_convert_from_device": lambda: ok(be.convert_raw(ddesc, True, nptrs)),
             "yardstick_convert_from_host": lambda: ok(be.convert_raw(hdesc, False, nptrs))}
    if check:                                 # one frame of each call against the restatement (the tests hold the rest)
        want = resize_ref.to_bgr_resized(frames[N - 1], h, w, *OUT_HW)
        for name in ("fused_from_device", "fused_from_host", "with_native_from_device"):
            outs[N - 1].zero_()
            calls[name]()
            assert (outs[N - 1].cpu().numpy() == want).all(), f"{name} does not compute the restatement"
        assert (native[N - 1].cpu().numpy() == yuv_ref.to_bgr(frames[N - 1], h, w)).all()
    torch.cuda.synchronize()
    return be, calls, (h, w)


def cmd_resize_calls(a):
    import torch

    from telescope_cam_detection_amd import ingest
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    res = {"frames": N, "out_hw": list(OUT_HW), "layout": "nv12", "tile_out_hw": list(ingest.resize_tile_hw()),
           "method": "host clock around the synchronous call; medians of five rounds after warm-up, the calls of a case alternating in one process"}
    for case in ([a.case] if a.case else list(RESIZE_CASES)):
        be, calls, (h, w) = resize_setup(case)
        for _ in range(3):
            for fn in calls.values():
                fn()
        rounds, per = 5, max(a.calls // 5, 1)
        t = {k: [] for k in calls}
        for _ in range(rounds):               # the sides alternate so that all see the same machine load
            for k, fn in calls.items():
                t[k].append(timed(fn, per if "host" not in k else max(per // 4, 1)))
        res[case] = {"source_hw": [h, w], "area2": ingest.resize_is_area2(w, h, OUT_HW[1], OUT_HW[0]), "nv12_bytes": N * h * w * 3 // 2,
                     "out_bytes": N * OUT_HW[0] * OUT_HW[1] * 3, "native_bytes": N * h * w * 3}
        for k, v in t.items():
            res[case][k + "_ms"] = med(v)
            res[case][k + "_ms_rounds"] = [round(x, 3) for x in v]
        be.close()
    print(json.dumps(res), flush=True)
    merge(a.out if a.out != os.path.join("profiles", "ingest_bench.json") else RESIZE_OUT, {"calls": res})


def cmd_resize_run(a):
    be, calls, _ = resize_setup(a.case or "area", check=False)
    try:
        for name in ("yardstick_convert_from_device", "fused_from_device", "with_native_from_device"):
            for _ in range(a.calls):
                calls[name]()
        print(json.dumps({"case": a.case or "area", "calls": a.calls}))
    finally:
        be.close()


def cmd_resize_kernels(a):
    import re
    case = a.case or "area"
    h, w = RESIZE_CASES[case]
    src, out, nat = N * h * w * 3 // 2, N * OUT_HW[0] * OUT_HW[1] * 3, N * h * w * 3
    moved = {"ingest_kernel": src + nat, "resize_kernel_yuv": src + out, "resize_kernel_bgr": nat + out}
    rows = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            m = re.search(r"resize_kernel(?:ILi|<\D*)(\d)", name)
            key = "ingest_kernel" if "ingest_kernel" in name else (("resize_kernel_yuv", "resize_kernel_bgr")[int(m.group(1))] if m else None)
            if key:
                avg_us = float(r["AverageNs"]) / 1e3
                rows[key] = {"calls": int(r["Calls"]), "avg_us": round(avg_us, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                             "max_us": round(float(r["MaxNs"]) / 1e3, 2), "stddev_us": round(float(r.get("StdDev", 0) or 0) / 1e3, 2),
                             "bytes_read_plus_written": moved[key], "gbytes_per_s": round(moved[key] / avg_us / 1e3, 1)}
    print(json.dumps(rows, indent=1))
    merge(a.out if a.out != os.path.join("profiles", "ingest_bench.json") else RESIZE_OUT, {"kernels_" + case: rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels", "resize-calls", "resize-run", "resize-kernels"])
    ap.add_argument("--case", choices=sorted(RESIZE_CASES))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "ingest_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels, "resize-calls": cmd_resize_calls, "resize-run": cmd_resize_run,
     "resize-kernels": cmd_resize_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
