"""Benchmark of the overlay renderer (rtd_overlay_draw, csrc/overlay.hip) on 8 x 1080p BGR device frames (synth.scene_frame) with ten
web-style detections each, FakeRasteriser labels (tests/overlay_ref.py) so that no font enters the timing.

    python tools/overlay_bench.py calls [--calls 100] [--out profiles/overlay_bench.json]
        the whole synchronous draw call in place and out of place (host clock around the call: medians of five rounds, the per-round
        lists kept), and one MJPEG tick at quality 90 (draw + encode of all 8 frames) beside the comparator of DESIGN.md §11:
        `tensor.cpu().numpy()` + Pillow's JPEG encoder per frame.  The comparator draws NOTHING (cv2 is absent here), so it understates
        what the reference does per tick.
    rocprofv3 --kernel-trace --stats -d DIR -o ovl --output-format csv -- python tools/overlay_bench.py run --calls 20
        the run to profile (a run of its own: tracing slows the host); out of place, so the copies are in it
    python tools/overlay_bench.py kernels --stats DIR/ovl_kernel_stats.csv [--out profiles/overlay_bench.json]
        kernel time from that file against the bytes of the touched tiles (read once and, at most, written once)
"""
import argparse
import csv
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N, DETS, QUALITY = 1080, 1920, 8, 10, 90
HBM_PEAK_GBS = 8000.0            # MI355X HBM3E peak


def scene(n=N):
    """(device frames, detection results, primitive lists, masks)"""
    import numpy as np
    import torch

    from telescope_cam_detection_amd import overlay as ov
    from telescope_cam_detection_amd.synth import scene_frame
    from tests.overlay_ref import FakeRasteriser
    rng = np.random.default_rng(1)
    names = ["person", "cat", "dog", "bird", "car", "deer"]
    results = []
    for _ in range(n):
        dets = []
        for _ in range(DETS):
            x1, y1 = float(rng.integers(0, W - 400)), float(rng.integers(30, H - 300))
            dets.append({"class_name": names[int(rng.integers(0, len(names)))], "confidence": float(rng.random()),
                         "bbox": {"x1": x1, "y1": y1, "x2": x1 + float(rng.integers(60, 400)), "y2": y1 + float(rng.integers(60, 300))}})
        results.append({"detections": dets, "total_latency_ms": 12.0})
    ras = FakeRasteriser()
    prims, masks = ov.lower([ov.plan_web(r, ras) for r in results], ov.MaskCache(ras))
    dev = [torch.from_numpy(scene_frame(40 + i, H, W)).cuda() for i in range(n)]
    torch.cuda.synchronize()
    return dev, results, prims, masks


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


def cmd_calls(a):
    import numpy as np
    import torch

    from telescope_cam_detection_amd import overlay as ov
    from tests.overlay_ref import FakeRasteriser, tiles_touched
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev, results, prims, masks = scene()
    be = ov.DeviceBackend(0)
    r = ov.OverlayRenderer(0, rasteriser=FakeRasteriser(), backend=be)
    th, tw, _ = be.tiles()
    ptrs, shapes = [d.data_ptr() for d in dev], [tuple(d.shape) for d in dev]
    outs = [torch.empty_like(d) for d in dev]
    optrs = [o.data_ptr() for o in outs]
    work = [d.clone() for d in dev]
    wptrs = [w_.data_ptr() for w_ in work]
    torch.cuda.synchronize()

    def comparator():
        out = []
        for t in dev:
            a_ = t.cpu().numpy()
            if Image is not None:
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(a_[:, :, ::-1])).save(buf, "JPEG", quality=QUALITY)
                out.append(buf.getvalue())
        return out

    rounds, per = 5, max(a.calls // 5, 1)
    inplace, outplace, tick, theirs = [], [], [], []
    for _ in range(3):
        be.draw_raw(wptrs, shapes, True, prims, masks, wptrs)
        be.draw_raw(ptrs, shapes, True, prims, masks, optrs)
        r.mjpeg_tick(dev, results, QUALITY)
    for _ in range(rounds):                   # the sides alternate so that all see the same machine load
        inplace.append(timed(lambda: be.draw_raw(wptrs, shapes, True, prims, masks, wptrs), per))
        outplace.append(timed(lambda: be.draw_raw(ptrs, shapes, True, prims, masks, optrs), per))
        tick.append(timed(lambda: r.mjpeg_tick(dev, results, QUALITY), max(per // 2, 1)))
        theirs.append(timed(comparator, max(per // 10, 1)))
    tiles = int(sum(tiles_touched(p, s, (th, tw)) for p, s in zip(prims, shapes)))
    res = {"frames": N, "hw": [H, W], "detections_per_frame": DETS, "primitives": int(sum(len(p) for p in prims)), "mask_bytes": int(masks.size),
           "tile": [th, tw], "tiles_launched": be.tiles()[2], "tiles_touched": tiles, "tiles_of_the_frames": N * -(-H // th) * -(-W // tw),
           "draw_inplace_ms": med(inplace), "draw_inplace_ms_rounds": [round(v, 3) for v in inplace],
           "draw_out_of_place_ms": med(outplace), "draw_out_of_place_ms_rounds": [round(v, 3) for v in outplace],
           "mjpeg_tick_ms": med(tick), "mjpeg_tick_ms_rounds": [round(v, 3) for v in tick], "quality": QUALITY,
           "comparator": ("tensor.cpu().numpy() + Pillow (libjpeg) per frame, one thread; it draws nothing (no cv2 here), so it understates the reference"
                          if Image is not None else "Pillow is missing: tensor.cpu().numpy() alone"),
           "comparator_ms": med(theirs), "comparator_ms_rounds": [round(v, 3) for v in theirs]}
    print(json.dumps(res), flush=True)
    r.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    import torch

    from telescope_cam_detection_amd import overlay as ov
    dev, _, prims, masks = scene()
    be = ov.DeviceBackend(0)
    ptrs, shapes = [d.data_ptr() for d in dev], [tuple(d.shape) for d in dev]
    outs = [torch.empty_like(d) for d in dev]
    torch.cuda.synchronize()
    try:
        for _ in range(a.calls):
            rc = be.draw_raw(ptrs, shapes, True, prims, masks, [o.data_ptr() for o in outs])
            assert rc == 0, rc
        print(json.dumps({"calls": a.calls, "tiles": be.tiles()[2]}))
    finally:
        be.close()


def cmd_kernels(a):
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f).get("calls", {})
    rows = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "overlay_kernel" in name:
                avg_us = float(r["AverageNs"]) / 1e3
                rows["overlay_kernel"] = {"calls": int(r["Calls"]), "avg_us": round(avg_us, 2)}
                if doc.get("tiles_touched"):
                    th, tw = doc["tile"]
                    b = doc["tiles_touched"] * th * tw * 3
                    rows["overlay_kernel"].update({"tile_bytes": b, "gbytes_per_s_read_once": round(b / avg_us / 1e3, 1)})
            elif "copy" in name.lower():                # the device-to-device copies, when the runtime runs them as kernels
                rows.setdefault("copy_kernels", []).append({"name": name[:60], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)})
    copy_bytes = 2 * N * H * W * 3
    rows["copy_bytes_read_plus_written"] = copy_bytes
    rows["copy_us_at_hbm_peak"] = round(copy_bytes / HBM_PEAK_GBS / 1e3, 1)
    if doc.get("draw_out_of_place_ms") and doc.get("draw_inplace_ms"):
        rows["copy_ms_by_difference_of_the_calls"] = round(doc["draw_out_of_place_ms"] - doc["draw_inplace_ms"], 3)
    print(json.dumps(rows, indent=1))
    merge(a.out, {"kernels": rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels"])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "overlay_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
