"""Benchmark of the JPEG encoder (rtd_jpeg_encode, csrc/jpeg.hip) on 1080p BGR device frames (synth.scene_frame, quality 90), beside
what the reference does for the same frames: `tensor.cpu().numpy()` followed by libjpeg on one thread (Pillow's encoder, which is
cv2.imencode's; src/snapshot_saver.py add_frame_to_buffer runs it per frame).

    python tools/jpeg_bench.py calls [--calls 100] [--out profiles/jpeg_bench.json]
        whole synchronous calls of 1 and of 8 device frames (host clock around a call that ends with the bytes on the host), bytes
        returned, and the comparator on the same frames in the same run; without Pillow the comparator is the D2H copy alone
    rocprofv3 --kernel-trace --stats -d DIR -o n8 --output-format csv -- python tools/jpeg_bench.py run --frames 8 --calls 20
        the run to profile (a run of its own: tracing slows the host)
    python tools/jpeg_bench.py kernels --stats DIR/n8_kernel_stats.csv --frames 8 [--out profiles/jpeg_bench.json]
        kernel time per pass from that file, over the bytes each pass has to move (computed from the shapes below), merged into --out

Bytes a pass has to move, per frame of H x W x 3 with B = 6 ceil(H/16) ceil(W/16) blocks, U unstuffed and S stuffed scan bytes:
transform 3 H W + 132 B (blocks and one side word each); size 8 B; write 136 B + U; stuff: count U, scatter U + S.  U and S are counted
in the files the `calls` leg got back.  The rounds of that leg alternate the two sides, but the machine's CPUs are shared with other
work: read the per-round lists, not only the medians.
"""
import argparse
import csv
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, QUALITY = 1080, 1920, 90
PASSES = {"transform_kernel": "transform", "size_kernel": "size", "chunk_scan_kernel": "size_scan", "write_kernel": "write",
          "stuff_kernel<false>": "stuff_count", "stuff_scan_kernel": "stuff_scan", "stuff_kernel<true>": "stuff_scatter",
          "stuff_kernelILb0": "stuff_count", "stuff_kernelILb1": "stuff_scatter"}


def device_frames(n):
    import torch

    from telescope_cam_detection_amd.synth import scene_frame
    frames = [scene_frame(40 + i, H, W) for i in range(n)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    return dev


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


def scan_sizes(files):
    """(stuffed, unstuffed) bytes of the entropy-coded segments: what lies between the SOS header and EOI; without restart markers every
    0xFF in it is followed by its stuffed 0x00"""
    stuffed = unstuffed = 0
    for f in files:
        i = f.index(b"\xff\xda")
        scan = f[i + 2 + int.from_bytes(f[i + 2:i + 4], "big"):-2]
        stuffed += len(scan)
        unstuffed += len(scan) - scan.count(b"\xff\x00")
    return stuffed, unstuffed


def timed(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e3


def cmd_calls(a):
    import numpy as np
    import torch

    from telescope_cam_detection_amd.jpeg import DeviceBackend
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    dev = device_frames(8)
    be = DeviceBackend(0)

    def reference(frames):
        out = []
        for t in frames:
            a_ = t.cpu().numpy()
            if Image is not None:
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(a_[:, :, ::-1])).save(buf, "JPEG", quality=QUALITY)
                out.append(buf.getvalue())
        return out

    res = {"hw": [H, W], "quality": QUALITY, "calls": a.calls, "comparator": "tensor.cpu().numpy() + Pillow (libjpeg) per frame, one thread"
           if Image is not None else "Pillow is missing on this machine: tensor.cpu().numpy() alone"}
    try:
        for n in (1, 8):
            fr = dev[:n]
            for _ in range(5):
                got = be.encode(fr, True, QUALITY)
            ref_out = reference(fr)
            if ref_out:
                assert got == ref_out, "the encoder's bytes differ from the comparator's"
            # alternate the two sides in rounds so that both see the same machine load
            ours, theirs = [], []
            rounds = 5
            for _ in range(rounds):
                ours.append(timed(lambda: be.encode(fr, True, QUALITY), max(a.calls // rounds, 1)))
                theirs.append(timed(lambda: reference(fr), max(a.calls // (rounds * 5), 1)))
            stuffed, unstuffed = scan_sizes(got)
            res[f"n{n}"] = {"frames": n, "bytes_returned": sum(len(g) for g in got), "raw_bytes": n * H * W * 3,
                            "scan_bytes_stuffed": stuffed, "scan_bytes_unstuffed": unstuffed,
                            "call_ms": round(sorted(ours)[rounds // 2], 3), "call_ms_rounds": [round(v, 3) for v in ours],
                            "comparator_ms": round(sorted(theirs)[rounds // 2], 3), "comparator_ms_rounds": [round(v, 3) for v in theirs]}
            print(json.dumps({f"n{n}": res[f"n{n}"]}), flush=True)
    finally:
        be.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    from telescope_cam_detection_amd.jpeg import DeviceBackend
    dev = device_frames(a.frames)
    be = DeviceBackend(0)
    try:
        for _ in range(a.calls):
            out = be.encode(dev, True, QUALITY)
    finally:
        be.close()
    print(json.dumps({"frames": a.frames, "calls": a.calls, "bytes": sum(len(o) for o in out)}))


def cmd_kernels(a):
    n = a.frames
    blocks = n * 6 * ((H + 15) // 16) * ((W + 15) // 16)
    calls_doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            calls_doc = json.load(f).get("calls", {})
    S = calls_doc.get(f"n{n}", {}).get("scan_bytes_stuffed")      # from the `calls` leg of the same --out file
    U = calls_doc.get(f"n{n}", {}).get("scan_bytes_unstuffed")
    need = {"transform": n * 3 * H * W + 132 * blocks, "size": 8 * blocks}
    if S:
        need.update({"write": 136 * blocks + U, "stuff_count": U, "stuff_scatter": U + S})
    rows = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            for key, label in PASSES.items():
                if key in name:
                    avg_us = float(r["AverageNs"]) / 1e3
                    rows[label] = {"calls": int(r["Calls"]), "avg_us": round(avg_us, 2)}
                    if label in need:
                        rows[label]["bytes"] = need[label]
                        rows[label]["gbytes_per_s"] = round(need[label] / avg_us / 1e3, 1)
    rows["sum_avg_us"] = round(sum(v["avg_us"] for v in rows.values()), 1)
    print(json.dumps(rows, indent=1))
    merge(a.out, {f"kernels_n{n}": rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels"])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "jpeg_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
