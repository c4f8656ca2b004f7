"""Benchmark of the YOLOX post-processing (rtd_yolox_post_run, csrc/yolox_post.hip) at A = 8400 anchors, C = 80 classes:
    b8_c100   8 images, about 100 candidates each      b8_c1000   8 images, about 1000 candidates each
    b1_c100   1 image                                   b1_c1000   1 image

    python tools/yolox_post_bench.py calls [--rounds 20] [--per 20] [--out profiles/yolox_post_bench.json]
        per workload: the whole call (one memset, four launches) between HIP events on torch's stream, `per` calls back to back per round,
        median and range over the rounds after a warm-up; and, in the same process, a pure-torch restatement on the same device
        (threshold, sort, one [m][m] IoU matrix per image, then the greedy walk on the host after one download).  torchvision does not
        exist on this stack, so that yardstick is what a user could write without it, not what upstream runs: a weak one.
    rocprofv3 --kernel-trace --stats -d DIR -o yp --output-format csv -- python tools/yolox_post_bench.py run --workload b8_c100 --calls 50
        the run to profile (one workload per run, so that a kernel's average belongs to one shape)
    python tools/yolox_post_bench.py kernels --workload b8_c100 --stats DIR/yp_kernel_stats.csv [--out profiles/yolox_post_bench.json]
        the four kernel times from that file; the score pass against the n * A * (5 + C) * 4 bytes it must read and HBM's peak
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A, C = 8400, 80
CONF, NMS = 0.25, 0.45
HBM_PEAK_GBS = 8000.0            # MI355X HBM3E peak, the figure bench.py uses
WORKLOADS = {"b8_c100": (8, 20, 5), "b8_c1000": (8, 100, 10), "b1_c100": (1, 20, 5), "b1_c1000": (1, 100, 10)}      # images, objects, anchors per object


def scene(workload, seed=7):
    """[n][A][5 + C] fp32: per image `objects` boxes on a 640 x 640 input, each seen by `dup` jittered anchors of one class, over a
    background that never passes"""
    n, objects, dup = WORKLOADS[workload]
    rng = np.random.default_rng(seed)
    pred = np.empty((n, A, 5 + C), np.float32)
    for p in pred:
        p[:, 0:2] = rng.uniform(20, 620, (A, 2))
        p[:, 2:4] = rng.uniform(8, 120, (A, 2))
        p[:, 4] = rng.uniform(0.0, 0.3, A)
        p[:, 5:] = rng.uniform(0.0, 0.3, (A, C))
        where = rng.permutation(A)[:objects * dup].reshape(objects, dup)
        for o in range(objects):
            centre, size, cls = rng.uniform(60, 580, 2), rng.uniform(20, 120, 2), int(rng.integers(0, C))
            for a in where[o]:
                p[a, 0:2] = centre + rng.uniform(-4, 4, 2)
                p[a, 2:4] = size * rng.uniform(0.85, 1.15, 2)
                p[a, 4] = rng.uniform(0.7, 0.99)
                p[a, 5 + cls] = rng.uniform(0.7, 0.99)
    return pred


def torch_restatement(pred, conf, nms):
    """per image the kept rows' anchors: class maximum, threshold, sort and the IoU matrix on the device, the greedy walk on the host"""
    import torch
    mats = []
    for p in pred:
        cconf, cid = p[:, 5:].max(1)
        score = p[:, 4] * cconf
        idx = torch.nonzero(score >= conf).flatten()
        order = torch.argsort(score[idx], descending=True, stable=True)
        idx = idx[order]
        b = p[idx]
        x1, y1, x2, y2 = b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
        area = (x2 - x1) * (y2 - y1)
        iw = (torch.minimum(x2[:, None], x2[None]) - torch.maximum(x1[:, None], x1[None])).clamp(min=0)
        ih = (torch.minimum(y2[:, None], y2[None]) - torch.maximum(y1[:, None], y1[None])).clamp(min=0)
        inter = iw * ih
        over = (inter / (area[:, None] + area[None] - inter) > nms) & (cid[idx][:, None] == cid[idx][None])
        mats.append((idx, over))
    out = []
    for idx, over in mats:
        idx, over = idx.cpu().numpy(), over.cpu().numpy()
        dead = np.zeros(len(idx), bool)
        kept = []
        for i in range(len(idx)):
            if not dead[i]:
                kept.append(int(idx[i]))
                dead[i + 1:] |= over[i, i + 1:]
        out.append(kept)
    return out


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


def cmd_calls(a):
    import time

    import torch

    from telescope_cam_detection_amd.yolox_detector import DeviceBackend
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    be = DeviceBackend(0, C, 8, A, 2048)
    res = {}
    try:
        for name in WORKLOADS:
            pred = torch.from_numpy(scene(name)).cuda()
            n = pred.shape[0]
            rows = torch.empty((n, be.max_candidates, 7), dtype=torch.float32, device="cuda")
            counts = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            call = lambda: be.run(pred, CONF, NMS, out=(rows, counts))
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            # the device rows against the yardstick's, so that both sides are known to do the same work
            got = [rows[i, :int(counts[i, 0])].cpu().numpy() for i in range(n)]
            want = torch_restatement(pred, CONF, NMS)
            assert [len(g) for g in got] == [len(w) for w in want], ([len(g) for g in got], [len(w) for w in want])
            device, yard = [], []
            for _ in range(max(a.rounds, 20)):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(a.per):
                    call()
                ev1.record()
                ev1.synchronize()
                device.append(ev0.elapsed_time(ev1) / a.per)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                torch_restatement(pred, CONF, NMS)
                yard.append((time.perf_counter() - t0) * 1e3)
            r = {"images": n, "anchors": A, "classes": C, "passed_per_image": [int(c) for c in counts[:, 1].cpu()], "kept_per_image": [int(c) for c in counts[:, 0].cpu()],
                 "calls_per_round": a.per, "rtd_yolox_post_run_device": summary(device),
                 "torch_restatement_host_clock": dict(summary(yard), note="threshold, sort and IoU matrix on the device, greedy walk on the host; "
                                                                          "includes its download and synchronisation; no torchvision on this stack")}
            res[name] = r
            print(json.dumps({name: r}), flush=True)
    finally:
        be.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    import torch

    from telescope_cam_detection_amd.yolox_detector import DeviceBackend
    be = DeviceBackend(0, C, 8, A, 2048)
    try:
        pred = torch.from_numpy(scene(a.workload)).cuda()
        for _ in range(a.calls):
            be.run(pred, CONF, NMS)
        torch.cuda.synchronize()
        print(json.dumps({"workload": a.workload, "calls": a.calls}))
    finally:
        be.close()


def cmd_kernels(a):
    n = WORKLOADS[a.workload][0]
    b = n * A * (5 + C) * 4                      # what the score pass must read; its candidate writes are a few KB
    rows = {"score_pass_bytes": b, "us_at_hbm_peak": round(b / HBM_PEAK_GBS / 1e3, 2), "hbm_peak_gbytes_per_s": HBM_PEAK_GBS}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            for k in ("yolox_score", "yolox_rank", "yolox_mask", "yolox_scan"):
                if k in name:
                    avg_us = float(r["AverageNs"]) / 1e3
                    rows[k] = {"calls": int(r["Calls"]), "avg_us": round(avg_us, 2)}
                    if k == "yolox_score":
                        gbs = b / avg_us / 1e3
                        rows[k].update(gbytes_per_s=round(gbs, 1), fraction_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
    print(json.dumps({a.workload: rows}, indent=1))
    merge(a.out, {"kernels": {a.workload: rows}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels"])
    ap.add_argument("--workload", choices=list(WORKLOADS), default="b8_c100")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--per", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "yolox_post_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
