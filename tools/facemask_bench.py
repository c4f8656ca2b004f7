"""Benchmark of the face masks (rtd_facemask_apply, csrc/facemask.hip) on 8 x 1080p device frames of seeded noise with 2 faces of
120 x 120 each (padded: 168 x 168), per mask style.

    python tools/facemask_bench.py calls [--calls 100] [--out profiles/facemask_bench.json]
        per style the whole synchronous call on device frames (host clock around the call: medians of five rounds after warm-up, the
        per-round lists kept); alternating with them in the same process the comparator: what a masking host loop must pay AT LEAST on the
        same frames, `.cpu().numpy()` of each plus the upload back and a synchronise.  cv2 is not installed here, so the comparator
        holds no masking at all: it understates the reference.  Also the gray plane of one frame (rtd_facemask_gray).
    rocprofv3 --kernel-trace --stats -d DIR -o fm --output-format csv -- python tools/facemask_bench.py run --calls 20
        the run to profile (a run of its own: tracing slows the host): every style in turn
    python tools/facemask_bench.py kernels --stats DIR/fm_kernel_stats.csv [--out profiles/facemask_bench.json]
        kernel time per launch from that file
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
FACES = [(400, 300, 120, 120), (1200, 600, 120, 120)]
BLUR_STRENGTH, BLOCKS = 25, 10
STYLES = ("gaussian_blur", "adaptive_blur", "pixelate", "black_box")
KERNELS = ("facemask_blur_rows", "facemask_blur_cols", "facemask_pix_small", "facemask_pix_nearest", "facemask_box", "facemask_gray")


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

    from tests import face_ref as ref
    from telescope_cam_detection_amd import face_masker as fm
    frames = [ref.noise(60 + i, H, W) for i in range(N)]
    dev = [torch.from_numpy(f.copy()).cuda() for f in frames]
    masker = fm.FaceMasker(blur_strength=BLUR_STRENGTH, pixelate_blocks=BLOCKS, device=0, detector=lambda g: FACES)
    be = masker._backend(dev[0])
    rows = {s: [r for i in range(N) for r in masker._face_rows(i, (H, W, 3), FACES, s)] for s in STYLES}
    torch.cuda.synchronize()
    return ref, fm, masker, be, frames, dev, rows


def cmd_calls(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    ref, fm, masker, be, frames, dev, rows = setup()
    ptrs, shapes = [d.data_ptr() for d in dev], [(H, W, 3)] * N

    def call(style):
        rc = be.apply_raw(ptrs, shapes, True, rows[style])     # in place, again and again: the cost does not depend on the content
        assert rc == 0, rc

    def comparator():
        host = [d.cpu().numpy() for d in dev]
        up = [torch.from_numpy(h).to("cuda") for h in host]
        torch.cuda.synchronize()
        return up

    for s in STYLES:                                           # what is timed computes the restatement
        got = masker.apply_mask(dev[0], FACES, s).cpu().numpy()
        assert (got == ref.apply_mask(frames[0], FACES, s, BLUR_STRENGTH, BLOCKS)).all(), s
    gray = lambda: be.gray(dev[0])
    for _ in range(3):
        for s in STYLES:
            call(s)
        comparator(), gray()
    rounds, per = 5, max(a.calls // 5, 1)
    ours, theirs, grays = {s: [] for s in STYLES}, [], []
    for _ in range(rounds):                                    # the sides alternate so that all see the same machine load
        for s in STYLES:
            ours[s].append(timed(lambda: call(s), per))
        theirs.append(timed(comparator, max(per // 4, 1)))
        grays.append(timed(gray, per))
    r3 = lambda v: [round(x, 3) for x in v]
    res = {"frames": N, "hw": [H, W], "faces_per_frame": len(FACES), "face": [120, 120], "padded": [168, 168], "blur_strength": BLUR_STRENGTH,
           "adaptive_k": fm.adaptive_k(BLUR_STRENGTH, 120, 120, H, W), "blocks": BLOCKS, "plan": fm.plan(shapes, rows["gaussian_blur"])["tiles"],
           "apply_ms": {s: med(ours[s]) for s in STYLES}, "apply_ms_rounds": {s: r3(ours[s]) for s in STYLES},
           "comparator": "d.cpu().numpy() of the 8 frames + torch.from_numpy(h).to(device) of each + synchronize: the least a host loop pays, "
                         "with NO masking in it (cv2 is not installed): it understates the reference",
           "comparator_ms": med(theirs), "comparator_ms_rounds": r3(theirs),
           "gray_one_frame_ms": med(grays), "gray_one_frame_ms_rounds": r3(grays)}
    print(json.dumps(res), flush=True)
    masker.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    ref, fm, masker, be, frames, dev, rows = setup()
    ptrs, shapes = [d.data_ptr() for d in dev], [(H, W, 3)] * N
    try:
        for _ in range(a.calls):
            for s in STYLES:
                rc = be.apply_raw(ptrs, shapes, True, rows[s])
                assert rc == 0, rc
            be.gray(dev[0])
        print(json.dumps({"calls": a.calls}))
    finally:
        masker.close()


def cmd_kernels(a):
    out = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r.get("Name", ""):
                    out[k] = {"launches": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                              "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    out["note"] = ("per launch; a launch covers the 16 faces of the call (168 x 168 pixels each); blur_rows / blur_cols hold the launches of "
                   "gaussian_blur (k 25) and adaptive_blur (k 27) together")
    print(json.dumps(out, indent=1))
    merge(a.out, {"kernels": out})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels"])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "facemask_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
