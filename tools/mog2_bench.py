"""Micro-benchmark of the motion filter (rtd_mog2_apply, csrc/mog2.hip): one 1080p BGR frame per call with n boxes (n model updates).

The model is warmed up first (its first frame allocates it), then `--calls` synchronous calls are timed with a host clock (the call
returns when the counts are on the host).  The 1080p BGR model (207 MB) fits the 256 MB Infinity Cache, so back-to-back calls read
it from there; the `cold` legs overwrite a 512 MB buffer before every call (outside the timed window), as the detector's own traffic
between two frames of a camera does.  State-pass bytes = chunks * H * W * (2 * 25 * 4 + 2 + 3 + 4): the model read and written
once per chunk of 32 updates, the modes-used byte read and written, the frame read, the foreground word written.
Legs: a device frame with n = 1, 8 and 32 boxes of 256 x 192, warm and cold; a host frame with n = 8 (pinned staging + one upload per
call included).
Kernel-only time: run under `rocprofv3 --kernel-trace --stats` and read the rows of mog2_state_kernel and mog2_roi_kernel.
    python tools/mog2_bench.py [--calls 200]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def boxes(n, H, W, bw=256, bh=192):
    out = []
    for i in range(n):
        x = (i * 397) % (W - bw)
        y = (i * 211) % (H - bh)
        out.append((x, y, x + bw, y + bh))
    return out


def leg(n, on_device, calls, cold=False, H=1080, W=1920, k=21):
    import torch

    from telescope_cam_detection_amd.motion_filter import DeviceBackend
    from telescope_cam_detection_amd.synth import scene_frame
    frame = scene_frame(77, H, W)
    arg = torch.from_numpy(frame).cuda() if on_device else frame
    torch.cuda.synchronize()
    be = DeviceBackend(0, 500, 16, True)
    rects = boxes(n, H, W)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda") if cold else None
    try:
        for _ in range(5):
            be.apply(arg, on_device, rects, k)
        total = 0.0
        for _ in range(calls):
            if cold:
                flush.fill_(1)
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            be.apply(arg, on_device, rects, k)
            total += time.perf_counter() - t0
        us = total / calls * 1e6
    finally:
        be.close()
    chunks = (n + 31) // 32
    state_bytes = chunks * H * W * (2 * 25 * 4 + 2 + 3 + 4)
    return {"n": n, "frames": "device" if on_device else "host", "cache": "cold" if cold else "warm", "hw": [H, W], "k": k, "us_per_call": round(us, 1),
            "state_pass_bytes": state_bytes, "gbytes_per_s_state_over_call": round(state_bytes / us / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    for n, dev, cold in ((1, True, False), (8, True, False), (32, True, False), (8, False, False), (1, True, True), (8, True, True),
                         (32, True, True)):
        print(json.dumps(leg(n, dev, a.calls, cold)), flush=True)


if __name__ == "__main__":
    main()
