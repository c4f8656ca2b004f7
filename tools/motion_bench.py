"""Micro-benchmark of the empty-frame filter (rtd_motion_check, csrc/motion.hip): 8 cameras x 1080p BGR frames per call.

Every slot is warmed up first (its first frame allocates its state), then `--calls` synchronous calls are timed with a host clock (the
call returns when the areas are on the host).  Bandwidth = 8 * (3 + 2) * H * W bytes (BGR in, state read + written) over the time.
Legs: device frames at k = 21 (the reference's default), host frames at k = 21 (pinned staging + one upload per call included), device
frames at k = 5 and k = 63.  Kernel-only time: run under `rocprofv3 --kernel-trace --stats` and read motion_kernel's row.
    python tools/motion_bench.py [--calls 300]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def leg(k, on_device, calls, H=1080, W=1920, n=8):
    import torch

    from telescope_cam_detection_amd.motion import DeviceBackend
    from telescope_cam_detection_amd.synth import scene_frame
    frames = [scene_frame(50 + i, H, W) for i in range(n)]
    args = [torch.from_numpy(f).cuda() for f in frames] if on_device else frames
    torch.cuda.synchronize()
    be = DeviceBackend(0, k)
    try:
        slots = list(range(n))
        for _ in range(5):
            be.check(args, on_device, slots, 25)
        t0 = time.perf_counter()
        for _ in range(calls):
            be.check(args, on_device, slots, 25)
        us = (time.perf_counter() - t0) / calls * 1e6
    finally:
        be.close()
    nbytes = n * (3 + 2) * H * W
    return {"k": k, "frames": "device" if on_device else "host", "n": n, "hw": [H, W], "us_per_call": round(us, 1),
            "gbytes_per_s_call": round(nbytes / us / 1e3, 1), "bytes_per_call": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    for k, dev in ((21, True), (21, False), (5, True), (63, True)):
        print(json.dumps(leg(k, dev, a.calls)), flush=True)


if __name__ == "__main__":
    main()
