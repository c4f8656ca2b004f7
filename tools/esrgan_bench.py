"""Benchmark of the Real-ESRGAN x4 crop upscaler (rtd_esrgan_upscale, csrc/esrgan.hip), 23 blocks, seeded weights, on four workloads:
    c128      one 128 x 128 crop
    c256      one 256 x 256 crop
    c128x8    eight 128 x 128 crops (one out of each of eight frames)
    c1080x640 one 1080 x 640 crop with the default tiling (tile 512, pad 10: 3 x 2 tiles)

    python tools/esrgan_bench.py calls [--calls 5] [--out profiles/esrgan_bench.json]
        per engine (f16x3, fp32) and workload: HIP-event time of the whole call on torch's stream, medians of five rounds (the lists are
        kept), beside the derived FLOP count and - f16x3 - the fraction of this device's measured fp16 MFMA rate (rtd_bench_mfma_rate, the
        in-library form of tools/mfma_rate_probe.hip) that three MFMAs per product amount to
    python tools/esrgan_bench.py conv [--out ...]
        the five conv shapes of a dense block on a 128 x 128 map through rtd_bench_conv (ReLU) and rtd_bench_conv_act (LeakyReLU):
        what the new epilogue costs
    rocprofv3 --kernel-trace --stats -d DIR -o esr --output-format csv -- python tools/esrgan_bench.py run --workload c128 --engine f16x3 --calls 5
    python tools/esrgan_bench.py kernels --workload c128 --engine f16x3 --calls 5 --stats DIR/esr_kernel_stats.csv [--out ...]
        per-kernel-name totals of that run, per call
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUM_BLOCK = 23
ENGINES = ("f16x3", "fp32")
# name: (frames, frame (h, w), rect, tile, tile_pad)
WORKLOADS = {
    "c128": (1, (360, 640), (100, 60, 228, 188), 512, 10),
    "c256": (1, (360, 640), (100, 60, 356, 316), 512, 10),
    "c128x8": (8, (360, 640), (100, 60, 228, 188), 512, 10),
    "c1080x640": (1, (720, 1280), (100, 40, 1180, 680), 512, 10),
}
MAC_DENSE = 9 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64)      # 239 616 per pixel and dense block
MAC_64 = 9 * 64 * 64


def macs_per_input_pixel(num_block=NUM_BLOCK, padded=False):
    """padded: what the kernels issue (conv_first reads 32 channels, conv_last writes 32; the 32-output convs still count their real N)"""
    first = 9 * (32 if padded else 3) * 64
    last = 16 * 9 * 64 * (32 if padded else 3)
    return first + 3 * num_block * MAC_DENSE + MAC_64 + 4 * MAC_64 + 16 * MAC_64 + 16 * MAC_64 + last


def tile_pixels(h, w, tile, pad):
    if tile <= 0:
        return h * w
    n = 0
    for y0 in range(0, h, tile):
        for x0 in range(0, w, tile):
            y1, x1 = min(y0 + tile, h), min(x0 + tile, w)
            n += (min(y1 + pad, h) - max(y0 - pad, 0)) * (min(x1 + pad, w) - max(x0 - pad, 0))
    return n


def scene(name):
    import torch

    from telescope_cam_detection_amd.synth import scene_frame
    n, (fh, fw), rect, _, _ = WORKLOADS[name]
    frames = [torch.from_numpy(scene_frame(40 + i, fh, fw)).cuda() for i in range(n)]
    torch.cuda.synchronize()
    return frames, [[rect] for _ in range(n)]


def make_upscaler(engine, name):
    from tests.esrgan_ref import synth_state
    from telescope_cam_detection_amd.esrgan import CropUpscaler
    _, _, _, tile, pad = WORKLOADS[name]
    return CropUpscaler(synth_state(NUM_BLOCK, 0), num_block=NUM_BLOCK, precision=engine, tile=tile, tile_pad=pad)


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

    from telescope_cam_detection_amd import _capi
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    rate = (C.c_float * 3)()
    assert _capi.lib().rtd_bench_mfma_rate(1, 20, rate) == _capi.RTD_OK
    mfma_tflops = float(rate[0])
    res = {"mfma_f16_tflops_random_operands": round(mfma_tflops, 1), "mfma_probe_clock_ghz": round(float(rate[1]), 3),
           "macs_per_input_pixel": macs_per_input_pixel(), "macs_per_input_pixel_issued": macs_per_input_pixel(padded=True)}
    for engine in ENGINES:
        up = None
        for name in WORKLOADS:
            if up is None:
                up = make_upscaler(engine, name)                    # (every workload uses the default tiling: one handle per engine)
            frames, rects = scene(name)
            n, _, rect, tile, pad = WORKLOADS[name]
            h, w = rect[3] - rect[1], rect[2] - rect[0]
            for _ in range(2):
                up.upscale(frames, rects)
            torch.cuda.synchronize()
            rounds = []
            for _ in range(5):
                ms = []
                for _ in range(a.calls):
                    up.upscale(frames, rects)
                    ms.append(up.last_call_ms())
                rounds.append(sum(ms) / len(ms))
            t = med(rounds)
            flop = 2.0 * macs_per_input_pixel() * n * h * w
            flop_issued = 2.0 * macs_per_input_pixel(padded=True) * n * tile_pixels(h, w, tile, pad)
            r = {"crops": n, "crop_hw": [h, w], "tiles_per_crop": len(range(0, h, tile)) * len(range(0, w, tile)), "call_ms": t,
                 "call_ms_rounds": [round(x, 4) for x in rounds], "ms_per_crop": round(t / n, 4), "derived_tflop": round(flop / 1e12, 4),
                 "derived_tflop_issued": round(flop_issued / 1e12, 4), "tflops_useful": round(flop / t / 1e9, 2),
                 "arena_mib": round(up.arena_bytes() / 2 ** 20, 1)}
            if engine == "f16x3":                                   # three fp16 MFMAs per product
                r["fraction_of_mfma_rate"] = round(3 * flop_issued / (t * 1e-3) / (mfma_tflops * 1e12), 4)
            res.setdefault(engine, {})[name] = r
            print(json.dumps({engine: {name: r}}), flush=True)
        up.close()
    merge(a.out, {"calls": res})


def cmd_conv(a):
    import torch

    from telescope_cam_detection_amd import _capi
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    L = _capi.lib()
    res = {}
    for dt_name, dt in (("f16x2", _capi.DT_F16X2), ("fp32", _capi.DT_F32)):
        for cin, cout, with_res in ((64, 32, 0), (96, 32, 0), (128, 32, 0), (160, 32, 0), (192, 64, 1)):
            out = (C.c_float * 2)()
            row = {}
            for rnd in range(5):                                    # the sides alternate
                for label, act in (("relu", 1), ("lrelu", 4)):
                    if act == 1:
                        rc = L.rtd_bench_conv(dt, 1, 128, 128, cin, cout, 3, 1, 1, with_res, 200, 0, out)
                    else:
                        rc = L.rtd_bench_conv_act(dt, 1, 128, 128, cin, cout, 3, 1, 1, with_res, act, 200, 0, out)
                    assert rc == _capi.RTD_OK, (L.rtd_last_error(None) or b"").decode()
                    row.setdefault(label + "_us_rounds", []).append(round(float(out[0]), 3))
            for label in ("relu", "lrelu"):
                row[label + "_us"] = med(row[label + "_us_rounds"])
            flop = 2.0 * 128 * 128 * 9 * cin * cout
            row["tflops_lrelu"] = round(flop / row["lrelu_us"] / 1e6, 2)
            res.setdefault(dt_name, {})[f"{cin}to{cout}{'_res' if with_res else ''}_128x128"] = row
            print(json.dumps({dt_name: {f"{cin}to{cout}": row}}), flush=True)
    merge(a.out, {"dense_block_convs": res})


def cmd_run(a):
    import torch
    frames, rects = scene(a.workload)
    up = make_upscaler(a.engine, a.workload)
    try:
        for _ in range(a.calls):
            up.upscale(frames, rects)
        torch.cuda.synchronize()
        print(json.dumps({"workload": a.workload, "engine": a.engine, "calls": a.calls}))
    finally:
        up.close()


def cmd_kernels(a):
    totals = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            m = re.search(r"(conv\w*_kernel|esrgan_\w+|k_axpby|k_upsample2x|k_splitk_reduce)", name)      # (some names arrive mangled)
            if not m:
                continue                                            # torch's fills / copies and the weight upload are not the call
            short = m.group(1)
            t = totals.setdefault(short, {"launches_per_call": 0.0, "us_per_call": 0.0})
            t["launches_per_call"] += int(r["Calls"]) / a.calls
            t["us_per_call"] += float(r["TotalDurationNs"]) / 1e3 / a.calls
    for t in totals.values():
        t["launches_per_call"] = round(t["launches_per_call"], 1)
        t["us_per_call"] = round(t["us_per_call"], 1)
    rows = {"kernels": dict(sorted(totals.items(), key=lambda kv: -kv[1]["us_per_call"])),
            "kernel_us_per_call": round(sum(t["us_per_call"] for t in totals.values()), 1)}
    print(json.dumps(rows, indent=1))
    merge(a.out, {"kernel_trace": {f"{a.engine}/{a.workload}": rows}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "conv", "run", "kernels"])
    ap.add_argument("--workload", choices=list(WORKLOADS), default="c128")
    ap.add_argument("--engine", choices=list(ENGINES), default="f16x3")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "esrgan_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "conv": cmd_conv, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
