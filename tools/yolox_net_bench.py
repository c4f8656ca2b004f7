"""Benchmark of the YOLOX network (rtd_yolox_net_run, csrc/yolox_net.hip): yolox-s at 640 x 640, 1 and 8 images, f16x3 and fp32, with
seeded weights (tests/yolox_net_ref.py synth_state).

    python tools/yolox_net_bench.py calls [--rounds 5] [--per 10] [--out profiles/yolox_net_bench.json]
        per workload: the whole call (Focus, the plan's convolutions, SPP, upsamples, head emit) between HIP events on torch's stream,
        `per` calls back to back per round, median and range over the rounds after a warm-up; and, in the same process and on the same
        device, the torch restatement in fp32 and under fp16 autocast.  The head rows of the two are compared first, so that both sides
        are known to do the same work.
    rocprofv3 --kernel-trace --stats -d DIR -o yn --output-format csv -- python tools/yolox_net_bench.py run --workload b1_f16x3 --calls 20
        the run to profile (one workload per run, so that a kernel's average belongs to one shape)
    python tools/yolox_net_bench.py kernels --workload b1_f16x3 --stats DIR/yn_kernel_stats.csv [--out profiles/yolox_net_bench.json]
        the per-kernel split of that run: calls, total and share per kernel name
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 640
GMAC_PER_IMAGE = 13.4            # yolox-s at 640 x 640 (upstream's table: 26.8 GFLOPs)
WORKLOADS = {"b1_f16x3": (1, "f16x3"), "b8_f16x3": (8, "f16x3"), "b1_fp32": (1, "fp32"), "b8_fp32": (8, "fp32")}


def make(workload):
    import torch

    from telescope_cam_detection_amd.yolox_network import YoloxNetwork
    from tests import yolox_net_ref as ref
    n, precision = WORKLOADS[workload]
    sd = ref.synth_state("yolox-s", 80, 1)
    net = YoloxNetwork(sd, "yolox-s", max_batch=8, precision=precision, input_size=(SIZE, SIZE))
    x = torch.from_numpy(ref.seeded_input(11, n, SIZE, SIZE)).cuda()
    return net, sd, x


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


def timed(call, rounds, per):
    import torch
    out = []
    for _ in range(rounds):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(per):
            call()
        ev1.record()
        ev1.synchronize()
        out.append(ev0.elapsed_time(ev1) / per)
    return out


def cmd_calls(a):
    import torch

    from tests import yolox_net_ref as ref
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    res = {}
    for name, (n, precision) in WORKLOADS.items():
        net, sd, x = make(name)
        try:
            dev_sd = {k: v.cuda() for k, v in sd.items()}

            def torch_fp32():
                with torch.no_grad():
                    return ref.forward(dev_sd, x)

            def torch_fp16():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    return ref.forward(dev_sd, x)

            for _ in range(3):
                got, want = net(x), torch_fp32()
                torch_fp16()
            torch.cuda.synchronize()
            err = float((got - want).abs().max())
            r = {"images": n, "input": [SIZE, SIZE], "precision": precision, "calls_per_round": a.per, "arena_mib": round(net.arena_bytes() / 2 ** 20, 1),
                 "max_abs_delta_to_torch_fp32": err, "rtd_yolox_net_run": summary(timed(lambda: net(x), a.rounds, a.per))}
            r["gmac_per_s"] = round(n * GMAC_PER_IMAGE / r["rtd_yolox_net_run"]["median_ms"] * 1e3, 1)
            if precision == "f16x3":             # the yardsticks do not depend on the engine: once per batch size
                r["torch_restatement_fp32"] = summary(timed(torch_fp32, a.rounds, a.per))
                r["torch_restatement_fp16_autocast"] = summary(timed(torch_fp16, a.rounds, a.per))
            res[name] = r
            print(json.dumps({name: r}), flush=True)
        finally:
            net.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    import torch
    net, _, x = make(a.workload)
    try:
        for _ in range(a.calls):
            net(x)
        torch.cuda.synchronize()
        print(json.dumps({"workload": a.workload, "calls": a.calls}))
    finally:
        net.close()


def cmd_kernels(a):
    rows, total = [], 0.0
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            total += ns
            rows.append({"kernel": r.get("Name", "")[:100], "calls": int(r["Calls"]), "total_ms": round(ns / 1e6, 3), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)})
    rows.sort(key=lambda r: -r["total_ms"])
    for r in rows:
        r["share"] = round(r["total_ms"] * 1e6 / total, 4) if total else 0.0
    out = {"kernel_ms_total": round(total / 1e6, 3), "kernels": rows[:24]}
    print(json.dumps({a.workload: out}, indent=1))
    merge(a.out, {"kernels": {a.workload: out}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels"])
    ap.add_argument("--workload", choices=list(WORKLOADS), default="b1_f16x3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "yolox_net_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
