"""Benchmark of the EVA02 species classifier (rtd_eva_forward, csrc/classifier.hip) at the reference's architecture, ViT-L/14 at 336 px
(24 blocks, 1024 channels, 16 heads, 577 tokens, 10 000 classes), with SEEDED weights: no network, no weights file.  No trained checkpoint
was available, so accuracy on real weights is not measured here - only time, and the distance to torch's own fp32 forward of the same
weights.

    python tools/eva_bench.py calls [--calls 5] [--out profiles/eva_bench.json]
        per batch size N = 1, 4, 16: HIP-event time of our handle (f16x3, fp32) on torch's stream, and in the same process the
        torch-ROCm forward of tests/eva_ref's module in fp32 and under fp16 autocast (the plain restatement: it materialises the softmax and
        calls no fused attention, so it is a lower bound on what a tuned torch model does); medians of five interleaved rounds of at least
        --window-ms each (the lists are kept), the derived FLOP count, and max |delta logit| of ours against that fp32 forward
    rocprofv3 --kernel-trace --stats -d DIR -o eva --output-format csv -- python tools/eva_bench.py run --batch 4 --engine f16x3 --calls 5
    python tools/eva_bench.py kernels --batch 4 --engine f16x3 --calls 5 --stats DIR/eva_kernel_stats.csv [--out ...]
        per-kernel-name totals of that run, per call
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 4, 16)
ENGINES = ("f16x3", "fp32")


def arch_of(a):
    from telescope_cam_detection_amd.eva_checkpoint import EvaArch
    return EvaArch(depth=a.depth)


def flop_per_image(arch):
    """2 flop per MAC of what the algorithm needs (no padding): patch embed, per block qkv + proj + fc1_g + fc1_x + fc2 and the two
    attention products, the head"""
    D, H, L = arch.dim, arch.hidden, arch.tokens
    block = L * (4 * D * D + 3 * D * H) + 2 * L * L * D
    return 2.0 * ((L - 1) * 3 * arch.patch ** 2 * D + arch.depth * block + D * arch.classes)


def make(a, engine):
    import torch

    from tests.eva_ref import synth_state
    from telescope_cam_detection_amd.classifier import Eva02Classifier
    arch = arch_of(a)
    sd = synth_state(arch, 0)
    clf = Eva02Classifier(sd, precision=engine, max_batch=max(BATCHES), arch=arch)
    x = torch.randn((max(BATCHES), 3, arch.img, arch.img), generator=torch.Generator().manual_seed(5)).cuda()
    return arch, sd, clf, x


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


def timed(fns, calls):
    """{name: fn} -> {name: five HIP-event times of `calls` calls each (ms per call)}, after two warm-up calls of every fn; the rounds
    are interleaved (round r times every fn once before round r + 1), so drift of the device or the host falls on all of them alike"""
    import torch
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            rounds[k].append(e0.elapsed_time(e1) / calls)
    return rounds


def cmd_calls(a):
    import torch

    from tests.eva_ref import EvaModule
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    res = {}
    arch, sd, clf, x = make(a, "f16x3")
    clfs = {"f16x3": clf}
    clfs["fp32"] = type(clf)(sd, precision="fp32", max_batch=max(BATCHES), arch=arch)
    mod = EvaModule(sd, arch).cuda().eval()
    res["arch"] = {"name": arch.name, "gflop_per_image": round(flop_per_image(arch) / 1e9, 2), "weights": "seeded (tests/eva_ref.synth_state, seed 0)"}

    def torch_fp32(n):
        with torch.no_grad():
            return mod(x[:n])

    def torch_fp16(n):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return mod(x[:n])

    for n in BATCHES:
        want = torch_fp32(n).double()
        row = {"torch_fp32_logit_max_abs": round(float(want.abs().max()), 4)}
        fns = {"ours_f16x3": lambda: clfs["f16x3"](x[:n]), "ours_fp32": lambda: clfs["fp32"](x[:n]), "torch_fp32": lambda: torch_fp32(n),
               "torch_fp16_autocast": lambda: torch_fp16(n)}
        calls = max(a.calls, -(-a.window_ms // 5))                   # (a round is at least ~window_ms at the fastest variant's ~5 ms per call)
        for name, rounds in timed(fns, calls).items():
            t = med(rounds)
            row[name] = {"call_ms": t, "calls_per_round": calls, "call_ms_rounds": [round(v, 4) for v in rounds], "ms_per_image": round(t / n, 4),
                         "tflops_useful": round(flop_per_image(arch) * n / t / 1e9, 2),
                         "max_abs_delta_logit_vs_torch_fp32": float((fns[name]().double() - want).abs().max())}
        row["saturated_values_f16x3"] = clfs["f16x3"].self_check()
        row["arena_mib_f16x3"] = round(clfs["f16x3"].arena_bytes() / 2 ** 20, 1)
        res[f"n{n}"] = row
        print(json.dumps({f"n{n}": row}), flush=True)
    for c in clfs.values():
        c.close()
    merge(a.out, {"calls": res})


def cmd_run(a):
    import torch
    _, _, clf, x = make(a, a.engine)
    try:
        for _ in range(a.calls):
            clf(x[:a.batch])
        torch.cuda.synchronize()
        print(json.dumps({"batch": a.batch, "engine": a.engine, "calls": a.calls}))
    finally:
        clf.close()


def cmd_kernels(a):
    totals = {}
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            m = re.search(r"(conv\w*_kernel|eva_[a-z]+(?:_[a-z]+)?(?=E|<|\b)|k_attention(?:_mfma_f32)?|k_splitk_reduce)", name)      # (some names arrive mangled)
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
    merge(a.out, {"kernel_trace": {f"{a.engine}/n{a.batch}": rows}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["calls", "run", "kernels"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--engine", choices=list(ENGINES), default="f16x3")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--window-ms", type=int, default=300, help="calls: least length of one timed round")
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--stats")
    ap.add_argument("--out", default=os.path.join("profiles", "eva_bench.json"))
    a = ap.parse_args()
    {"calls": cmd_calls, "run": cmd_run, "kernels": cmd_kernels}[a.cmd](a)


if __name__ == "__main__":
    main()
