"""Writes tests/golden/yolox_net_yardstick.json: for every seeded case of tests/yolox_net_ref.py (NET_CASES and the end-to-end case) the
max-abs errors of the torch fp32 and torch fp16 restatements against fp64 on the CPU, on the head rows and on every named stage, with
the seeds; and for the end-to-end case its candidate counts and margins.  tests/test_gpu_yolox_net.py gates the device results at a
quarter of the recorded fp16 error; this script asserts that the fp32 restatement is at least 4 x inside that gate (otherwise: change
the case's seed) and that the end-to-end case meets its input conditions on the restatement alone.

    python tools/make_yolox_net_yardstick.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import yolox_net_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "yolox_net_yardstick.json")


def errors(sd, x):
    s64, s32, s16 = {}, {}, {}
    o64 = R.forward(sd, x.double(), s64)
    o32 = R.forward(sd, x.float(), s32)
    o16 = R.forward_fp16(sd, x.float(), s16)
    s64["head"], s32["head"], s16["head"] = o64, o32, o16
    out = {}
    for k in ("head",) + R.STAGES:
        out[k] = {"fp32": float((s32[k].double() - s64[k]).abs().max()), "fp16": float((s16[k].double() - s64[k]).abs().max()),
                  "max_abs": float(s64[k].abs().max())}
        assert out[k]["fp32"] * 16 <= out[k]["fp16"], (k, out[k])      # fp32 at least 4 x inside the gate of fp16 / 4
    return out


def main():
    torch.manual_seed(0)
    doc = {"note": "max-abs errors of the torch restatements (tests/yolox_net_ref.py) against fp64, CPU; gate of the GPU tests = fp16 / 4",
           "torch": torch.__version__, "cases": {}}
    for name, (model, C, state_seed, input_seed, n, h, w) in R.NET_CASES.items():
        e = errors(R.case_state(name), R.case_input(name))
        doc["cases"][name] = {"model": model, "classes": C, "state_seed": state_seed, "input_seed": input_seed, "n": n, "h": h, "w": w, "errors": e}
        print(name, "head fp32 %.3e fp16 %.3e" % (e["head"]["fp32"], e["head"]["fp16"]))
    batch = R.e2e_batch(R.e2e_frames())
    e = errors(R.case_state("e2e"), batch)
    cond = R.e2e_conditions(batch, e["head"]["fp32"])
    for c in cond:
        assert 20 <= c["passed"] <= 500 and c["d_score"] > c["m"] and c["d_iou"] > c["m"] and c["same_rows"], c
    doc["cases"]["e2e"] = {**{k: (list(v) if isinstance(v, tuple) else v) for k, v in R.E2E.items()}, "errors": e, "images": cond}
    print("e2e head fp32 %.3e fp16 %.3e" % (e["head"]["fp32"], e["head"]["fp16"]), cond)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
