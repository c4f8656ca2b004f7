"""tests/golden/esrgan_yardstick.json: what plain fp32 and plain fp16 (the reference's own `realesrgan_half=True` mode) cost against the
fp64 restatement (tests/esrgan_ref.py) on the cases the ESRGAN tests use - max |delta| of the float output, the share of differing
bytes, the worst byte, and for the stage case the max |delta| of every named stage.  CPU only; the 23-block fp16 run takes most of a
minute, which is why the numbers are recorded rather than recomputed by the tests.

    python tools/make_esrgan_yardstick.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import esrgan_ref as ref  # noqa: E402


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    out = {"note": "errors of the torch fp32 / fp16 runs of tests/esrgan_ref.py against its fp64 run (seeded weights, seed 0)", "cases": {}}
    for name in ref.CASES:
        out["cases"][name] = dict(ref.CASES[name], **ref.measure_case(name))
        print(name, json.dumps(out["cases"][name])[:300], flush=True)
    path = os.path.join(ROOT, "tests", "golden", "esrgan_yardstick.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
