"""The fp32 conv kernels' accumulation order restated on the CPU, under the per-element gate of tests/conv_range_cases.py (no GPU).

conv_igemm_kernel / conv_igemm_ws_kernel keep ONE fp32 accumulator per output element and walk K in order: K-steps of 32 columns
(tap-major, channel-minor), four sub-steps of 8, each four v_mfma_f32_32x32x2f32 that take columns (j, 4 + j) of the sub-step
(Mma<float>, csrc/conv_igemm.hip).  Restated: acc = fl32(acc + x_k w_k) over the columns in that order - every product exact (fp64) and
one fp32 rounding per column, as a chain of fused multiply-adds - then bias, residual and activation in fp32.  torch's fp32 GEMM on the
CPU, the gate's yardstick, sums in blocks, so over K = 288 .. 576 columns a sequential sum is the wider of two honest orders.

Prints, for every fp32 row of RANGE_CASES, the restatement's worst (err - floor) / (rho A): the figure the kernel's own ratio is compared
with in EXPERIMENTS.md.
    python tools/conv_f32_order.py [row name substring]
Bit for bit against the kernels (rows without a residual):
    python tools/conv_f32_order.py --dump DIR [substring]      on the MI355X: launches the rows and writes DIR/f32_<row>.npy
    python tools/conv_f32_order.py --against DIR [substring]   anywhere: counts the elements whose bits differ from the restatement's
(K = 288 on ws.f32.s2.bn128 and K = 576 on tile.f32.64x64.smallc0, no transcendental in the activation: 0 of 4 194 304 and 0 of 6144
differ.  A SiLU / GELU row differs in the activation's last bits, not in the sum.)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import conv_range_cases as cr                   # noqa: E402
from tests.conv_reference import ACT_FN                   # noqa: E402
from tests.test_gpu_conv_instances import Operands        # noqa: E402

MFMA_ORDER = (0, 4, 1, 5, 2, 6, 3, 7)                     # columns of an 8-column sub-step in the order the four MFMAs take them


def sequential(cols, w, chunk=4096):
    """fp32 [M, N]: acc = fl32(acc + cols[:, k] w[:, k]) over k in the kernel's order"""
    M, K = cols.shape
    order = [8 * s + j for s in range((K + 7) // 8) for j in MFMA_ORDER if 8 * s + j < K]
    wd = w.double()
    out = torch.empty(M, w.shape[0])
    for m0 in range(0, M, chunk):
        c = cols[m0: m0 + chunk].double()
        acc = torch.zeros(c.shape[0], w.shape[0])
        for k in order:
            acc = torch.addcmul(acc.double(), c[:, k: k + 1], wd[None, :, k]).float()
        out[m0: m0 + chunk] = acc
    return out


def dump_path(d, r):
    return os.path.join(d, "f32_" + r["name"].replace("/", "_") + ".npy")


def dump(d, pick):
    """the kernels' own outputs, through the range test's launch (guards, the pinned kernel asserted)"""
    import numpy as np

    from telescope_cam_detection_amd import _capi
    from tests.test_gpu_conv_range import launch
    os.makedirs(d, exist_ok=True)
    for r in cr.RANGE_CASES:
        if r["dtype"] == "f32" and pick in r["name"] and not r["res_mode"]:
            out = launch(_capi.lib(), Operands(r, scales=cr.draw_scales))
            _capi.debug_option("reset", 0)
            np.save(dump_path(d, r), out["y"].float().numpy())
            print("wrote", dump_path(d, r), flush=True)


def main():
    argv = sys.argv[1:]
    mode = argv.pop(0) if argv and argv[0] in ("--dump", "--against") else None
    d = argv.pop(0) if mode else None
    pick = argv[0] if argv else ""
    if mode == "--dump":
        return dump(d, pick)
    worst = 0.0
    for r in cr.RANGE_CASES:
        if r["dtype"] != "f32" or pick not in r["name"]:
            continue
        ops = Operands(r, scales=cr.draw_scales, device="cpu")
        want, y32, A = cr.references(ops)
        v = sequential(cr.columns(ops), ops.wv).reshape(want.shape) + ops.b
        if r["res_mode"] == 1:
            v = v + ops.rv
        v = ACT_FN[r["act"]](v)
        if r["res_mode"] == 2:
            v = v + ops.rv
        if mode == "--against" and os.path.exists(dump_path(d, r)):
            import numpy as np
            differ = int((torch.from_numpy(np.load(dump_path(d, r))) != v).sum())
            print(f"{r['name']}: {differ} of {v.numel()} elements differ from the kernel's bits", flush=True)
        rho = cr.yardstick(want, y32, A)
        ratio = cr.worst_ratio(v.double(), want, *cr.bounds(want, A, rho, False))
        worst = max(worst, ratio)
        print(f"{r['name']} | K {r['k'] * r['k'] * r['Cin']} | rho {rho:.3e} | sequential fp32 {ratio:.2f}", flush=True)
    print(f"worst {worst:.2f}")


if __name__ == "__main__":
    main()
