"""GPU: the conv kernels across the pair format's range (rows, scales and gate: tests/conv_range_cases.py).  The operands of
tests/test_gpu_conv_instances.py get per-channel power-of-two scales - 2^-8 .. 2^4 on the inputs, 2^-10 .. 2^6 on the outputs - and every
output ELEMENT is held to F rho A_i + floor_i against fp64 on the values the kernel sees, so a small-magnitude channel cannot hide next
to max |y|.  The scales change no shape: the row's pinned kernel, S and grid must run.
Then, one row per kernel family (relu wherever the family has it) and the split-K epilogue:
  saturation: the last 32-channel group's scale is 2^16; pair outputs are clamp(reference, +-65504) under the same gate and exactly
              +-65504 (hi 0x7BFF / 0xFBFF, lo 0) beyond the bound, fp32 rows are not clamped;
  NaN:        one NaN in x; the outputs that are NaN are those the fp64 reference has as NaN - its receptive field, every channel, the
              follower's output included - and everything else holds the gate.  (The fused max-pool of reg3x3.cog2.pool drops NaNs as
              the stand-alone max-pools do, DESIGN.md: there the kernel's NaNs must lie inside the reference's set.)"""
import numpy as np
import pytest
import torch

from telescope_cam_detection_amd import _capi
from tests import conv_range_cases as cr
from tests.conv_range_cases import follower_references, references
from tests.conv_reference import pooled_ref
from tests.test_gpu_conv_instances import ACT_CODE, Guarded, L, Operands, ck, pool_avg_bits, set_options  # noqa: F401 (L: fixture)
from tests.test_gpu_conv_views import ViewBuf

pytestmark = pytest.mark.gpu


def launch(L, ops, finite=True):
    """The row's launch (on its views where it has them) with guards; asserts the pinned kernel ran.
    Returns dict(y, y1, pooled: fp64 values or None; y_buf, avg_buf, pooled_buf: the output buffers)."""
    r = ops.row
    B, H, W, Cin, Cout, k, Cn = r["B"], r["H"], r["W"], r["Cin"], r["Cout"], r["k"], r["Cnext"]
    OH, OW = ops.OH, ops.OW
    out = dict(y=None, y1=None, pooled=None, y_buf=None, avg_buf=None, pooled_buf=None)
    set_options(r["opts"])
    if "views" in r:
        kind = "pair" if ops.pair else r["dtype"]
        dt = _capi.DT_F16X2 if ops.pair else _capi.DT_F32
        gv = r["views"]
        xb = ViewBuf(kind, B, H, W, Cin, *gv["x"]).load(ops.xd)
        rb = ViewBuf(kind, B, OH, OW, Cout, *gv["res"]).load(ops.rd) if r["res_mode"] else None
        yb = ViewBuf(ops.out_kind(), B, OH, OW, Cout, *gv["y"]).prefill_nan()
        for b in (xb, rb, yb):
            if b is not None:
                b.snapshot()
        ck(L, L.rtd_op_conv_views(dt, xb.ptr(), xb.ld, None, 0, 0, ops.wd.data_ptr(), ops.bd.data_ptr(), rb.ptr() if rb is not None else None,
                                  rb.ld if rb is not None else 0, yb.ptr(), yb.ld, B, H, W, Cin, Cout, k, r["stride"], r["pad"], ACT_CODE[r["act"]],
                                  r["res_mode"], r["out_f32"], 0))
        ran = _capi.last_conv()
        assert yb.outside_unchanged(), "the launch wrote outside its channel slice"
        assert xb.unchanged() and (rb is None or rb.unchanged()), "an operand buffer changed"
        out.update(y=yb.values(finite), y_buf=yb)
    else:
        y = Guarded(ops.out_kind(), B, OH, OW, Cout) if not r["pool"] else None
        y1 = Guarded("pair", B, OH, OW, Cn) if Cn else None
        avg = Guarded("pair", B, OH // 2, OW // 2, Cout) if r["avg"] else None
        pooled = Guarded("pair", B, OH // 2, OW // 2, Cout) if r["pool"] else None
        ck(L, ops.launch(L, y, y1, avg, pooled))
        ran = _capi.last_conv()
        out.update(y=y.values(finite) if y else None, y1=y1.values(finite) if y1 else None, pooled=pooled.values(finite) if pooled else None,
                   y_buf=y, avg_buf=avg, pooled_buf=pooled)
        if avg is not None:
            avg.values(finite)
    assert (ran["key"], ran["S"], ran["grid"]) == (r["key"], r["S"], r["grid"]), ran
    return out


def plant_nan(ops, b, py, px, c):
    """x[b, py, px, c] = NaN, in the seen values and in the stored words (pair: hi and lo of the channel's 32-group)"""
    ops.xv[b, py, px, c] = float("nan")
    if ops.pair:
        g, j = divmod(c, 32)
        ops.xd[b, py, px, 64 * g + j] = 0x7E00
        ops.xd[b, py, px, 64 * g + 32 + j] = 0x7E00
    else:
        ops.xd[b, py, px, c] = float("nan")


def pooled_bounds(rhoA, floor):
    """the max-pool of the per-element bounds"""
    return pooled_ref(rhoA), pooled_ref(floor)


def check_row(ops, out, want, y32, A, what, clamp=False):
    """Part A's gate on everything the launch wrote; returns the printed ratios."""
    r = ops.row
    factor = cr.FACTOR[r["dtype"]]
    pair_out = ops.out_kind() == "pair"
    rho = cr.yardstick(want, y32, A)
    if clamp and pair_out:
        want = want.clamp(-cr.PAIR_MAX, cr.PAIR_MAX)             # 1-Lipschitz: the bounds hold as they are
    rhoA, floor = cr.bounds(want, A, rho, pair_out)
    ratios = {}
    if r["pool"]:
        ratios["pooled"] = cr.assert_gate(f"{what} pooled", out["pooled"], pooled_ref(want), *pooled_bounds(rhoA, floor), factor)
        return ratios
    ratios["y"] = cr.assert_gate(what, out["y"], want, rhoA, floor, factor)
    if r["Cnext"]:
        got = out["y"]
        want1, y32_1, A1 = follower_references(ops, got)
        rho1 = cr.yardstick(want1, y32_1, A1)
        ratios["y1"] = cr.assert_gate(f"{what} y1", out["y1"], want1, *cr.bounds(want1, A1, rho1, True), factor)
    return ratios


@pytest.mark.parametrize("row", cr.RANGE_CASES, ids=[r["name"] for r in cr.RANGE_CASES])
def test_conv_across_the_range(L, row):
    r = row
    try:
        ops = Operands(r, scales=cr.draw_scales)
        out = launch(L, ops)
        ratios = check_row(ops, out, *references(ops), r["name"])
        if r["avg"]:                                             # bits of rtd_op_pool of the same call's y, as test_conv_instantiation holds it
            np.testing.assert_array_equal(out["avg_buf"].bits(), pool_avg_bits(L, out["y_buf"], r["B"], ops.OH, ops.OW, r["Cout"]))
        print(f"RANGE | {r['name']} | {r['key']} | S {r['S']} | " + " | ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    finally:
        _capi.debug_option("reset", 0)


FAMILY_IDS = [r["family"] for r in cr.FAMILY_CASES]


@pytest.mark.parametrize("row", cr.FAMILY_CASES, ids=FAMILY_IDS)
def test_saturation_in_every_family(L, row):
    r = row
    try:
        ops = Operands(r, scales=cr.draw_saturating_scales)
        out = launch(L, ops)
        want, y32, A = references(ops)
        beyond = (want[..., -32:].abs() > cr.PAIR_MAX).double().mean().item()
        assert beyond > 0.05, (r["name"], beyond)                # the case saturates (relu: on the positive side only)
        ratios = check_row(ops, out, want, y32, A, f"{r['family']} saturating", clamp=True)
        got, buf = (out["pooled"], out["pooled_buf"]) if r["pool"] else (out["y"], out["y_buf"])
        if ops.out_kind() == "pair":
            rho = cr.yardstick(want, y32, A)
            beyond_by = want.abs() - (cr.PAIR_MAX + cr.FACTOR[r["dtype"]] * rho * A)
            if r["pool"]:                                        # relu: the window's maximum is beyond the bound where one of its elements is
                want, beyond_by = pooled_ref(want), pooled_ref(torch.where(want > 0, beyond_by, -1.0))
            far = beyond_by > 0
            assert far.any()
            assert torch.equal(got[far], torch.sign(want[far]) * cr.PAIR_MAX)
            # ... as bits: hi = +-65504, lo = 0
            Cout = r["Cout"]
            words = torch.from_numpy(buf.bits()).reshape(got.shape[:3] + (Cout // 32, 2, 32))
            hi, lo = words[..., 0, :].reshape(got.shape), words[..., 1, :].reshape(got.shape)
            assert ((hi[far] & 0x7FFF) == 0x7BFF).all() and ((lo[far] & 0x7FFF) == 0).all()
        else:
            assert got.abs().max().item() > cr.PAIR_MAX           # fp32 rows: not clamped (the gate above holds them to the reference)
        print(f"SATURATION | {r['family']} | {r['name']} | {r['act']} | {100 * beyond:.0f} % of the group beyond | "
              + " | ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    finally:
        _capi.debug_option("reset", 0)


@pytest.mark.parametrize("row", cr.FAMILY_CASES, ids=FAMILY_IDS)
def test_a_nan_reaches_its_receptive_field_in_every_family(L, row):
    r = row
    try:
        ops = Operands(r, scales=cr.draw_scales)
        b, py, px, c = r["B"] - 1, ops.xv.shape[1] // 2, ops.xv.shape[2] // 2 - 1, r["Cin"] // 2 + 1        # an interior pixel
        plant_nan(ops, b, py, px, c)
        out = launch(L, ops, finite=False)
        want, y32, A = references(ops)
        ref_nan = torch.isnan(want)
        n_pixels = int(ref_nan[..., 0].sum())
        assert ref_nan.all(dim=-1).eq(ref_nan.any(dim=-1)).all() and 1 <= n_pixels <= 9, n_pixels     # whole pixels of the receptive field
        if r["pool"]:                                            # the fused max-pool drops NaNs: no NaN outside the reference's
            pw = pooled_ref(want)
            got = out["pooled"]
            assert not (torch.isnan(got) & ~torch.isnan(pw)).any()
            ratios = check_row(ops, out, want, y32, A, f"{r['family']} NaN")
            print(f"NAN | {r['family']} | {r['name']} | {r['act']} | {int(torch.isnan(got).sum())} NaN outputs, inside the reference's "
                  f"{int(torch.isnan(pw).sum())} | " + " | ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
            return
        got = out["y"]
        assert torch.equal(torch.isnan(got), ref_nan), (r["name"], int(torch.isnan(got).sum()), int(ref_nan.sum()))
        if r["Cnext"]:
            want1 = follower_references(ops, got)[0]
            assert torch.isnan(want1).any() and torch.equal(torch.isnan(out["y1"]), torch.isnan(want1)), r["name"]
        ratios = check_row(ops, out, want, y32, A, f"{r['family']} NaN")
        print(f"NAN | {r['family']} | {r['name']} | {r['act']} | {n_pixels} NaN pixels x {r['Cout']} channels | "
              + " | ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    finally:
        _capi.debug_option("reset", 0)
