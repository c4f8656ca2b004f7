"""GPU: the conv kernel families on channel-slice views, one small launch per row of tests/conv_view_cases.py (found by
tools/conv_case_search.py): x and y - and, per form, the residual and the second input - are slices [c0 | C | c1] of wider buffers with
pairwise different pixel strides, B >= 2, at stride 1 and 2, one-pass and two-pass split-K, as the networks launch them through
Tensor::slice_c.  Per row: the named kernel ran (rtd_debug_last_conv), the slice agrees with fp64 on the values the kernel sees at the
bounds tests/test_gpu_conv_instances.py holds, nothing outside the slice was written, no operand buffer changed, and the slice has the
bits the dense launch of the same operands writes under the same options (same key, S and grid).

Every word of a buffer outside the slice, and of its guard bands, holds 2^14 in the buffer's storage type (pair buffers: in every fp16
word, hi and lo).  It is finite on purpose: the loaders may multiply a loaded chunk by a zero-padded filter column, which a NaN would
turn into a false alarm; against operands of unit scale one stray product is of the order 10^2..10^3 and cannot hide in any bound."""
import numpy as np
import pytest
import torch

from telescope_cam_detection_amd import _capi
from tests.conv_view_cases import VIEW_CASES
from tests.test_gpu_conv_instances import ACT_CODE, GUARD_PIXELS, Guarded, L, Operands, ck, pair_values, set_options  # noqa: F401 (L: fixture)

pytestmark = pytest.mark.gpu

POISON_BITS = {"pair": 0x7400, "bf16": 0x4680, "f32": 0x46800000}     # 2^14 as fp16, bf16, fp32
TORCH_KIND = {"pair": torch.int16, "f32": torch.float32, "bf16": torch.bfloat16}


def raw(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class ViewBuf:
    """A device tensor [B, H, W, C] of `kind` as the channel slice [c0 : c0 + C] of a buffer [B, H, W, c0 + C + c1] between two guard
    bands of GUARD_PIXELS pixels; every word outside the slice holds 2^14."""

    def __init__(self, kind, B, H, W, C, c0, c1):
        self.kind, self.shape = kind, (B, H, W, C)
        wpc = 2 if kind == "pair" else 1                          # storage words per channel
        self.ld = c0 + C + c1                                     # pixel stride in channels, as the entry point takes it
        self.ldw, self.w0, self.cw = wpc * self.ld, wpc * c0, wpc * C
        self.n = B * H * W * self.ldw
        self.g = GUARD_PIXELS * self.ldw
        self.buf = torch.empty(self.n + 2 * self.g, dtype=TORCH_KIND[kind], device="cuda")
        raw(self.buf).fill_(POISON_BITS[kind])
        self.before = None

    def inside(self, flat):
        B, H, W, _ = self.shape
        return flat[self.g: self.g + self.n].view(B, H, W, self.ldw)[..., self.w0: self.w0 + self.cw]

    @property
    def view(self):
        return self.inside(self.buf)

    def ptr(self):
        p = self.view.data_ptr()
        assert p % 16 == 0
        return p

    def load(self, storage):
        self.view.copy_(storage)
        return self

    def prefill_nan(self):
        raw(self.view).fill_(-1)                                  # fp32: 0xffffffff, bf16 / fp16: 0xffff - NaNs all
        return self

    def snapshot(self):
        self.before = raw(self.buf).clone()

    def unchanged(self):
        return torch.equal(raw(self.buf), self.before)

    def outside_unchanged(self):
        diff = raw(self.buf) != self.before
        self.inside(diff).fill_(False)
        return not bool(diff.any())

    def bits(self):
        return raw(self.view).contiguous().cpu().numpy()

    def values(self, finite=True):
        v = self.view.contiguous().cpu()
        v = pair_values(v) if self.kind == "pair" else v.float()
        assert not finite or torch.isfinite(v).all(), "unwritten or non-finite output elements"
        return v.double()


def error_text(row, pair, got, want):
    """The row's error against fp64, asserted at the bounds of test_conv_instantiation: pairs 2e-5 of max |y| and 1e-5 rel-l2; fp32 2e-5;
    bf16 operands 2e-3 into fp32 rows, 2e-2 / 1e-2 into bf16 rows.  Stride and pixel strides change which addresses are read, not K or
    the accumulation: the same bounds."""
    if pair:
        err = (got - want).abs().max().item() / want.abs().max().item()
        rel = (torch.linalg.norm(got - want) / torch.linalg.norm(want)).item()
        text = f"max err / max |y| {err:.2e}, rel l2 {rel:.2e}"
        print(f"{row['name']}: {text}")
        assert err < 2e-5 and rel < 1e-5, (row["name"], err, rel)
        return text
    tol = dict(atol=2e-5, rtol=2e-5) if row["dtype"] == "f32" else (dict(atol=2e-3, rtol=2e-3) if row["out_f32"] else dict(atol=2e-2, rtol=1e-2))
    text = f"max abs err {(got - want).abs().max().item():.2e}"
    print(f"{row['name']}: {text}")
    torch.testing.assert_close(got.float(), want.float(), **tol)
    return text


@pytest.mark.parametrize("row", VIEW_CASES, ids=[r["name"] for r in VIEW_CASES])
def test_conv_on_views(L, row):
    r = dict(row, Cnext=0, avg=0, pool=0)
    B, H, W, Cin, Cout, C2, k = r["B"], r["H"], r["W"], r["Cin"], r["Cout"], r["C2"], r["k"]
    try:
        ops = Operands(r)
        OH, OW = ops.OH, ops.OW
        want = ops.reference()
        kind = "pair" if ops.pair else r["dtype"]
        gv = r["views"]
        xb = ViewBuf(kind, *ops.xd.shape[:3], Cin, *gv["x"]).load(ops.xd)
        x2b = ViewBuf(kind, B, OH, OW, C2, *gv["x2"]).load(ops.x2d) if C2 else None
        rb = ViewBuf(kind, B, OH, OW, Cout, *gv["res"]).load(ops.rd) if r["res_mode"] else None
        yb = ViewBuf(ops.out_kind(), B, OH, OW, Cout, *gv["y"]).prefill_nan()
        if rb is not None:
            assert len({xb.ld, yb.ld, rb.ld}) == 3, "pixel strides of x, y and the residual must differ pairwise"
        bufs = [b for b in (xb, x2b, rb, yb) if b is not None]
        for b in bufs:
            b.snapshot()
        dt = _capi.DT_F16X2 if ops.pair else {"bf16": _capi.DT_BF16, "f32": _capi.DT_F32}[r["dtype"]]
        set_options(r["opts"])
        ck(L, L.rtd_op_conv_views(dt, xb.ptr(), xb.ld, x2b.ptr() if C2 else None, C2, x2b.ld if C2 else 0, ops.wd.data_ptr(), ops.bd.data_ptr(),
                                  rb.ptr() if rb is not None else None, rb.ld if rb is not None else 0, yb.ptr(), yb.ld, B, H, W, Cin, Cout, k, r["stride"],
                                  r["pad"], ACT_CODE[r["act"]], r["res_mode"], r["out_f32"], r["x_up2"]))
        ran = _capi.last_conv()
        assert (ran["key"], ran["S"], ran["grid"]) == (r["key"], r["S"], r["grid"]), ran
        # nothing else was written: the y buffer outside the slice and its guards, and every operand buffer, keep their bits
        assert yb.outside_unchanged(), "the launch wrote outside its channel slice"
        for b, what in ((xb, "x"), (x2b, "x2"), (rb, "res")):
            assert b is None or b.unchanged(), f"the {what} buffer changed"
        text = error_text(r, ops.pair, yb.values(), want)
        # the dense launch of the same operands under the same options: same kernel, same bits (the K rows too: k_splitk_reduce sums the
        # slices in a fixed order)
        y = Guarded(ops.out_kind(), B, OH, OW, Cout)
        ck(L, ops.launch(L, y))
        dense = _capi.last_conv()
        assert (dense["key"], dense["S"], dense["grid"]) == (r["key"], r["S"], r["grid"]), dense
        y.values()
        np.testing.assert_array_equal(yb.bits(), y.bits(), err_msg=f"{r['name']}: view vs dense launch")
        print(f"{r['name']} [{ran['key']}, S = {ran['S']}, grid {ran['grid']}]: {text}, bits == dense")
    finally:
        _capi.debug_option("reset", 0)
