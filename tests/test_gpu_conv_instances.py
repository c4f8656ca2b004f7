"""GPU: every conv kernel instantiation launch_conv can name, one small launch each (tests/conv_cases.py, found by
tools/conv_case_search.py), against fp64 on the values the kernel sees - with the assertion that the named kernel is the one that ran
(rtd_debug_last_conv), guard bands around every output, and bit-identity of the flexible / quad pair tiles with the fixed tile.
Plus the two fused consumers that had no kernel-level entry point: the 2 x 2 average (rtd_op_conv_avg) and stem.2 + max-pool
(rtd_op_conv_pool), each bit for bit against its two-launch form."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from telescope_cam_detection_amd import _capi
from tests.conv_cases import CASES
from tests.conv_reference import ACT_FN, conv_ref, epilogue_ref, pooled_ref  # noqa: F401 (the other conv tests import them from here)

pytestmark = pytest.mark.gpu

ACT_CODE = {"none": 0, "relu": 1, "silu": 2, "gelu": 3, "lrelu": 4}
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
GUARD_PIXELS = 256            # the tallest tile of any conv kernel (conv_igemm_wsq_kernel<8, 8>: 16 * (8 + 8) pixels)
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _capi.lib()


def ck(L, rc):
    assert rc == 0, (rc, L.rtd_last_error(None))


def set_options(opts):
    _capi.debug_option("reset", 0)
    for name, value in opts.items():
        _capi.debug_option(name, value)


# ---- pair (F16X2) storage with torch (threads; the big rows hold 10^8 values): the words of _capi.to_split / the values of from_split ----
def pair_words(x):
    """fp32 [..., C] -> int16 [..., 2C]: per 32-channel group [32 hi | 32 lo], hi = fp16(x), lo = fp16(x - hi), saturating at +-65504."""
    x = x.float().clamp(-65504.0, 65504.0)
    C = x.shape[-1]
    hi = x.half()
    lo = (x - hi.float()).half()
    g = x.shape[:-1] + (C // 32, 32)
    return torch.stack([hi.view(torch.int16).reshape(g), lo.view(torch.int16).reshape(g)], dim=-2).reshape(x.shape[:-1] + (2 * C,)).contiguous()


def pair_values(words):
    """int16 [..., 2C] -> fp32 [..., C] = hi + lo (exact in fp32)."""
    C = words.shape[-1] // 2
    g = words.contiguous().reshape(words.shape[:-1] + (C // 32, 2, 32)).view(torch.float16).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(words.shape[:-1] + (C,))


class Guarded:
    """A device output [B, H, W, C] of `kind` ('pair': F16X2 words, 'f32', 'bf16') between two guard bands of GUARD_PIXELS pixels filled
    with a sentinel; the tensor itself is prefilled with NaN (pair: -1 words = fp16 NaNs)."""

    def __init__(self, kind, B, H, W, C):
        self.kind, self.shape = kind, (B, H, W, C)
        self.tdt = {"pair": torch.int16, "f32": torch.float32, "bf16": torch.bfloat16}[kind]
        self.words = 2 * C if kind == "pair" else C
        self.n = B * H * W * self.words
        self.g = GUARD_PIXELS * self.words                       # whole pixels: the view stays 16-byte aligned
        self.buf = torch.empty(self.n + 2 * self.g, dtype=self.tdt, device="cuda")
        self.prefill()

    def raw(self, t):
        return t.view(torch.int16 if self.tdt != torch.float32 else torch.int32)

    def prefill(self):
        self.raw(self.buf).fill_(SENTINEL)
        self.raw(self.view).fill_(-1)                            # fp32: 0xffffffff, bf16 / fp16: 0xffff - NaNs all

    @property
    def view(self):
        return self.buf[self.g: self.g + self.n].view(self.shape[:3] + (self.words,))

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        r = self.raw(self.buf)
        return bool((r[: self.g] == SENTINEL).all()) and bool((r[self.g + self.n:] == SENTINEL).all())

    def untouched(self):
        return self.guards_intact() and bool((self.raw(self.view) == -1).all())

    def bits(self):
        return self.raw(self.view).cpu().numpy().copy()

    def values(self, finite=True):
        """fp64 [B, H, W, C] on the host; asserts the guards and that every element was written and is finite (finite=False: the
        caller holds the non-finite elements to a reference of its own)."""
        assert self.guards_intact(), "a guard band was written"
        v = self.view.cpu()
        v = pair_values(v) if self.kind == "pair" else v.float()
        assert not finite or torch.isfinite(v).all(), "unwritten or non-finite output elements"
        return v.double()


def assert_pair_bound(got, want, what):
    err = (got - want).abs().max().item() / want.abs().max().item()
    rel = (torch.linalg.norm(got - want) / torch.linalg.norm(want)).item()
    print(f"{what}: max err / max |y| {err:.2e}, rel l2 {rel:.2e}")
    assert err < 2e-5 and rel < 1e-5, (what, err, rel)


class Operands:
    """Operands of one table row, seeded by its name: fp32 draws, their storage on the device, and the values the kernel sees.
    scales: None, or a hook (generator, row) -> dict(e=[Cin], e2=[C2] or None, f=[Cout]) of integer exponents, called after the draws
    (which it therefore leaves as they are): input channel c is multiplied by 2^e_c (second input: 2^e2_c), filter column (tap, c) of
    row n by 2^(f_n - e_c), bias and residual channel n by 2^f_n, the follower filter's column n by 2^-f_n; b1 stays.  Powers of two,
    applied before the storage rounding: the pre-activation of channel n is the unscaled one times 2^f_n, term by term.
    device: where the storage goes ("cpu": the seen values alone are wanted, tools/conv_f32_order.py)."""

    def __init__(self, row, scales=None, device="cuda"):
        self.row = r = row
        g = torch.Generator().manual_seed(zlib.crc32(r["name"].encode()))
        B, H, W, Cin, Cout, k, C2, Cn = r["B"], r["H"], r["W"], r["Cin"], r["Cout"], r["k"], r["C2"], r["Cnext"]
        self.pair = r["dtype"] == "f16x2"
        self.OH, self.OW = (H + 2 * r["pad"] - k) // r["stride"] + 1, (W + 2 * r["pad"] - k) // r["stride"] + 1
        K = k * k * Cin + C2
        x = torch.randn(B, H // 2, W // 2, Cin, generator=g) if r["x_up2"] else torch.randn(B, H, W, Cin, generator=g)   # x_up2: H, W are the output extents
        w = torch.randn(Cout, K, generator=g) * (1.0 / K) ** 0.5                                   # [tap-major x | x2] columns (OHWI rows)
        self.b = torch.randn(Cout, generator=g) * 0.1
        x2 = torch.randn(B, self.OH, self.OW, C2, generator=g) if C2 else None
        res = torch.randn(B, self.OH, self.OW, Cout, generator=g) if r["res_mode"] else None
        w1 = torch.randn(Cn, Cout, generator=g) * (1.0 / Cout) ** 0.5 if Cn else None
        self.b1 = torch.randn(Cn, generator=g) * 0.1 if Cn else None
        self.scales = scales(g, r) if scales is not None else None
        if self.scales is not None:
            p2 = lambda e: torch.ldexp(torch.ones(e.shape), e)            # exact powers of two
            e, e2, f = self.scales["e"], self.scales["e2"], self.scales["f"]
            x *= p2(e)
            w[:, : k * k * Cin] *= p2(f[:, None, None] - e[None, None, :]).expand(Cout, k * k, Cin).reshape(Cout, k * k * Cin)
            self.b *= p2(f)
            if C2:
                x2 *= p2(e2)
                w[:, k * k * Cin:] *= p2(f[:, None] - e2[None, :])
            if res is not None:
                res *= p2(f)
            if Cn:
                w1 *= p2(-f)[None, :]
        if self.pair:
            store = lambda t: pair_words(t)
            seen = lambda s: pair_values(s)
            self.wv = pair_values(pair_words(w))
            self.w1v = pair_values(pair_words(w1)) if Cn else None
        else:
            tdt = TORCH_DT[r["dtype"]]
            store = lambda t: t.to(tdt)
            seen = lambda s: s.float()
            self.wv = w.to(tdt).float()
            self.w1v = None
        xs = store(x)
        self.xv, self.xd = seen(xs), xs.to(device)
        del x, xs
        self.x2v = self.x2d = self.rv = self.rd = None
        if C2:
            s = store(x2)
            self.x2v, self.x2d = seen(s), s.to(device)
        if res is not None:
            s = store(res)
            self.rv, self.rd = seen(s), s.to(device)
        self.wd, self.bd = w.contiguous().to(device), self.b.to(device)
        self.w1d, self.b1d = (w1.contiguous().to(device), self.b1.to(device)) if Cn else (None, None)

    def reference(self):
        r = self.row
        y = conv_ref(self.xv, self.wv, self.b, r["k"], r["pad"], self.x2v, r["stride"], r["x_up2"])
        return epilogue_ref(y, r["act"], r["res_mode"], self.rv)

    def out_kind(self):
        return "f32" if self.row["out_f32"] else ("pair" if self.pair else self.row["dtype"])

    def launch(self, L, y, y1=None, avg=None, pooled=None, y_dead=0):
        """The entry point the row's form belongs to; returns its status."""
        r, p = self.row, (lambda t: t.data_ptr() if t is not None else None)
        dt = _capi.DT_F16X2 if self.pair else {"bf16": _capi.DT_BF16, "f32": _capi.DT_F32}[r["dtype"]]
        B, H, W, Cin, Cout, k = r["B"], r["H"], r["W"], r["Cin"], r["Cout"], r["k"]
        act = ACT_CODE[r["act"]]
        if r["pool"]:
            return L.rtd_op_conv_pool(p(self.xd), p(self.wd), p(self.bd), pooled.ptr(), B, H, W)
        if r["avg"]:
            return L.rtd_op_conv_avg(p(self.xd), p(self.wd), p(self.bd), p(self.rd), y.ptr(), p(self.w1d), p(self.b1d), y1.ptr() if y1 else None, avg.ptr(),
                                     B, H, W, Cin, Cout, r["Cnext"], act, r["res_mode"], ACT_CODE["relu"], y_dead)
        if r["Cnext"]:
            return L.rtd_op_conv_next(dt, p(self.xd), p(self.x2d), p(self.wd), p(self.bd), p(self.rd), y.ptr(), p(self.w1d), p(self.b1d), y1.ptr(),
                                      B, H, W, Cin, r["C2"], Cout, r["Cnext"], act, r["res_mode"], ACT_CODE["relu"])
        if r["C2"]:
            return L.rtd_op_conv_dual(dt, p(self.xd), p(self.x2d), p(self.wd), p(self.bd), p(self.rd), y.ptr(), B, H, W, Cin, r["C2"], Cout, k, r["stride"],
                                      r["pad"], act, r["res_mode"], r["out_f32"], r["x_up2"])
        return L.rtd_op_conv(dt, p(self.xd), p(self.wd), p(self.bd), p(self.rd), y.ptr(), B, H, W, Cin, Cout, k, k, r["stride"], r["pad"], act,
                             r["res_mode"], r["out_f32"])


def pool_avg_bits(L, y, B, H, W, C):
    """rtd_op_pool(kind 1: 2 x 2 average) of the pair tensor y, as bits."""
    out = Guarded("pair", B, H // 2, W // 2, C)
    ck(L, L.rtd_op_pool(1, _capi.DT_F16X2, y.ptr(), out.ptr(), B, H, W, C, C, C))
    out.values()
    return out.bits()


@pytest.mark.parametrize("row", CASES, ids=[r["name"] for r in CASES])
def test_conv_instantiation(L, row):
    """One launch per instantiation: the named kernel ran, wrote all of its output and nothing else, and agrees with fp64.
    Bounds as tests/test_gpu_ops.py holds them: pairs 2e-5 of max |y| and 1e-5 rel-l2 (the dropped lo*lo term 2^-18 per product, fp32
    accumulation, one hi / lo rounding of the output); fp32 2e-5; bf16 operands 2e-3 into fp32 rows, + one bf16 rounding into bf16."""
    r = row
    B, Cout, Cn = r["B"], r["Cout"], r["Cnext"]
    try:
        ops = Operands(r)
        OH, OW = ops.OH, ops.OW
        want = ops.reference()
        y = Guarded(ops.out_kind(), B, OH, OW, Cout) if not r["pool"] else None
        y1 = Guarded("pair", B, OH, OW, Cn) if Cn else None
        avg = Guarded("pair", B, OH // 2, OW // 2, Cout) if r["avg"] else None
        pooled = Guarded("pair", B, OH // 2, OW // 2, Cout) if r["pool"] else None
        set_options(r["opts"])
        ck(L, ops.launch(L, y, y1, avg, pooled))
        ran = _capi.last_conv()
        assert (ran["key"], ran["S"], ran["grid"]) == (r["key"], r["S"], r["grid"]), ran
        if r["pool"]:
            assert_pair_bound(pooled.values(), pooled_ref(want), f"{r['name']} pooled")
            return
        got = y.values()
        if ops.pair:
            assert_pair_bound(got, want, r["name"])
        else:
            tol = dict(atol=2e-5, rtol=2e-5) if r["dtype"] == "f32" else (dict(atol=2e-3, rtol=2e-3) if r["out_f32"] else dict(atol=2e-2, rtol=1e-2))
            print(f"{r['name']}: max abs err {(got - want).abs().max().item():.2e}")
            torch.testing.assert_close(got.float(), want.float(), **tol)
        if Cn:                                                   # the follower reads the kernel's own (rounded) y
            want1 = F.relu(got @ ops.w1v.double().t() + ops.b1.double())
            assert_pair_bound(y1.values(), want1, f"{r['name']} y1")
        if r["avg"]:
            avg.values()
            np.testing.assert_array_equal(avg.bits(), pool_avg_bits(L, y, B, OH, OW, Cout))
        family = r["key"].split(".")[0]
        if family in ("wsf", "wsq"):
            bits = y.bits()
            y.prefill()
            if r["S"] == 1:                                      # the flexible / quad tile against the fixed 128-pixel tile: same bits
                set_options(dict(r["opts"], split_flex=0, split_wsq=0, split_k2=0))
                ck(L, ops.launch(L, y))
                assert _capi.last_conv()["key"].startswith("wsx."), _capi.last_conv()
                y.values()
                np.testing.assert_array_equal(bits, y.bits(), err_msg=f"{r['name']} vs {_capi.last_conv()['key']}")
            else:                                                # reported, not asserted: the slices are summed in another order
                set_options(dict(r["opts"], split_k2=0))
                ck(L, ops.launch(L, y))
                y.values()
                print(f"{r['name']}: S = {r['S']} bits {'==' if (bits == y.bits()).all() else '!='} one-pass bits ({_capi.last_conv()['key']})")
        elif r["S"] > 1:
            bits = y.bits()
            y.prefill()
            set_options(dict(r["opts"], split_k2=0))
            ck(L, ops.launch(L, y))
            y.values()
            print(f"{r['name']}: S = {r['S']} bits {'==' if (bits == y.bits()).all() else '!='} one-pass bits ({_capi.last_conv()['key']})")
    finally:
        _capi.debug_option("reset", 0)


def avg_row(B, H, W, Cin, Cout, Cnext, act, res_mode):
    return dict(name=f"avg {B}x{H}x{W} {Cin}->{Cout}+{Cnext}", dtype="f16x2", B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=1, stride=1, pad=0, C2=0, x_up2=0,
                Cnext=Cnext, avg=1, pool=0, act=act, res_mode=res_mode, out_f32=0)


@pytest.mark.parametrize("shape", [(1, 80, 80, 64, 256, 128, "relu", 1), (2, 82, 96, 128, 512, 0, "silu", 2)], ids=["64-256-next128", "128-512"])
def test_conv_avg_against_the_two_launch_forms(L, shape):
    """rtd_op_conv_avg (ConvArgs::avg_y, y_dead): avg_y is the 2 x 2 average rtd_op_pool gives of the same call's y; y and y1 are what
    the launch without the average writes; with y_dead the y buffer keeps its prefill and y1 / avg_y keep their bits."""
    B, H, W, Cin, Cout, Cn = shape[:6]
    r = avg_row(*shape)
    try:
        ops = Operands(r)
        y, avg = Guarded("pair", B, H, W, Cout), Guarded("pair", B, H // 2, W // 2, Cout)
        y1 = Guarded("pair", B, H, W, Cn) if Cn else None
        ck(L, ops.launch(L, y, y1, avg))
        ran = _capi.last_conv()
        assert ran["key"] == f"sx.x{Cin // 32}.x2_0.res1.next{Cn}.f32_0.avg1", ran
        got = y.values()
        assert_pair_bound(got, ops.reference(), r["name"])
        if Cn:
            assert_pair_bound(y1.values(), F.relu(got @ ops.w1v.double().t() + ops.b1.double()), r["name"] + " y1")
        avg.values()
        np.testing.assert_array_equal(avg.bits(), pool_avg_bits(L, y, B, H, W, Cout))
        # the same launch without the average
        y_b, y1_b = Guarded("pair", B, H, W, Cout), (Guarded("pair", B, H, W, Cn) if Cn else None)
        ops.row = dict(r, avg=0)
        ck(L, ops.launch(L, y_b, y1_b))
        ops.row = r
        assert _capi.last_conv()["key"] == ran["key"].replace("avg1", "avg0")
        y_b.values()
        np.testing.assert_array_equal(y.bits(), y_b.bits())
        if Cn:
            y1_b.values()
            np.testing.assert_array_equal(y1.bits(), y1_b.bits())
            # y_dead: the stores of y are dropped, nothing else changes
            y_d, y1_d, avg_d = Guarded("pair", B, H, W, Cout), Guarded("pair", B, H, W, Cn), Guarded("pair", B, H // 2, W // 2, Cout)
            ck(L, ops.launch(L, y_d, y1_d, avg_d, y_dead=1))
            assert _capi.last_conv()["key"] == ran["key"]
            assert y_d.untouched(), "y_dead: the y buffer was written"
            y1_d.values(), avg_d.values()
            np.testing.assert_array_equal(y1.bits(), y1_d.bits())
            np.testing.assert_array_equal(avg.bits(), avg_d.bits())
    finally:
        _capi.debug_option("reset", 0)


@pytest.mark.parametrize("why,H,W,with_res", [("odd H", 81, 80, 1), ("W % 16", 80, 88, 1), ("no residual", 80, 80, 0)])
def test_conv_avg_refuses_what_the_predicate_refuses(L, why, H, W, with_res):
    r = avg_row(1, H, W, 128, 256, 0, "relu", 1 if with_res else 0)
    ops = Operands(r)
    y, avg = Guarded("pair", 1, H, W, 256), Guarded("pair", 1, H // 2, W // 2, 256)
    rc = ops.launch(L, y, None, avg)
    assert rc == _capi.RTD_E_INVALID, (why, rc, L.rtd_last_error(None))
    assert y.untouched() and avg.untouched(), why


@pytest.mark.parametrize("B,H,W", [(1, 60, 100), (3, 60, 108)])
def test_conv_pool_against_conv_then_pool(L, B, H, W):
    """rtd_op_conv_pool (conv3x3_reg_split_kernel<2, true> + k_pool_fixup) at the 32-tile floor (8 x 4 tiles of 8 x 32 pixels, the last
    row and column of tiles ragged): the pooled tensor has the bits of rtd_op_conv (direct 3x3 kernel) followed by rtd_op_pool(kind 0),
    and holds the pair bound against fp64.  Extents are multiples of 4: the stand-alone max-pool takes pair tensors with even POOLED
    extents only (the table's own pool row, 58 x 98 -> 29 x 49, is held to fp64 in test_conv_instantiation)."""
    r = dict(name=f"pool {B}x{H}x{W}", dtype="f16x2", B=B, H=H, W=W, Cin=32, Cout=64, k=3, stride=1, pad=1, C2=0, x_up2=0, Cnext=0, avg=0, pool=1,
             act="relu", res_mode=0, out_f32=0)
    try:
        ops = Operands(r)
        pooled = Guarded("pair", B, H // 2, W // 2, 64)
        ck(L, ops.launch(L, None, pooled=pooled))
        assert _capi.last_conv()["key"] == "reg3x3.cog2.pool", _capi.last_conv()
        assert_pair_bound(pooled.values(), pooled_ref(ops.reference()), r["name"])
        ops.row = dict(r, pool=0)
        y, two = Guarded("pair", B, H, W, 64), Guarded("pair", B, H // 2, W // 2, 64)
        ck(L, ops.launch(L, y))
        assert _capi.last_conv()["key"] == "reg3x3.cog2", _capi.last_conv()
        y.values()
        ck(L, L.rtd_op_pool(0, _capi.DT_F16X2, y.ptr(), two.ptr(), B, H, W, 64, 64, 64))
        two.values()
        np.testing.assert_array_equal(pooled.bits(), two.bits())
        # odd extents: refused before any launch
        ops.row = dict(r, H=H - 1)
        pooled.prefill()
        assert ops.launch(L, None, pooled=pooled) == _capi.RTD_E_INVALID
        assert pooled.untouched()
    finally:
        _capi.debug_option("reset", 0)
