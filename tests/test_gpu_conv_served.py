"""GPU: every conv launch signature the served networks make (tests/conv_served_cases.py, found by tools/served_conv_census.py), one small
launch each with the served channels, stride, activation, residual mode and output type, against fp64 on the values the kernel sees.
Per row: the named kernel ran with the named S and grid (rtd_debug_last_conv), every output element was written, and the error holds
the bounds of tests/test_gpu_conv_views.py's error_text (pairs 2e-5 of max |y| and 1e-5 rel-l2, fp32 2e-5).  Rows with `views` run
through rtd_op_conv_views on slices with the served offsets, with the poison and guard checks of test_conv_on_views.
And the census against the real plans: seeded handles of the three networks report their plans' conv launches
(rtd_debug_*_plan_convs), which must be the lists tools/served_conv_census.py restates, entry by entry."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from telescope_cam_detection_amd import _capi, classifier, esrgan, yolox_network
from telescope_cam_detection_amd.eva_checkpoint import EvaArch, make_blob
from tests import esrgan_ref, eva_ref, yolox_net_ref
from tests.conv_served_cases import COVERED_ELSEWHERE, SERVED_CASES, UNREACHED_SERVED
from tests.test_gpu_conv_instances import ACT_CODE, ACT_FN, Guarded, L, Operands, ck, set_options  # noqa: F401 (L: fixture)
from tests.test_gpu_conv_views import ViewBuf, error_text
from tools import conv_case_search as search
from tools import served_conv_census as census

pytestmark = pytest.mark.gpu


def torch_fp32_text(ops, r, want):
    """The same row in torch fp32 on the CPU against fp64: the figures error_text prints, for a row that misses its bound."""
    k, N = r["k"], r["Cout"]
    w = ops.wv.reshape(N, k, k, r["Cin"]).permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(ops.xv.permute(0, 3, 1, 2).float(), w.float(), ops.b.float(), stride=r["stride"], padding=r["pad"]).permute(0, 2, 3, 1)
    if r["res_mode"] == 1:
        y = y + ops.rv.float()
    y = ACT_FN[r["act"]](y)
    if r["res_mode"] == 2:
        y = y + ops.rv.float()
    y = y.double()
    err = (y - want).abs().max().item() / want.abs().max().item()
    rel = (torch.linalg.norm(y - want) / torch.linalg.norm(want)).item()
    return f"torch fp32 on the CPU: max err / max |y| {err:.2e}, rel l2 {rel:.2e}, max abs err {(y - want).abs().max().item():.2e}"


@pytest.mark.parametrize("row", SERVED_CASES, ids=[r["name"] for r in SERVED_CASES])
def test_served_launch(L, row):
    r = row
    B, H, W, Cin, Cout, k = r["B"], r["H"], r["W"], r["Cin"], r["Cout"], r["k"]
    try:
        ops = Operands(r)
        OH, OW = ops.OH, ops.OW
        want = ops.reference()
        kind = "pair" if ops.pair else r["dtype"]
        dt = _capi.DT_F16X2 if ops.pair else _capi.DT_F32
        set_options(r["opts"])
        if "views" in r:
            gv = r["views"]
            xb = ViewBuf(kind, B, H, W, Cin, *gv["x"]).load(ops.xd)
            rb = ViewBuf(kind, B, OH, OW, Cout, *gv["res"]).load(ops.rd) if r["res_mode"] else None
            yb = ViewBuf(ops.out_kind(), B, OH, OW, Cout, *gv["y"]).prefill_nan()
            bufs = [b for b in (xb, rb, yb) if b is not None]
            for b in bufs:
                b.snapshot()
            ck(L, L.rtd_op_conv_views(dt, xb.ptr(), xb.ld, None, 0, 0, ops.wd.data_ptr(), ops.bd.data_ptr(), rb.ptr() if rb is not None else None,
                                      rb.ld if rb is not None else 0, yb.ptr(), yb.ld, B, H, W, Cin, Cout, k, r["stride"], r["pad"], ACT_CODE[r["act"]],
                                      r["res_mode"], r["out_f32"], 0))
            ran = _capi.last_conv()
            assert yb.outside_unchanged(), "the launch wrote outside its channel slice"
            for b, what in ((xb, "x"), (rb, "res")):
                assert b is None or b.unchanged(), f"the {what} buffer changed"
            got = yb.values()                                    # (asserts that every element of the slice was written and is finite)
        else:
            y = Guarded(ops.out_kind(), B, OH, OW, Cout)
            ck(L, ops.launch(L, y))
            ran = _capi.last_conv()
            got = y.values()                                     # (... and that the guard bands are intact)
        assert (ran["key"], ran["S"], ran["grid"]) == (r["key"], r["S"], r["grid"]), ran
        print(f"{r['name']} [{ran['key']}, S = {ran['S']}, grid {ran['grid']}, {B} x {H} x {W}, {Cin} -> {Cout}]")
        try:
            error_text(r, ops.pair, got, want)
        except AssertionError:
            print(f"{r['name']}: {torch_fp32_text(ops, r, want)}")
            raise
    finally:
        _capi.debug_option("reset", 0)


# ---- the census against the real plans -------------------------------------------------------------------------------------------------------
ENGINE_NAME = {"f16x2": "f16x3", "f32": "fp32"}
ALL_SIGNATURES = {census.row_signature(r) for r in SERVED_CASES} | set(COVERED_ELSEWHERE) | set(UNREACHED_SERVED)


def assert_plan_is_the_census(reported, expected, by_name):
    assert len(reported) == len(expected), (len(reported), len(expected))
    for i, (got, f) in enumerate(zip(reported, expected)):
        want = dict(dtype=search.DT[f["dtype"]], B=f["B"], H=f["H"], W=f["W"], Cin=f["Cin"], Cout=f["Cout"], k=f["k"], stride=f["stride"], pad=f["pad"],
                    act=ACT_CODE[f["act"]], res_mode=f["res_mode"], out_f32=f["out_f32"], ldx=f["ldx"], ldy=f["ldy"], ldres=f["ldres"])
        assert {k: got[k] for k in want} == want, (i, f["name"], got)
        assert got["name"] == (f["name"] if by_name else str(i)), (i, got["name"], f["name"])
        c = census.choice(f)
        assert c is not None and (got["key"], got["S"], got["grid"]) == (c["key"], c["S"], c["grid"]), (f["name"], got, c)
        assert census.signature(f, got) in ALL_SIGNATURES, (f["name"], census.signature(f, got))


_YOLOX_STATE, _EVA_BLOB = {}, {}


def yolox_state(variant):
    """Seeded weights, shared by the engines.  The plan does not depend on them: the BatchNorm statistics come from one 96 x 96 image
    (the default calibration batch costs yolox-l eight seconds on the host)."""
    if variant not in _YOLOX_STATE:
        calib = torch.from_numpy(yolox_net_ref.seeded_input(7919, 1, 96, 96))
        _YOLOX_STATE[variant] = yolox_net_ref.synth_state(variant, census.YOLOX_CLASSES, 0, calib=calib)
    return _YOLOX_STATE[variant]


# (creating a YOLOX-l handle uploads 217 MB of filters and takes 9 s, so it is made once: the walk restated in Python is one function for
# both engines, and YOLOX-s holds it to both)
@pytest.mark.parametrize("variant,n,dtype", [("yolox-s", 8, "f16x2"), ("yolox-s", 8, "f32"), ("yolox-l", 1, "f16x2")])
def test_yolox_plan_is_the_census(L, variant, n, dtype):
    _capi.debug_option("reset", 0)
    net = yolox_network.YoloxNetwork(yolox_state(variant), variant, max_batch=n, precision=ENGINE_NAME[dtype], input_size=census.YOLOX_INPUT)
    try:
        with pytest.raises(_capi.RtdError):
            _capi.plan_convs("yolox", net._h)                    # RTD_E_STATE before the first run
        pred = net(torch.zeros((n, 3) + census.YOLOX_INPUT, device="cuda"))
        torch.cuda.synchronize()
        assert torch.isfinite(pred).all()
        assert_plan_is_the_census(_capi.plan_convs("yolox", net._h), census.yolox_launches(variant, n, dtype), by_name=True)
    finally:
        net.close()


@pytest.mark.parametrize("dtype", census.ENGINES)
def test_eva_plan_is_the_census(L, dtype):
    _capi.debug_option("reset", 0)
    arch, n = EvaArch(depth=1), 4                                # full ViT-L width; every block makes the same launches
    if "blob" not in _EVA_BLOB:
        _EVA_BLOB["blob"] = make_blob(eva_ref.synth_state(arch, 0), arch)[1]
    clf = classifier.Eva02Classifier(_EVA_BLOB["blob"], precision=ENGINE_NAME[dtype], max_batch=n, arch=arch)
    try:
        with pytest.raises(_capi.RtdError):
            _capi.plan_convs("eva", clf._h)
        x = torch.randn((n, 3, arch.img, arch.img), generator=torch.Generator().manual_seed(3)).cuda()
        logits = clf(x)
        torch.cuda.synchronize()
        assert torch.isfinite(logits).all()
        assert_plan_is_the_census(_capi.plan_convs("eva", clf._h), census.eva_launches(n, dtype, arch), by_name=False)
        # ... and the served depth repeats these blocks: the census of the full network is this list with its block 24 times
        full, one = census.eva_launches(n, dtype), census.eva_launches(n, dtype, arch)
        strip = lambda f: {k: v for k, v in f.items() if k != "name"}
        assert [strip(f) for f in full] == [strip(one[0])] + [strip(f) for f in one[1:5]] * census.EVA_ARCH.depth + [strip(one[5])]
    finally:
        clf.close()


@pytest.mark.parametrize("dtype", census.ENGINES)
def test_esrgan_plan_is_the_census(L, dtype):
    _capi.debug_option("reset", 0)
    up = esrgan.CropUpscaler(esrgan_ref.synth_state(1, 0), num_block=1, precision=ENGINE_NAME[dtype], tile=512)
    try:
        with pytest.raises(_capi.RtdError):
            _capi.plan_convs("esrgan", up._h)
        frame = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (128, 128, 3), dtype=np.uint8)).cuda()
        buf, _, shapes = up.upscale([frame], [[(0, 0, 128, 128)]])
        torch.cuda.synchronize()
        assert shapes == [(512, 512)]
        assert_plan_is_the_census(_capi.plan_convs("esrgan", up._h), census.esrgan_launches(128, 128, dtype, num_block=1), by_name=True)
    finally:
        up.close()
