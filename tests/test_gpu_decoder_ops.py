"""GPU: the kernels between the encoder and the detections - query selection (select_score_kernel, k_gather_ln), the pair-format
converters, the decoder's glue and box kernels, the post-processor and the MS-deformable sampler on the engine's value layout - each
called through its kernel-level entry point and compared with a plain fp64 restatement on the CPU (copies, index kernels and single
exactly rounded operations: bit for bit).

Tolerance of every floating-point comparison: the same operation in torch fp32 on the CPU has the error e_ref against fp64 on these
very inputs; the kernel must stay within FACTOR * (e_ref + ulp(max |ref|)), FACTOR = 4 - a different but legitimate summation order and
__expf / rsqrtf / __logf at 1-2 ulp, with a floor of 4 ulp where torch happens to be exact.  Every case prints its measured error,
e_ref and the ratio err / (e_ref + ulp); DESIGN.md holds the worst ratio per family."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import plateau_keys, topk_path, within

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1
DT = {"bf16": BF16, "f32": F32}


@pytest.fixture(scope="module")
def L():
    from telescope_cam_detection_amd import _capi
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _capi.lib()


def ck(L, rc):
    assert rc == 0, (rc, L.rtd_last_error(None))


def ln_ref(x, g, b, dt):
    x, g, b = x.to(dt), g.to(dt), b.to(dt)
    return F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


# ------------------------------------------------------------------------------------------ query selection
SEL_CASES = [(3, 735, 80),    # S % 16 = 15: tiles straddle image boundaries, no rotation
             (2, 400, 80),    # 25 tiles per image: the chunk rotation wraps past 16
             (1, 16, 80),
             (2, 64, 7),      # one partial class tile
             (2, 64, 91),     # second pass, partial tile
             (1, 48, 200),    # three passes
             (1, 33, 96)]     # second pass of one whole tile


def sel_inputs(B, S, C_, seed):
    """rows whose true class logits are ALL negative (bias mean -6: a zero-padded column would win the max); a third of the rows have
    their winner planted in column C - 1, and with C > 80 another third in a column >= 80 (the later passes)"""
    g_ = torch.Generator().manual_seed(seed)
    rows = B * S
    w = torch.randn(C_, 256, generator=g_) * (0.5 / 16)
    bias = -6.0 + 0.1 * torch.randn(C_, generator=g_)
    gam = 1.0 + 0.1 * torch.randn(256, generator=g_)
    bet = 0.1 * torch.randn(256, generator=g_)
    x = torch.randn(rows, 256, generator=g_)
    want_col = torch.full((rows,), -1, dtype=torch.long)
    for r in range(rows):
        if r % 3 == 0:
            want_col[r] = C_ - 1
        elif r % 3 == 1 and C_ > 80:
            want_col[r] = 80 + (r // 3) % (C_ - 80)
        if want_col[r] >= 0:
            wc = w[want_col[r]]
            x[r] += 0.6 * (wc - wc.mean()) / wc.std()
    x = x * (0.5 + 3.5 * torch.rand(rows, 1, generator=g_)) + 2.0 * torch.randn(rows, 1, generator=g_)
    return x.contiguous(), w.contiguous(), bias, gam, bet, want_col


def sel_ref(x, w, bias, gam, bet, dt):
    return ln_ref(x, gam, bet, dt) @ w.to(dt).t() + bias.to(dt)


def run_select(L, x, w, bias, gam, bet, B, S, C_, ldx=256):
    rows = B * S
    if ldx == 256:
        xd = x.cuda()
        xp = xd.data_ptr()
    else:                                   # the rows as a channel slice (offset 32) of a wider buffer filled with 1e4
        xd = torch.full((rows, ldx), 1.0e4)
        xd[:, 32:32 + 256] = x
        xd = xd.cuda()
        xp = xd.data_ptr() + 32 * 4
    wd, bd, gd, btd = w.cuda(), bias.cuda(), gam.cuda(), bet.cuda()
    mx = torch.full((rows,), float("nan"), device="cuda")
    ck(L, L.rtd_op_select_score(xp, ldx, wd.data_ptr(), bd.data_ptr(), gd.data_ptr(), btd.data_ptr(), mx.data_ptr(), B, S, C_, 256))
    return mx.cpu()


@pytest.mark.parametrize("case", SEL_CASES)
def test_select_score_against_fp64(L, case):
    """select_score_kernel: max over classes of LayerNorm(x) W^T + bias, dense rows and rows sliced out of a 320-wide buffer (the launcher
    takes any row stride that keeps 16-byte rows; the engine itself only uses it dense)"""
    B, S, C_ = case
    x, w, bias, gam, bet, want_col = sel_inputs(B, S, C_, 1000 + SEL_CASES.index(case))
    lg64 = sel_ref(x, w, bias, gam, bet, torch.float64)
    assert (lg64 < 0).all(), "test data: every true logit must be negative"
    planted = want_col >= 0
    assert (lg64.argmax(1)[planted] == want_col[planted]).all(), "test data: the planted column must win its row"
    ref64, ref32 = lg64.max(1).values, sel_ref(x, w, bias, gam, bet, torch.float32).max(1).values
    for ldx in (256, 320):
        got = run_select(L, x, w, bias, gam, bet, B, S, C_, ldx)
        within("select_score", f"{case} ldx {ldx}", got, ref64, ref32)


@pytest.mark.parametrize("S", [400, 735])
def test_select_score_is_batch_invariant_bit_for_bit(L, S):
    """a row's score depends on the row and its position in its image only: image 0 alone == the same rows as image 2 of a batch of 3
    (S = 400: rotated chunk order; S = 735: tiles straddle the images, no rotation), and two images with identical rows agree"""
    x, w, bias, gam, bet, _ = sel_inputs(3, S, 80, 1100 + S)
    alone = run_select(L, x[:S].contiguous(), w, bias, gam, bet, 1, S, 80)
    xb = torch.cat([x[S:2 * S], x[2 * S:], x[:S]], 0).contiguous()          # image 0's rows now image 2
    batch = run_select(L, xb, w, bias, gam, bet, 3, S, 80)
    assert torch.equal(alone.view(torch.int32), batch[2 * S:].view(torch.int32))
    twin = run_select(L, torch.cat([x[:S], x[:S]], 0).contiguous(), w, bias, gam, bet, 2, S, 80)
    assert torch.equal(twin[:S].view(torch.int32), twin[S:].view(torch.int32))
    assert torch.equal(twin[:S].view(torch.int32), alone.view(torch.int32))


@pytest.mark.parametrize("Q", [50, 300])
def test_gather_ln_against_fp64_and_bit_identical_rows(L, Q):
    """k_gather_ln: dst[b][q] = LayerNorm(x[b][idx[b][q]]).  The index rule: an index outside [0, S) is CLAMPED to the nearest valid row
    (-3 reads row 0, S + 5 reads row S - 1).  Repeated indices; ldd 256 and 384 (the columns behind a row stay untouched); the same
    source row gathered at another Q position or from another batch slot gives the same bits."""
    B, S = 2, 735
    g_ = torch.Generator().manual_seed(1200 + Q)
    x = torch.randn(B, S, 256, generator=g_) * (0.5 + 3.5 * torch.rand(B, S, 1, generator=g_)) + 2.0 * torch.randn(B, S, 1, generator=g_)
    x[1, 100] = x[0, 17]                                                     # one row present in both images
    gam = 1.0 + 0.1 * torch.randn(256, generator=g_)
    bet = 0.1 * torch.randn(256, generator=g_)
    idx = torch.randint(0, S, (B, Q), generator=g_, dtype=torch.int32)
    idx[0, 1], idx[0, 2], idx[1, 3], idx[1, 4] = -3, S + 5, S, -1           # clamped
    idx[0, 5], idx[0, 44], idx[1, 9] = 17, 17, 100                            # the shared row, three times
    idx[0, 6], idx[0, 7], idx[1, Q - 1] = S - 1, 0, S - 1
    src = torch.stack([x[b][idx[b].long().clamp(0, S - 1)] for b in range(B)])
    ref64, ref32 = ln_ref(src, gam, bet, torch.float64), ln_ref(src, gam, bet, torch.float32)
    xd, id_, gd, bd = x.cuda(), idx.cuda(), gam.cuda(), bet.cuda()
    for ldd in (256, 384):
        dst = torch.full((B, Q, ldd), 77.0, device="cuda")
        ck(L, L.rtd_op_gather_ln(xd.data_ptr(), 256, S, id_.data_ptr(), B, Q, gd.data_ptr(), bd.data_ptr(), dst.data_ptr(), ldd))
        got = dst.cpu()
        assert (got[..., 256:] == 77.0).all(), "columns behind the row were written"
        within("gather_ln", f"Q {Q} ldd {ldd}", got[..., :256], ref64, ref32)
        bits = got[..., :256].contiguous().view(torch.int32)
        assert torch.equal(bits[0, 5], bits[0, 44]) and torch.equal(bits[0, 5], bits[1, 9])
        assert torch.equal(bits[0, 1], bits[0, 7]) and torch.equal(bits[0, 2], bits[0, 6])      # clamped == the edge rows themselves


# ------------------------------------------------------------------------------------------ pair-format conversion
EDGE_VALUES = [0.0, -0.0, 65504.0, -65504.0, 65520.0, -65520.0, 1.0e6, -1.0e6, float("inf"), -float("inf"), float("nan"),
               2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, -(2.0 ** -25), -1.5 * 2.0 ** -24,
               2047.9, 0.99999, -4095.9, 65503.9, 32767.99,                 # hi rounds up across a binade
               1.0 + 2.0 ** -20, 0.1, -3.0 - 2.0 ** -18, 1024.0 + 2.0 ** -16, 6.0e-5, 6.1e-5, 2.0 ** -14 + 2.0 ** -26]   # lo is an fp16 subnormal


def split_inputs(rows, C_, seed):
    g_ = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C_, generator=g_) * torch.tensor([1.0, 1.0e-3, 3.0e4, 1.0, 1.0e-3][:rows])[:, None]
    flat = x.reshape(-1)
    pos = torch.randperm(flat.numel(), generator=g_)[:len(EDGE_VALUES)]
    flat[pos] = torch.tensor(EDGE_VALUES, dtype=torch.float32)
    return flat.reshape(rows, C_).contiguous().numpy()


def hi_lo_nan_mask(x):
    """uint16 positions (hi and lo word) of the NaN channels of x [rows, C] in its pair storage [rows, 2C]"""
    rows, C_ = x.shape
    m = np.zeros((rows, C_ // 32, 2, 32), bool)
    m[:] = np.isnan(x).reshape(rows, C_ // 32, 1, 32)
    return m.reshape(rows, 2 * C_)


@pytest.mark.parametrize("C_", [32, 96])
@pytest.mark.parametrize("strided", [False, True])
def test_pair_conversion_kernels_match_the_host_mirror_bit_for_bit(L, C_, strided):
    """k_f32_to_split / k_split_to_f32 against _capi.to_split / from_split on the uint16 storage: random rows at three magnitudes plus
    signed zeros, saturation (+-65504, beyond, inf), fp16 subnormal hi and lo halves, hi halves that round up across a binade; dense
    rows and rows of stride 2C with the padding untouched.  A NaN stays a NaN where it was (compared by isnan, not by payload)."""
    from telescope_cam_detection_amd import _capi
    rows, ld = 5, (2 * C_ if strided else C_)
    x = split_inputs(rows, C_, 1300 + C_)
    want = _capi.to_split(x)                                                  # uint16 [rows, 2C]
    nanw = hi_lo_nan_mask(x)
    assert np.isnan(x).sum() == 1
    # fp32 -> pair
    src = torch.full((rows, ld), 123.0)
    src[:, :C_] = torch.from_numpy(x)
    srcd = src.cuda()
    dst = torch.full((rows, 2 * ld), 0x7777, dtype=torch.int16, device="cuda")
    ck(L, L.rtd_op_split_convert(0, srcd.data_ptr(), dst.data_ptr(), rows, C_, ld, ld))
    got = dst.cpu().numpy().view(np.uint16)
    assert (got[:, 2 * C_:] == 0x7777).all(), "padding behind the pair rows was written"
    got = got[:, :2 * C_]
    np.testing.assert_array_equal(got[~nanw], want[~nanw])
    assert np.isnan(got[nanw].view(np.float16)).all() and np.isnan(want[nanw].view(np.float16)).all()
    # pair -> fp32, from the host mirror's storage
    ps = torch.full((rows, 2 * ld), 0x7777, dtype=torch.int16)
    ps[:, :2 * C_] = torch.from_numpy(want.view(np.int16))
    psd = ps.cuda()
    back = torch.full((rows, ld), 123.0, device="cuda")
    ck(L, L.rtd_op_split_convert(1, psd.data_ptr(), back.data_ptr(), rows, C_, ld, ld))
    b = back.cpu().numpy()
    assert (b[:, C_:] == 123.0).all(), "padding behind the fp32 rows was written"
    want_back = _capi.from_split(want)
    nanf = np.isnan(x)
    np.testing.assert_array_equal(b[:, :C_][~nanf].view(np.uint32), want_back[~nanf].view(np.uint32))
    assert np.isnan(b[:, :C_][nanf]).all() and np.isnan(want_back[nanf]).all()
    # round trip on the device: fp32 -> pair -> fp32 == from_split(to_split(x))
    rt = torch.full((rows, ld), 123.0, device="cuda")
    ck(L, L.rtd_op_split_convert(1, dst.data_ptr(), rt.data_ptr(), rows, C_, ld, ld))
    r = rt.cpu().numpy()[:, :C_]
    np.testing.assert_array_equal(r[~nanf].view(np.uint32), want_back[~nanf].view(np.uint32))
    assert np.isnan(r[nanf]).all()


@pytest.mark.parametrize("C_", [32, 96])
def test_count_saturated_counts_hi_halves_only(L, C_):
    """k_count_saturated == a numpy count of |hi| == 65504 over the hi halves; 0x7BFF / 0xFBFF words planted in LO halves do not count"""
    from telescope_cam_detection_amd import _capi
    rows = 5
    s = _capi.to_split(split_inputs(rows, C_, 1400 + C_)).reshape(rows, C_ // 32, 2, 32).copy()
    s[1, 0, 1, 3], s[2, -1, 1, 31], s[4, 0, 1, 0] = 0x7BFF, 0xFBFF, 0x7BFF       # lo halves
    want = int(((s[:, :, 0, :] & 0x7FFF) == 0x7BFF).sum())
    assert want >= 6 and int(((s & 0x7FFF) == 0x7BFF).sum()) == want + 3
    sd = torch.from_numpy(s.reshape(rows, 2 * C_).view(np.int16)).cuda()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ck(L, L.rtd_op_split_convert(2, sd.data_ptr(), cnt.data_ptr(), rows, C_, C_, 0))
    assert int(cnt.item()) == want


# ------------------------------------------------------------------------------------------ glue (bit-exact)
def as_dev(t, dt):
    return (t.to(torch.bfloat16) if dt == BF16 else t.float()).cuda()


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("nrows", [1, 7])
def test_set_rows_exact(L, dt, nrows):
    B, S, C_, ld = 3, 20, 40, 48
    g_ = torch.Generator().manual_seed(1500 + nrows)
    y = torch.randn(B, S, ld, generator=g_)
    vec = torch.randn(C_, generator=g_)
    rows = torch.randperm(S, generator=g_)[:nrows].to(torch.int32)
    yd, vd, rd = as_dev(y, dt), vec.cuda(), rows.cuda()
    want = yd.cpu().clone()
    want[:, rows.long(), :C_] = vec.to(want.dtype)                           # one rounding to the storage type; everything else intact
    ck(L, L.rtd_op_set_rows(dt, yd.data_ptr(), ld, C_, rd.data_ptr(), nrows, S, vd.data_ptr(), B))
    assert torch.equal(yd.cpu().view(torch.int16 if dt == BF16 else torch.int32), want.view(torch.int16 if dt == BF16 else torch.int32))


@pytest.mark.parametrize("rows", [1, 5, 33])
@pytest.mark.parametrize("C_", [1, 15, 16, 17, 80, 91])
def test_rowmax_exact(L, rows, C_):
    """k_rowmax (16 lanes per row; 33 rows x 16 lanes is no multiple of the block): rows of stride C + 3, rows that hold -inf (one of
    them nothing else) and rows whose max sits in the last column"""
    g_ = torch.Generator().manual_seed(1600 + rows * 100 + C_)
    ld = C_ + 3
    x = torch.randn(rows, ld, generator=g_)
    x[:, C_:] = 1.0e9                                                        # behind the row: must not be read
    x[0, :C_] = -float("inf")
    if rows > 1:
        x[1, C_ - 1] = 50.0
        x[rows - 1, 0] = -float("inf")
        x[rows - 1, C_ - 1] = 7.0
    xd = x.cuda()
    out = torch.full((rows,), float("nan"), device="cuda")
    ck(L, L.rtd_op_rowmax(xd.data_ptr(), ld, C_, rows, out.data_ptr()))
    assert torch.equal(out.cpu().view(torch.int32), x[:, :C_].max(1).values.view(torch.int32))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_gather_rows_exact(L, dt):
    """k_gather_rows bf16 / fp32 -> fp32: clamped indices (the rule of k_gather_ln), source rows of stride C + 8, ldd > C untouched"""
    B, S, Q, C_, lds, ldd = 2, 37, 19, 40, 48, 44
    g_ = torch.Generator().manual_seed(1700 + dt)
    src = torch.randn(B, S, lds, generator=g_)
    idx = torch.randint(0, S, (B, Q), generator=g_, dtype=torch.int32)
    idx[0, 0], idx[0, 1], idx[1, 2], idx[1, Q - 1], idx[1, 0] = -5, S + 9, S, 0, S - 1
    sd, id_ = as_dev(src, dt), idx.cuda()
    dst = torch.full((B, Q, ldd), 77.0, device="cuda")
    ck(L, L.rtd_op_gather_rows(dt, sd.data_ptr(), lds, S, id_.data_ptr(), B, Q, C_, dst.data_ptr(), ldd))
    got = dst.cpu()
    want = torch.stack([sd.cpu().float()[b][idx[b].long().clamp(0, S - 1)][:, :C_] for b in range(B)])
    assert (got[..., C_:] == 77.0).all()
    assert torch.equal(got[..., :C_].contiguous().view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.parametrize("bcast", [0, 1])
@pytest.mark.parametrize("dts", [(BF16, F32, F32), (F32, F32, F32)])
def test_add_exact(L, dts, bcast):
    """k_add for the dtype triples the engine instantiates (AIFI tokens bf16 or fp32 + fp32 position table -> fp32; decoder fp32 + fp32
    -> fp32), b per image and b = one [rows][C] tensor read for every image: one exactly rounded fp32 addition"""
    B, rows, C_ = 3, 7, 40
    g_ = torch.Generator().manual_seed(1800 + bcast)
    a = torch.randn(B, rows, C_, generator=g_) * 3
    b = torch.randn(1 if bcast else B, rows, C_, generator=g_)
    ad, bd = as_dev(a, dts[0]), as_dev(b, dts[1])
    yd = torch.full((B, rows, C_), float("nan"), device="cuda")
    ck(L, L.rtd_op_add(dts[0], dts[1], dts[2], ad.data_ptr(), bd.data_ptr(), yd.data_ptr(), B, rows, C_, bcast))
    want = ad.cpu().float() + bd.cpu().float()
    assert torch.equal(yd.cpu().view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------ box chain
def inverse_sigmoid(x, eps=1e-5):
    """HF modeling_rt_detr_v2.inverse_sigmoid"""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


@pytest.mark.parametrize("ldd", [4, 8])
def test_ref_init_against_fp64(L, ldd):
    """k_ref_init: ref_unact = delta + anchors[clamp(idx)] (one exactly rounded addition: bit for bit), ref = sigmoid(ref_unact) against
    fp64; lanes 4..7 of both outputs zero; indices clamped; a masked anchor (FLT_MAX) gives a box of exactly 1"""
    rows, S = 301, 50
    g_ = torch.Generator().manual_seed(1900)
    delta = torch.randn(rows, ldd, generator=g_) * 2
    delta[:, 4:] = 1.0e9
    anchors = torch.randn(S, 4, generator=g_) * 3
    anchors[7] = torch.finfo(torch.float32).max
    idx = torch.randint(0, S, (rows,), generator=g_, dtype=torch.int32)
    idx[0], idx[1], idx[2], idx[3] = -2, S + 4, 7, S
    dd, ad, id_ = delta.cuda(), anchors.cuda(), idx.cuda()
    un = torch.full((rows, 8), float("nan"), device="cuda")
    rf = torch.full((rows, 8), float("nan"), device="cuda")
    ck(L, L.rtd_op_boxes(dd.data_ptr(), ldd, rows, rf.data_ptr(), ad.data_ptr(), id_.data_ptr(), S, un.data_ptr()))
    un, rf = un.cpu(), rf.cpu()
    assert (un[:, 4:] == 0).all() and (rf[:, 4:] == 0).all()
    u32 = delta[:, :4] + anchors[idx.long().clamp(0, S - 1)]
    assert torch.equal(un[:, :4].contiguous().view(torch.int32), u32.contiguous().view(torch.int32))
    assert (rf[2, :4] == 1.0).all()
    within("box chain", f"ref_init ldd {ldd}", rf[:, :4], torch.sigmoid(u32.double()), torch.sigmoid(u32))


def test_box_refine_six_layers_against_fp64(L):
    """k_box_refine iterated six times on the same ref8 as the decoder does, compared after every layer (a drift would show): boxes
    planted at 0, 1, 1e-6, 1 - 1e-6, 1e-5 (the eps itself) and 0.5 - both clamps and the eps of inverse_sigmoid - against every delta
    of +-{0, 1e-3, 5, 20}, plus random rows.  The fp64 chain starts from the fp32 boxes the kernel reads."""
    boxes = [0.0, 1.0, 1.0e-6, 1.0 - 1.0e-6, 1.0e-5, 0.5]
    deltas = [0.0, 1.0e-3, -1.0e-3, 5.0, -5.0, 20.0, -20.0]
    g_ = torch.Generator().manual_seed(2000)
    ref = torch.tensor([[bx] * 4 for bx in boxes for _ in deltas])
    dl = torch.tensor([[d, d, -d, d] for _ in boxes for d in deltas])
    ref = torch.cat([ref, torch.rand(214, 4, generator=g_)])
    dl = torch.cat([dl, torch.randn(214, 4, generator=g_)])
    rows = ref.shape[0]
    ref8 = torch.zeros(rows, 8)
    ref8[:, :4] = ref
    ref8[:, 4:] = 0.25                                                       # lanes 4..7 are not the kernel's to touch
    rd, dd = ref8.cuda(), dl.contiguous().cuda()
    r64, r32 = ref.double(), ref.clone()
    for layer in range(6):
        ck(L, L.rtd_op_boxes(dd.data_ptr(), 4, rows, rd.data_ptr(), None, None, 0, None))
        r64 = torch.sigmoid(dl.double() + inverse_sigmoid(r64))
        r32 = torch.sigmoid(dl + inverse_sigmoid(r32))
        got = rd.cpu()
        assert (got[:, 4:] == 0.25).all()
        within("box chain", f"box_refine layer {layer}", got[:, :4], r64, r32)


# ------------------------------------------------------------------------------------------ post-processor
POST_CASES = [(2, 50, 80, 50, "spread"), (1, 300, 80, 300, "spread"), (2, 300, 91, 300, "spread"),
              (1, 300, 110, 300, "spread"),     # Q * C > 32768: the one-launch form must decline
              (1, 7, 3, 7, "spread"),
              (2, 300, 80, 300, "eighths"),     # logits quantised to 1/8: many sigmoid ties, some across the cut
              # the cases above stay on k_topk's fast path (at most 1024 candidates); these leave it in the one-launch form too:
              (2, 300, 80, 300, "flat"),        # one score everywhere: 24 000 candidates, the tie group walked in index order
              (2, 300, 80, 300, "plateau"),     # a tie group of 200 at the cut, wholly taken
              (1, 16, 80, 16, "flat")]          # 1 280 candidates: the smallest shape that leaves the fast path
POST_PATHS = {"flat": "general/in-order", "plateau": "general/all-ties"}          # tests.util.topk_path; every other kind: "fast"


@pytest.mark.parametrize("case", POST_CASES)
def test_postprocess_fused_and_three_launch_forms(L, case):
    """block6 = [label, score, x1, y1, x2, y2] of the K best of sigmoid(logits) over Q * C (ties: lowest flat index first), label =
    index % C, query = index // C, cxcywh -> xyxy * (w, h, w, h): the one-launch POST form of k_topk == k_pp_scores + k_topk + k_pp_gather
    bit for bit; labels and queries exact and scores / boxes to the tolerance rule against torch in fp64.  sigmoid is monotone, so the
    expected order is that of the logits themselves: "spread" logits are a shuffled even grid over [-9, 5] (neighbouring scores differ by
    far more than an fp32 rounding, so the order does not depend on how a sigmoid rounds), "eighths" are random multiples of 1/8, "flat" is
    -1.25 everywhere and "plateau" is tests.util.plateau_keys - 3 (logits -2, with 100 at 0 and 200 at -1)."""
    B, Q, C_, K, kind = case
    g_ = torch.Generator().manual_seed(2100 + POST_CASES.index(case))
    if kind == "flat":
        logits = torch.full((B, Q, C_), -1.25)
    elif kind == "plateau":
        logits = (plateau_keys(B, Q * C_, K) - 3.0).view(B, Q, C_)
    elif kind == "eighths":
        logits = torch.round((torch.randn(B, Q, C_, generator=g_) * 2.0 - 3.0) * 8) / 8
    else:
        logits = torch.stack([torch.linspace(-9.0, 5.0, Q * C_)[torch.randperm(Q * C_, generator=g_)] for _ in range(B)]).view(B, Q, C_)
    ref8 = torch.zeros(B, Q, 8)
    ref8[..., :2] = torch.rand(B, Q, 2, generator=g_)
    ref8[..., 2:4] = torch.rand(B, Q, 2, generator=g_) * 0.5 + 0.01
    scale = torch.tensor([[1920.0, 1080.0], [641.0, 479.0]])[:B].contiguous()
    ld, rd, sd = logits.cuda(), ref8.cuda(), scale.cuda()
    out = {}
    for fused in (1, 0):
        blk = torch.full((B, K, 6), float("nan"), device="cuda")
        rc = L.rtd_op_postprocess(ld.data_ptr(), rd.data_ptr(), sd.data_ptr(), B, Q, C_, K, fused, blk.data_ptr())
        if fused and Q * C_ > 32768:
            assert rc != 0, "the one-launch form keeps Q * C <= 32768 keys in registers: it must decline, not fall back"
            continue
        ck(L, rc)
        out[fused] = blk.cpu()
    if 1 in out:
        assert torch.equal(out[1].view(torch.int32), out[0].view(torch.int32))
    got = out[0]
    flat = logits.reshape(B, Q * C_)
    order = np.stack([np.lexsort((np.arange(Q * C_), -flat[b].double().numpy()))[:K] for b in range(B)])     # (logit desc, index asc)
    order = torch.from_numpy(order)
    for b in range(B):      # sigmoid is strictly increasing over these logits: the kernel's keys order and tie as the logits do
        assert topk_path(flat[b].numpy(), K) == POST_PATHS.get(kind, "fast"), ("test data: the path this case is here for", case, b)
    if kind == "eighths":
        kth = torch.gather(flat, 1, order[:, K - 1:K])
        assert ((flat == kth).sum(1) > 1).all(), "test data: a tie group at the cut"
    label, query = order % C_, order // C_
    assert torch.equal(got[..., 0], label.float())
    sel64 = torch.gather(flat, 1, order).double()
    within("postprocess", f"{case} scores", got[..., 1], torch.sigmoid(sel64), torch.sigmoid(sel64.float()))

    def boxes(dt):
        r = torch.gather(ref8[..., :4].to(dt), 1, query[..., None].expand(B, K, 4))
        cx, cy, w, h = r.unbind(-1)
        s = scale.to(dt)[:, None, :]
        return torch.stack([(cx - 0.5 * w) * s[..., 0], (cy - 0.5 * h) * s[..., 1], (cx + 0.5 * w) * s[..., 0], (cy + 0.5 * h) * s[..., 1]], -1)

    within("postprocess", f"{case} boxes", got[..., 2:], boxes(torch.float64), boxes(torch.float32))
    # the query index itself: the centre of every output box names one query
    cx_got = (got[..., 2] + got[..., 4]).double() / 2 / scale[:, None, 0].double()
    nearest = (cx_got[..., None] - ref8[..., 0].double()[:, None, :]).abs().argmin(-1)
    assert torch.equal(nearest, query)


# ------------------------------------------------------------------------------------------ sampler
def msdeform_ref(value, offaw, ref, heads, hd, shapes, n_points, offset_scale, dt):
    """HF modeling_rt_detr_v2 multi-scale deformable attention ("default" method) restated in dtype `dt`; value [B, S, heads * hd]"""
    value, offaw, ref = value.to(dt), offaw.to(dt), ref.to(dt)
    B, S, _ = value.shape
    Q, Lv = ref.shape[1], len(shapes)
    LP = Lv * n_points
    off = offaw[..., : heads * LP * 2].view(B, Q, heads, LP, 2)
    aw = torch.softmax(offaw[..., heads * LP * 2:].view(B, Q, heads, LP), -1)
    r = ref[:, :, None, None, :]
    scale = torch.tensor(1.0 / n_points, dtype=torch.float32).to(dt)         # the model's fp32 1 / n_points (the kernel's pscale)
    loc = r[..., :2] + off * scale * r[..., 2:] * offset_scale
    grids = (2 * loc - 1).permute(0, 2, 1, 3, 4).flatten(0, 1)
    vlist = value.view(B, S, heads, hd).permute(0, 2, 3, 1).flatten(0, 1).split([h * w for h, w in shapes], dim=-1)
    samp = []
    for l, (h, w) in enumerate(shapes):
        samp.append(F.grid_sample(vlist[l].reshape(B * heads, hd, h, w), grids[:, :, l * n_points:(l + 1) * n_points],
                                  mode="bilinear", padding_mode="zeros", align_corners=False))
    a = aw.permute(0, 2, 1, 3).reshape(B * heads, 1, Q, LP)
    return (torch.cat(samp, -1) * a).sum(-1).view(B, heads * hd, Q).transpose(1, 2).contiguous()


def grid_locations(shapes):
    """(x, y) sampling locations that put a bilinear tap, in at least one level, exactly on a pixel centre, half-way between two, on the
    edge of the zero padding (pixel coordinate -0.5 and W - 0.5), one pixel outside and far outside (+-3): the kernel's
    ix = loc * W - 0.5 inverted"""
    pts = []
    for h, w in shapes:
        xs = [0.5 / w, (w - 0.5) / w, min(1.0, 1.0 / w), 0.0, 1.0, -0.5 / w, (w + 0.5) / w, 3.0, -3.0]
        ys = [0.5 / h, (h - 0.5) / h, min(1.0, 1.0 / h), 0.0, 1.0, -0.5 / h, (h + 0.5) / h, -3.0, 3.0]
        pts += list(zip(xs, ys))
        pts += [(xs[0], ys[4]), (xs[3], ys[1]), (xs[2], ys[5])]
    return pts


MSD_CASES = [
    # B, Q, heads, level shapes, n_points, value_coff
    (2, 75, 8, [(6, 8), (1, 7), (5, 1)], 4, 256),
    (2, 75, 8, [(1, 1)], 1, 0),
    (2, 75, 8, [(4, 4), (1, 1)], 3, 512),
    (2, 75, 8, [(6, 8), (3, 5), (1, 7), (5, 1)], 2, 256),
    (1, 75, 8, [(6, 8), (1, 7), (5, 1)], 4, 512),
    (1, 75, 5, [(6, 8), (1, 7), (5, 1)], 4, 256),     # 375 (query, head) items: the last block of 8 items is partial
]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", MSD_CASES)
def test_msdeform_on_a_channel_slice_of_the_value_buffer(L, dt, case):
    """k_msdeform<DEC_DEFAULT, ...> as the engine calls it: the layer's channels at offset value_coff of 768-wide value rows (the other slices hold 1e4),
    batch stride S * 768; levels x points 3 x 4, 1 x 1, 2 x 3, 4 x 2 with 1 x 1, 1 x 7 and 5 x 1 maps; a grid of locations with zero
    offsets (grid_locations) next to random ones with large offsets; attention logits all equal and with one +40 entry."""
    B, Q, heads, shapes, n_points, coff = case
    hd, ldv, Lv = 32, 768, len(shapes)
    D, LP = heads * hd, len(shapes) * n_points
    S = sum(h * w for h, w in shapes)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    g_ = torch.Generator().manual_seed(2200 + MSD_CASES.index(case))
    value = torch.randn(B, S, D, generator=g_).to(tdt).float()               # the values the kernel sees
    offaw = torch.randn(B, Q, heads * LP * 3, generator=g_) * 2.0
    ref = torch.rand(B, Q, 4, generator=g_)
    ref[..., 2:] = ref[..., 2:] * 0.5 + 0.05
    ref[0, Q - 1] = 1.0                                                       # the masked-anchor reference box, large offsets
    pts = grid_locations(shapes)[:Q - 8]
    for i, (px, py) in enumerate(pts):
        ref[:, i, 0], ref[:, i, 1] = px, py
        offaw[:, i, : heads * LP * 2] = 0.0
    awl = offaw[..., heads * LP * 2:].view(B, Q, heads, LP)
    awl[:, 0::5] = 0.25                                                       # all-equal logits
    awl[:, 1::5, :, 0] = 40.0                                                 # one saturating entry (first ...
    awl[:, 2::5, :, LP - 1] = 40.0                                            # ... or last tap)
    buf = torch.full((B, S, ldv), 1.0e4)
    buf[..., coff:coff + D] = value
    vd, od, rd = buf.to(tdt).cuda(), offaw.cuda(), ref.cuda()
    out = torch.full((B, Q, D), float("nan"), device="cuda")
    lv = (C.c_int32 * (2 * Lv))(*[v for hw in shapes for v in hw])
    ck(L, L.rtd_op_msdeform_view(DT[dt], vd.data_ptr(), ldv, coff, od.data_ptr(), rd.data_ptr(), out.data_ptr(), B, Q, heads, hd, Lv, n_points, lv, 0.5))
    ref64 = msdeform_ref(value, offaw, ref, heads, hd, shapes, n_points, 0.5, torch.float64)
    ref32 = msdeform_ref(value, offaw, ref, heads, hd, shapes, n_points, 0.5, torch.float32)
    within("msdeform", f"{dt} {case}", out.cpu(), ref64, ref32)

