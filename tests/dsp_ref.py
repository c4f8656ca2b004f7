"""The discrete cross-attention sampler of RT-DETRv2's "dsp" checkpoints (`cross_attn_method: discrete`; HF modeling_rt_detr_v2.py
multi_scale_deformable_attention_v2, branch method == "discrete", and the module above it), restated for the tests:

  off = ((offset * (1 / n_points)) * ref_wh) * offset_scale        loc = ref_xy + off
  cx = int(loc_x * W + 0.5), cy = int(loc_y * H + 0.5)             (conversion truncates toward zero)
  then clamped to [0, W - 1] / [0, H - 1]; the output is the attention-weighted sum of value[cy, cx].

`msdeform_discrete_ref` is the kernel-level reference (any dtype), `discrete_oracle()` turns oracle/rtdetr_oracle.py into the dsp
yardstick without editing it, `near_boundary_items` names the items whose taps a rounding error may legitimately move.
"""
import contextlib
import json
import os

import numpy as np
import torch

from oracle import rtdetr_oracle as orc
from telescope_cam_detection_amd.arch import ARCHS
from telescope_cam_detection_amd.synth import make_frame

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixture -> arch (the .npz carries seeds / sizes / frame list itself, as the c* / t* files do)
DSP_CASE_ARCH = {"d1_r18dsp_160x224": "r18_dsp", "d2_tinycdsp_160x224": "tinyc_dsp"}


def load_dsp_case(name):
    """(arch, weight seed, input size, frames, npz) of a d* fixture: tests.util.load_case for the dsp files"""
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    wseed, ih, iw, n = (int(v) for v in g["meta"])
    frames = [make_frame(str(g["kind"]), int(s), int(h), int(w)) for s, h, w in g["frames"]]
    return ARCHS[DSP_CASE_ARCH[name]], wseed, (ih, iw), frames, g


def yardstick():
    with open(os.path.join(GOLDEN_DIR, "dsp_yardstick.json")) as fh:
        return json.load(fh)


def discrete_coords(off, ref, shapes, n_points, offset_scale):
    """off [B, Q, heads, LP, 2], ref [B, Q, 4] in one dtype -> the un-truncated tap coordinates loc * (W, H) + 0.5, [B, Q, heads, LP, 2]
    (x, y), every product and sum rounded on its own in that dtype and in HF's order"""
    dt = off.dtype
    scale = torch.tensor(1.0 / n_points, dtype=torch.float32).to(dt)         # the model's fp32 1 / n_points (n_points_scale)
    r = ref[:, :, None, None, :]
    loc = r[..., :2] + off * scale * r[..., 2:] * offset_scale
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=dt).repeat_interleave(n_points, 0)     # [LP, 2]: (W, H) of each tap's level
    return loc * wh + 0.5


def discrete_taps(coords, shapes, n_points):
    """coordinates -> flat token index [B, Q, heads, LP] into the concatenated level maps: truncate toward zero, clamp into the map"""
    c = coords.to(torch.int64)                                              # torch truncates toward zero
    w = torch.tensor([w for _, w in shapes]).repeat_interleave(n_points)
    h = torch.tensor([h for h, _ in shapes]).repeat_interleave(n_points)
    start = torch.tensor(np.cumsum([0] + [hh * ww for hh, ww in shapes])[:-1]).repeat_interleave(n_points)
    cx = torch.minimum(c[..., 0].clamp(min=0), w - 1)
    cy = torch.minimum(c[..., 1].clamp(min=0), h - 1)
    return start + cy * w + cx


def msdeform_discrete_ref(value, offaw, ref, heads, hd, shapes, n_points, offset_scale, dt):
    """HF's multi-scale deformable attention with method "discrete", restated in dtype `dt`; value [B, S, heads * hd], offaw
    [B, Q, heads * LP * 3] (offsets | attention logits), ref [B, Q, 4]: the signature of msdeform_ref in tests/test_gpu_decoder_ops.py.
    Returns (output [B, Q, heads * hd], un-truncated tap coordinates [B, Q, heads, LP, 2])."""
    value, offaw, ref = value.to(dt), offaw.to(dt), ref.to(dt)
    B, S, _ = value.shape
    Q, LP = ref.shape[1], len(shapes) * n_points
    off = offaw[..., : heads * LP * 2].view(B, Q, heads, LP, 2)
    aw = torch.softmax(offaw[..., heads * LP * 2:].view(B, Q, heads, LP), -1)
    coords = discrete_coords(off, ref, shapes, n_points, offset_scale)
    idx = discrete_taps(coords, shapes, n_points)                           # [B, Q, heads, LP]
    v = value.view(B, S, heads, hd).permute(0, 2, 1, 3)                     # [B, heads, S, hd]
    gi = idx.permute(0, 2, 1, 3).reshape(B, heads, Q * LP, 1).expand(-1, -1, -1, hd)
    taps = v.gather(2, gi).view(B, heads, Q, LP, hd)
    out = (taps * aw.permute(0, 2, 1, 3)[..., None]).sum(3)                 # [B, heads, Q, hd]
    return out.permute(0, 2, 1, 3).reshape(B, Q, heads * hd).contiguous(), coords


def ms_deform_attn_discrete(arch, w, pfx, hs, pos, ref, memory, shapes):
    """oracle.rtdetr_oracle.ms_deform_attn with the discrete sampler (same arguments, same projections)"""
    B, Q, D = hs.shape
    H, LP = arch.dec_heads, arch.n_levels * arch.n_points
    q = hs + pos
    value = orc.linear(w, pfx + ".vp", memory)
    offaw = torch.cat([orc.linear(w, pfx + ".off", q), orc.linear(w, pfx + ".aw", q)], -1)
    assert offaw.shape[-1] == H * LP * 3
    o, _ = msdeform_discrete_ref(value, offaw, ref, H, D // H, shapes, arch.n_points, arch.offset_scale, hs.dtype)
    return orc.linear(w, pfx + ".op", o)


@contextlib.contextmanager
def discrete_oracle():
    """inside the block oracle.rtdetr_oracle samples as the dsp checkpoints do: decoder_and_heads looks ms_deform_attn up in its module,
    so orc.model_forward and orc.detect_batch become the discrete yardstick; the bilinear function is put back on the way out"""
    saved = orc.ms_deform_attn
    orc.ms_deform_attn = ms_deform_attn_discrete
    try:
        yield orc
    finally:
        orc.ms_deform_attn = saved


def near_boundary_items(coords, shapes, delta):
    """coords [B, Q, heads, LP, 2] (x, y; LP = levels * points) -> bool [B, Q, heads]: the items with a tap coordinate c that lies within
    delta of an integer without being one (0 < |c - round(c)| < delta) and inside (-1, extent + 1) - a rounding error of the
    coordinate may move such a tap, so a comparison leaves the item out.  A coordinate exactly ON an integer is kept."""
    c = coords.double()
    LP = c.shape[3]
    n_points = LP // len(shapes)
    ext = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).repeat_interleave(n_points, 0)     # [LP, 2]
    d = (c - torch.round(c)).abs()
    near = (d > 0) & (d < delta) & (c > -1) & (c < ext + 1)
    return near.flatten(3).any(-1)


# ---- the inputs of the kernel-level test (tests/test_gpu_dsp.py) and of its CPU twin (tests/test_dsp_oracle.py) ----
MSD_LDV = 768            # width of the value rows the layer's channels are a slice of
MSD_DELTA = 1e-4         # px: items with a coordinate this close to an integer (but not on it) are left out of the comparison
MSD_CASES = [
    # B, Q, heads, level shapes (power-of-two extents: the exact-boundary grid exists), n_points, value_coff
    (2, 75, 8, [(8, 8), (2, 4), (4, 1)], 4, 256),
    (2, 75, 8, [(1, 1)], 1, 0),
    (2, 75, 8, [(4, 4), (1, 1)], 3, 512),
    (1, 75, 5, [(16, 8), (1, 4), (4, 1)], 4, 256),     # 375 (query, head) items: the last block of 8 items is partial
]


def boundary_locations(shapes):
    """(x, y) locations k / (2 W), k / (2 H) around both ends and the middle of every level: with zero offsets the coordinate
    c = loc * W + 0.5 = (k + 1) / 2 is exact in fp32 and fp64 alike (power-of-two extents), an integer for odd k - the tap changes
    exactly there - and a half for even k.  They pin the truncation toward zero (c = -0.5 -> 0), the + 0.5 step and both clamps
    (c = -1 -> 0, c = W -> W - 1); two points per level lie 3 maps outside."""
    pts = []
    for h, w in shapes:
        ks = lambda n: [-3, -2, -1, 0, 1, 2, 3, n - 1, n, n + 1, 2 * n - 3, 2 * n - 2, 2 * n - 1, 2 * n, 2 * n + 1, 2 * n + 2, 2 * n + 3]
        pts += [(kx / (2.0 * w), ky / (2.0 * h)) for kx, ky in zip(ks(w), ks(h))]
        pts += [(3.0, -3.0), (-3.0, 3.0)]
    return pts


def msd_inputs(case, dt):
    """the inputs of test_msdeform_on_a_channel_slice_of_the_value_buffer (tests/test_gpu_decoder_ops.py) for the discrete sampler:
    the layer's channels at offset value_coff of 768-wide value rows whose other slices hold 1e4; attention logits all equal and with
    one +40 entry; the masked-anchor box ref = 1 with large offsets; the exact-boundary grid with zero offsets next to random
    locations.  dt "f32" | "bf16" = the storage of the value rows.  Returns (value [B, S, D] as the kernel sees it, the 768-wide
    buffer, offaw, ref)."""
    B, Q, heads, shapes, n_points, coff = case
    hd = 32
    D, LP = heads * hd, len(shapes) * n_points
    S = sum(h * w for h, w in shapes)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    g_ = torch.Generator().manual_seed(3300 + MSD_CASES.index(case))
    value = torch.randn(B, S, D, generator=g_).to(tdt).float()
    offaw = torch.randn(B, Q, heads * LP * 3, generator=g_) * 2.0
    ref = torch.rand(B, Q, 4, generator=g_)
    ref[..., 2:] = ref[..., 2:] * 0.5 + 0.05
    ref[0, Q - 1] = 1.0                                                       # the masked-anchor reference box ...
    offaw[0, Q - 1, : heads * LP * 2] *= 50.0                                 # ... with offsets that leave every map by far
    pts = boundary_locations(shapes)[:Q - 8]
    for i, (px, py) in enumerate(pts):
        ref[:, i, 0], ref[:, i, 1] = px, py
        offaw[:, i, : heads * LP * 2] = 0.0
    awl = offaw[..., heads * LP * 2:].view(B, Q, heads, LP)
    awl[:, 0::5] = 0.25                                                       # all-equal logits
    awl[:, 1::5, :, 0] = 40.0                                                 # one saturating entry (first ...
    awl[:, 2::5, :, LP - 1] = 40.0                                            # ... or last tap)
    buf = torch.full((B, S, MSD_LDV), 1.0e4)
    buf[..., coff:coff + D] = value
    return value, buf.to(tdt), offaw, ref


# ---- the rounding ORDER of the tap coordinate: inputs where op-by-op fp32 and fused multiply-adds pick different taps ----
ROUNDING_SHAPES = [(20, 28), (10, 14), (5, 7)]       # the level maps of a 160 x 224 input
ROUNDING_POINTS = 4
ROUNDING_OFFSET_SCALE = 0.3                          # no power of two: (offset * scale) is rounded before it is added to the reference
                                                     # (with the models' 0.5 that product is exact and a fused add changes nothing)


def _tap32(loc, ext):
    c = np.float32(np.float32(np.float32(loc) * np.float32(ext)) + np.float32(0.5))
    return int(np.clip(int(c), 0, ext - 1))


def _step32(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(4.0 if k > 0 else -4.0), dtype=np.float32)
    return x


def rounding_order_locations(shapes=ROUNDING_SHAPES, scale=ROUNDING_OFFSET_SCALE):
    """[(level, axis, ref, offset, tap op by op, tap fused)] with ref_wh = 1 and n_points = 4: for every tap boundary N of every level
    and axis, a reference and an offset for which loc = fl(ref + fl(t * scale)), t = offset / 4, as torch computes it op by op, is the
    first fp32 location of tap N, while loc = fl(ref + t * scale), one fused multiply-add, is the last location of tap N - 1 (or the
    other way round).  Constructed, not searched at random: the sum is aimed at the midpoint between those two locations and the few
    fp32 neighbours of t are tried.  The fused side is evaluated exactly in fp64 (a product of two fp32 and its sum with a third fit a
    double here)."""
    s32 = np.float32(scale)
    out = []
    for l, (h, w) in enumerate(shapes):
        for axis, ext in ((0, w), (1, h)):
            for n in range(1, ext):
                lb = np.float32((n - 0.5) / ext)
                while _tap32(lb, ext) >= n:
                    lb = _step32(lb, -1)
                while _tap32(lb, ext) < n:
                    lb = _step32(lb, 1)                                   # the first location whose tap is n
                mid = (np.float64(_step32(lb, -1)) + np.float64(lb)) / 2
                ref = np.float32(lb - np.float32(0.1))
                t0 = np.float32((mid - np.float64(ref)) / np.float64(s32))
                for k in range(-12, 13):
                    t = _step32(t0, k)
                    loc_op = np.float32(ref + np.float32(t * s32))
                    loc_fused = np.float32(np.float64(ref) + np.float64(t) * np.float64(s32))
                    c_fused = np.float32(np.float64(loc_fused) * ext + 0.5)
                    t_op, t_fused = _tap32(loc_op, ext), int(np.clip(int(c_fused), 0, ext - 1))
                    if t_op != t_fused:
                        out.append((l, axis, float(ref), float(np.float32(t * np.float32(4.0))), t_op, t_fused))
                        break
    return out


def rounding_order_inputs():
    """one query per entry of rounding_order_locations(): the offset on the first point of the entry's level, a +80 logit on that point
    so that the output IS that tap's value row, and value rows that spell their own position: channel 0 = x, 1 = y, 2 = level, the rest
    0.  The other axis sits inside a pixel, far from its edges, with a zero offset.  One head, ref_wh = 1.  Returns (value [1, S, 32], offaw
    [1, Q, 36], ref [1, Q, 4], expected [Q, 3] = (x, y, level) of the op-by-op tap, the same for the fused evaluation)."""
    shapes, P = ROUNDING_SHAPES, ROUNDING_POINTS
    locs = rounding_order_locations(shapes)
    Q, LP = len(locs), len(shapes) * P
    S = sum(h * w for h, w in shapes)
    value = torch.zeros(1, S, 32)
    s0 = 0
    for l, (h, w) in enumerate(shapes):
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        value[0, s0:s0 + h * w, 0], value[0, s0:s0 + h * w, 1], value[0, s0:s0 + h * w, 2] = xs.flatten().float(), ys.flatten().float(), float(l)
        s0 += h * w
    offaw = torch.zeros(1, Q, LP * 3)
    ref = torch.ones(1, Q, 4)
    want_op, want_fused = torch.zeros(Q, 3), torch.zeros(Q, 3)
    for q, (l, axis, r, offset, t_op, t_fused) in enumerate(locs):
        other_ext = shapes[l][0] if axis == 0 else shapes[l][1]
        o_tap = other_ext // 2
        ref[0, q, axis], ref[0, q, 1 - axis] = r, (o_tap + 0.25) / other_ext          # c = o_tap + 0.75: far from a boundary
        offaw[0, q, (l * P) * 2 + axis] = offset
        offaw[0, q, LP * 2 + l * P] = 80.0
        for want, t in ((want_op, t_op), (want_fused, t_fused)):
            want[q, axis], want[q, 1 - axis], want[q, 2] = float(t), float(o_tap), float(l)
    return value, offaw, ref, want_op, want_fused
