"""Test inputs for the discrete cross-attention sampler of RT-DETRv2's "dsp" checkpoints.  The sampler itself is restated in
oracle/rtdetr_oracle.py (`msdeform_discrete_ref` is the kernel-level reference, any dtype); here are the inputs of the kernel-level
tests and `near_boundary_items`, which names the items whose taps a rounding error may legitimately move.
"""
import json
import os

import numpy as np
import torch

from oracle.rtdetr_oracle import discrete_coords, discrete_taps, msdeform_discrete_ref  # noqa: F401  (the tests import them from here)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def yardstick():
    with open(os.path.join(GOLDEN_DIR, "dsp_yardstick.json")) as fh:
        return json.load(fh)


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
