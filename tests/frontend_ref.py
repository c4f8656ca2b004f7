"""Plain references of the f16x3 front end (csrc/ops.hip stem0_u8_kernel): backbone.stem.0 straight from uint8 BGR frames, in fp64 on
the values the kernel sees, and the tap-map launch whose output words are known exactly; checked against torch's own
conv2d in tests/test_frontend_host.py before any kernel is held to them."""
import numpy as np

from telescope_cam_detection_amd import _capi

TAPS, REAL = 9, 27            # 3 x 3 taps; 27 real (tap, RGB channel) filter columns of the 72 (8 padded channels per tap)


# (n, H, W) at the kernel's own tile scale - a block is 8 x 32 output pixels from a 17 x 65 pixel patch, 4 waves x 2 rows: exactly one tile;
# 2 x 2 tiles with one row / one column in the last ones; odd extents (201-byte rows walk through all four row-start alignments, the last
# output row and column read taps outside the frame); interior tiles and three images; two frames smaller than one patch (12 and 45 bytes)
SHAPES = [(1, 16, 64), (2, 18, 66), (2, 17, 67), (3, 48, 160), (1, 2, 2), (1, 3, 5)]


def operands(n, H, W):
    """seeded by the shape: n uniform random frames, w = randn * 27^-1/2 with 1e3 in the pad channels 3..7, bias = 0.1 randn"""
    rng = np.random.default_rng(1000 * n + 100 * H + W)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    w = (rng.standard_normal((32, 3, 3, 8)) * 27 ** -0.5).astype(np.float32)
    w[:, :, :, 3:] = 1e3
    bias = (0.1 * rng.standard_normal(32)).astype(np.float32)
    return frames, w, bias


def out_extent(n):
    """3 / stride 2 / pad 1"""
    return (n - 1) // 2 + 1


def pair_round(a):
    """fp32 values of any shape -> the fp32 value of their hi + lo fp16 pair (_capi.to_split / from_split: 32-channel rows)."""
    a = np.ascontiguousarray(a, np.float32)
    flat = np.zeros((a.size + 31) // 32 * 32, np.float32)
    flat[: a.size] = a.ravel()
    return _capi.from_split(_capi.to_split(flat.reshape(-1, 32))).ravel()[: a.size].reshape(a.shape)


def pixels_seen(frame_u8):
    """[H, W, 3] uint8 BGR -> fp32 [H, W, 3] RGB: float32(v) / float32(255) as a hi + lo pair."""
    x = np.asarray(frame_u8, np.uint8).astype(np.float32) / np.float32(255.0)
    return pair_round(x)[:, :, ::-1]                # frame byte cb -> model channel 2 - cb


def activation(y, act):
    if act == _capi.ACT["none"]:
        return y
    if act == _capi.ACT["relu"]:
        return np.maximum(y, 0.0)
    if act == _capi.ACT["silu"]:
        return y / (1.0 + np.exp(-y))
    raise ValueError(f"stem0: no activation {act}")


def stem0_ref(frames_u8, w, bias, act):
    """fp64 [n, OH, OW, 32]: act(conv3x3 / stride 2 / pad 1 (pixels, w) + bias).  frames_u8: n [H, W, 3] uint8 BGR frames of one size,
    w [32, 3, 3, 8] fp32 (OHWI, channels RGB + 5 pad that are never read), bias [32].  Pixels and filter as pairs; the rest in fp64."""
    wv = pair_round(np.asarray(w, np.float32)[:, :, :, :3]).astype(np.float64)                   # [32, kh, kw, rgb]
    H, W = frames_u8[0].shape[:2]
    OH, OW = out_extent(H), out_extent(W)
    y = np.zeros((len(frames_u8), OH, OW, 32), np.float64)
    for b, f in enumerate(frames_u8):
        assert f.shape == (H, W, 3)
        xp = np.zeros((H + 2, W + 2, 3), np.float64)
        xp[1: H + 1, 1: W + 1] = pixels_seen(f)
        for kh in range(3):
            for kw in range(3):
                win = xp[kh: kh + 2 * OH - 1: 2, kw: kw + 2 * OW - 1: 2]                         # [OH, OW, rgb]
                y[b] += win @ wv[:, kh, kw, :].T
    return activation(y + np.asarray(bias, np.float64), act)


def tap_map_filter():
    """(w [32, 3, 3, 8], bias [32]): output channel c < 27 copies tap c // 3 (kh = tap // 3, kw = tap % 3), RGB channel c % 3."""
    w = np.zeros((32, 3, 3, 8), np.float32)
    for c in range(REAL):
        tap, ch = divmod(c, 3)
        w[c, tap // 3, tap % 3, ch] = 1.0
    return w, np.zeros(32, np.float32)


def tap_map_words(frames):
    """uint16 [n, OH, OW, 64]: the pair words the tap-map launch must write, exactly.  Channel c < 27 of output pixel (oy, ox) is the
    pixel value v = hi + lo at row 2 oy - 1 + kh, column 2 ox - 1 + kw (0 outside the frame): the kernel's sum is hi * 1 + lo * 1 plus
    exact zeros, exact in fp32, and the epilogue splits it again."""
    H, W = frames[0].shape[:2]
    OH, OW = out_extent(H), out_extent(W)
    v = np.zeros((len(frames), OH, OW, 32), np.float32)
    for b, f in enumerate(frames):
        x = pixels_seen(f)
        for oy in range(OH):
            for ox in range(OW):
                for tap in range(TAPS):
                    iy, ix = 2 * oy - 1 + tap // 3, 2 * ox - 1 + tap % 3
                    if 0 <= iy < H and 0 <= ix < W:
                        v[b, oy, ox, 3 * tap: 3 * tap + 3] = x[iy, ix]
    return _capi.to_split(v)


FILLER = 4096


class Placed:
    """frames (uint8 arrays) in one device buffer filled with `fill`: frame i starts offs[i] bytes past a 16-byte boundary, >= FILLER
    bytes after the previous frame's end, and FILLER bytes of filler follow the last one."""

    def __init__(self, frames, offs, fill):
        pos, end = [], 0
        for f, off in zip(frames, offs):
            pos.append((end + FILLER + 15) // 16 * 16 + off)
            end = pos[-1] + f.size
        host = np.full(end + FILLER, fill, np.uint8)
        for f, p in zip(frames, pos):
            host[p: p + f.size] = f.ravel()
        import torch
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptrs = [self.buf.data_ptr() + p for p in pos]
        self.views = [self.buf[p: p + f.size].view(f.shape) for f, p in zip(frames, pos)]
        assert all(v.data_ptr() == p and v.is_contiguous() for v, p in zip(self.views, self.ptrs))
        torch.cuda.synchronize()
