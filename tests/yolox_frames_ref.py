"""The YOLOX uint8 front end restated in numpy float32, in the kernel's operation order (csrc/yolox_net_host.h frame_tap / frame_blend,
csrc/yolox_net.hip yolox_focus_u8): the reference's `F.interpolate(frame.float(), mode="bilinear", align_corners=False)` from the bytes.

    sy = f32(h) / f32(in_h)                       fy = max(sy * (f32(y) + 0.5) - 0.5, 0)          (every operation one fp32 rounding)
    y0 = min(int(fy), h - 1)   y1 = min(y0 + 1, h - 1)   ly1 = fy - f32(y0)   ly0 = 1 - ly1       (x likewise)
    R[c][y][x] = ly0 * (lx0 * p[y0][x0][c] + lx1 * p[y0][x1][c]) + ly1 * (lx0 * p[y1][x0][c] + lx1 * p[y1][x1][c])

numpy's float32 arrays round every operation on its own, so `resize` has the kernel's bits; `resize64` blends in fp64 from the SAME fp32
indices and weights (what the nine roundings of the blend cost, and nothing else).  Seeded frames and the byte buffer that puts frames
at odd addresses are here too, shared by the host and the GPU tests."""
import numpy as np

F32 = np.float32


def taps(src, dst):
    """per output index 0..dst-1: (i0, i1, l0, l1) - int64 indices, float32 weights"""
    scale = F32(src) / F32(dst)
    d = np.arange(dst, dtype=F32)
    centre = d + F32(0.5)
    scaled = scale * centre
    f = np.maximum(scaled - F32(0.5), F32(0))
    assert f.dtype == F32 and scaled.dtype == F32
    i0 = np.minimum(f.astype(np.int64), src - 1)
    i1 = np.minimum(i0 + 1, src - 1)
    l1 = f - i0.astype(F32)
    l0 = F32(1) - l1
    assert l0.dtype == F32 and l1.dtype == F32
    return i0, i1, l0, l1


def _blend(frame, in_h, in_w, dt):
    h, w = frame.shape[:2]
    y0, y1, ly0, ly1 = taps(h, in_h)
    x0, x1, lx0, lx1 = taps(w, in_w)
    p = frame.astype(dt)                                                 # [h][w][3]
    ly0, ly1 = ly0.astype(dt)[:, None, None], ly1.astype(dt)[:, None, None]
    lx0, lx1 = lx0.astype(dt)[None, :, None], lx1.astype(dt)[None, :, None]
    top = lx0 * p[y0][:, x0] + lx1 * p[y0][:, x1]
    bot = lx0 * p[y1][:, x0] + lx1 * p[y1][:, x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == dt
    return np.ascontiguousarray(out.transpose(2, 0, 1))                   # [3][in_h][in_w]


def resize(frame, in_h, in_w):
    """uint8 [h][w][3] -> float32 [3][in_h][in_w], the kernel's bits"""
    return _blend(frame, in_h, in_w, np.float32)


def resize64(frame, in_h, in_w):
    """the same blend in fp64 from the same fp32 indices and weights"""
    return _blend(frame, in_h, in_w, np.float64)


def batch(frames, in_h, in_w):
    """float32 [n][3][in_h][in_w]: what rtd_yolox_net_run must be given to compute what rtd_yolox_net_run_frames computes from `frames`"""
    return np.stack([resize(f, in_h, in_w) for f in frames])


def seeded_frame(seed, h, w):
    """uint8 [h][w][3]: smooth gradients under full-range noise, with the extremes 0 and 255 present"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.stack([xx * 3 + yy, xx + yy * 5, xx * 2 + yy * 2], 2) % 256).astype(np.int64)
    f = np.where(rng.random((h, w, 3)) < 0.5, base, rng.integers(0, 256, (h, w, 3))).astype(np.uint8)
    f.reshape(-1)[0] = 255
    f.reshape(-1)[-1] = 0
    return f


def carve(frames, offsets=(1, 2, 3), fill=0xA5):
    """One uint8 buffer that holds the frames back to back with gaps, frame i starting at an offset that is offsets[i % len] mod 4:
    (buffer, [start of frame i]).  The gaps keep `fill`."""
    pos, starts = 0, []
    for i, f in enumerate(frames):
        pos += 16
        pos += (offsets[i % len(offsets)] - pos) % 4
        starts.append(pos)
        pos += f.size
    buf = np.full(pos + 16, fill, np.uint8)
    for f, s in zip(frames, starts):
        buf[s:s + f.size] = f.reshape(-1)
    return buf, starts
