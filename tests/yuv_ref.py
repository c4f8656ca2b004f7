"""The restatement csrc/ingest.hip must equal bit for bit: OpenCV's COLOR_YUV2BGR_NV12 / _NV21 / _I420 fixed-point conversion, in numpy
integers, extended to odd sizes and to four matrix / range tables.

* the chroma plane has ceil(H/2) rows of ceil(W/2) samples; pixel (y, x) takes sample (y >> 1, x >> 1), no interpolation
* u = U - 128, v = V - 128, y' = max(Y - 16, 0) (limited range) or Y (full range), all sums in int32:
    B = clip8((y' CY + 2^19 + CUB u) >> 20)
    G = clip8((y' CY + 2^19 + CVG v + CUG u) >> 20)
    R = clip8((y' CY + 2^19 + CVR v) >> 20)
  with an arithmetic shift, and the constants floor(c 2^20 + 0.5) of the decimal coefficients below.

cv2 is not a dependency: where it is importable tests/test_ingest_host.py compares BT.601 limited on even sizes with cv2.cvtColor.
Also here: a seeded content generator that drives every channel into both clamps, packing of planes into the three layouts (tight or
with padded pitches), and `RefIngest`, a stand-in for ingest.FrameIngest that answers from this restatement with host tensors.
"""
import math

import numpy as np

LAYOUTS = ("nv12", "nv21", "i420")
MATRICES = ("bt601", "bt709")
# (matrix, full_range) -> decimal coefficients CY, CVR, CVG, CUG, CUB
COEFFS = {
    ("bt601", False): (1.164, 1.596, -0.813, -0.391, 2.018),     # OpenCV's own
    ("bt709", False): (1.164, 1.793, -0.533, -0.213, 2.112),
    ("bt601", True): (1.0, 1.402, -0.714, -0.344, 1.772),
    ("bt709", True): (1.0, 1.575, -0.468, -0.187, 1.856),
}
TABLES = tuple(COEFFS)
SHIFT = 20


def table(matrix="bt601", full_range=False):
    """THE constants of the restatement: floor(c 2^20 + 0.5), order CY, CVR, CVG, CUG, CUB"""
    return tuple(int(math.floor(c * (1 << SHIFT) + 0.5)) for c in COEFFS[(matrix, bool(full_range))])


def chroma_hw(h, w):
    return (h + 1) // 2, (w + 1) // 2


def frame_bytes(h, w):
    ch, cw = chroma_hw(h, w)
    return h * w + 2 * ch * cw


def planes_to_bgr(Y, U, V, matrix="bt601", full_range=False):
    """Y [H, W], U and V [ceil(H/2), ceil(W/2)] uint8 -> [H, W, 3] uint8 BGR"""
    H, W = Y.shape
    assert U.shape == V.shape == chroma_hw(H, W), (Y.shape, U.shape, V.shape)
    cy, cvr, cvg, cug, cub = table(matrix, full_range)
    y = Y.astype(np.int32)
    if not full_range:
        y = np.maximum(y - 16, 0)
    yc = y * np.int32(cy) + np.int32(1 << (SHIFT - 1))
    rows, cols = np.arange(H) >> 1, np.arange(W) >> 1
    u = (U.astype(np.int32) - 128)[rows][:, cols]
    v = (V.astype(np.int32) - 128)[rows][:, cols]
    b = (yc + np.int32(cub) * u) >> SHIFT                        # int32 throughout; >> on a signed numpy integer is arithmetic
    g = (yc + np.int32(cvg) * v + np.int32(cug) * u) >> SHIFT
    r = (yc + np.int32(cvr) * v) >> SHIFT
    assert b.dtype == g.dtype == r.dtype == np.int32
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def unclamped(Y, U, V, matrix="bt601", full_range=False):
    """the three channels before clip8 (int32 [H, W, 3], BGR order): what the content generator's own test looks at"""
    H, W = Y.shape
    cy, cvr, cvg, cug, cub = table(matrix, full_range)
    y = Y.astype(np.int64) if full_range else np.maximum(Y.astype(np.int64) - 16, 0)
    yc = y * cy + (1 << (SHIFT - 1))
    rows, cols = np.arange(H) >> 1, np.arange(W) >> 1
    u = (U.astype(np.int64) - 128)[rows][:, cols]
    v = (V.astype(np.int64) - 128)[rows][:, cols]
    out = np.stack([(yc + cub * u) >> SHIFT, (yc + cvg * v + cug * u) >> SHIFT, (yc + cvr * v) >> SHIFT], axis=-1)
    assert np.abs(out).max() < (1 << 31) >> SHIFT                # (the sums before the shift fit int32)
    return out


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def chroma_row_bytes(layout, w):
    cw = (w + 1) // 2
    return cw if layout == "i420" else 2 * cw


def pack(Y, U, V, layout="nv12", y_pitch=None, c_pitch=None, fill=0xFF):
    """planes -> (flat uint8 buffer, offsets (y, u, v), pitches (y, c)): tight by default (what ffmpeg's rawvideo writes), or with padded
    rows whose padding holds `fill`.  For nv12 / nv21 the u offset is the interleaved plane's and the v offset is None."""
    H, W = Y.shape
    ch, cw = U.shape
    crow = chroma_row_bytes(layout, W)
    yp = W if y_pitch is None else y_pitch
    cp = crow if c_pitch is None else c_pitch
    assert yp >= W and cp >= crow
    ybuf = np.full((H, yp), fill, np.uint8)
    ybuf[:, :W] = Y
    if layout == "i420":
        ubuf, vbuf = np.full((ch, cp), fill, np.uint8), np.full((ch, cp), fill, np.uint8)
        ubuf[:, :cw], vbuf[:, :cw] = U, V
        parts = [ybuf.reshape(-1), ubuf.reshape(-1), vbuf.reshape(-1)]
        offs = (0, ybuf.size, ybuf.size + ubuf.size)
    else:
        first, second = (U, V) if layout == "nv12" else (V, U)
        cbuf = np.full((ch, cp), fill, np.uint8)
        cbuf[:, 0:2 * cw:2], cbuf[:, 1:2 * cw:2] = first, second
        parts = [ybuf.reshape(-1), cbuf.reshape(-1)]
        offs = (0, ybuf.size, None)
    return np.ascontiguousarray(np.concatenate(parts)), offs, (yp, cp)


def unpack(buf, h, w, layout="nv12"):
    """a tightly packed frame -> (Y, U, V)"""
    buf = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.asarray(buf, np.uint8).reshape(-1)
    ch, cw = chroma_hw(h, w)
    assert buf.size == frame_bytes(h, w), (buf.size, h, w)
    Y = buf[:h * w].reshape(h, w)
    c = buf[h * w:]
    if layout == "i420":
        return Y, c[:ch * cw].reshape(ch, cw), c[ch * cw:].reshape(ch, cw)
    pairs = c.reshape(ch, cw, 2)
    a, b = pairs[..., 0], pairs[..., 1]
    return (Y, a, b) if layout == "nv12" else (Y, b, a)


def to_bgr(buf, h, w, layout="nv12", matrix="bt601", full_range=False):
    """a tightly packed frame -> [h, w, 3] uint8 BGR"""
    return planes_to_bgr(*unpack(buf, h, w, layout), matrix=matrix, full_range=full_range)


# ---- content ----------------------------------------------------------------------------------------------------------------------------
# (Y, U, V) triples that drive a channel past a clamp under all four tables: bright with extreme chroma overflows, dark underflows
_EXTREMES = [(255, 255, 128), (255, 128, 255), (255, 0, 0), (235, 255, 255),      # B, R, G (both chroma low), B and R above 255
             (0, 0, 128), (0, 128, 0), (16, 255, 255), (30, 0, 255), (30, 255, 0)]   # B, R, G below 0 in turn


def planes(seed, h, w):
    """seeded content (Y, U, V): uniform noise over the whole byte range (limited-range streams do carry values outside 16..235), with
    the extreme triples above written over whole 2 x 2 blocks where there is room, so that every channel meets both clamps and no two
    of the four tables give the same picture."""
    rng = np.random.default_rng(seed)
    ch, cw = chroma_hw(h, w)
    Y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    U = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    V = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    blocks = ch * cw
    where = rng.permutation(blocks)[:min(blocks, len(_EXTREMES))]
    for k, idx in enumerate(where):
        by, bx = divmod(int(idx), cw)
        y, u, v = _EXTREMES[k]
        Y[2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = y
        U[by, bx], V[by, bx] = u, v
    return Y, U, V


def scene_planes(seed, h, w):
    """camera-like content: the package's synthetic scene (BGR), taken to Y, U, V by plain BT.601 limited-range arithmetic and averaged
    over 2 x 2 blocks: smooth areas and edges rather than noise (the chain test's frame)"""
    from telescope_cam_detection_amd.synth import scene_frame
    bgr = scene_frame(seed, h, w).astype(np.float64)
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    Y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    U = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    V = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    ch, cw = chroma_hw(h, w)

    def sub(p):
        q = np.pad(p, ((0, 2 * ch - h), (0, 2 * cw - w)), mode="edge")
        return q.reshape(ch, 2, cw, 2).mean(axis=(1, 3))
    to8 = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    return to8(Y), to8(sub(U)), to8(sub(V))


def frame(seed, h, w, layout="nv12"):
    """a tightly packed frame of planes(seed, h, w)"""
    return pack(*planes(seed, h, w), layout=layout)[0]


class RefIngest:
    """ingest.FrameIngest's to_bgr from the restatement, with host tensors (the capture class's `ingest` seam in CPU tests)"""

    def __init__(self):
        self.calls = 0

    def to_bgr(self, frames, sizes, layout="nv12", matrix="bt601", full_range=False, out=None):
        import torch
        self.calls += 1
        return [torch.from_numpy(to_bgr(f, h, w, layout, matrix, full_range)) for f, (h, w) in zip(frames, sizes)]
