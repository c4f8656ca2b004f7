"""Numpy restatement of the reference's `ImageEnhancer.enhance_clahe_bilateral` (src/image_enhancement.py, method "clahe") for
3-channel 8-bit crops: cv2.cvtColor(BGR2LAB) -> CLAHE(clipLimit, tileGridSize) on L -> cv2.cvtColor(LAB2BGR) ->
cv2.bilateralFilter(d, sigmaColor, sigmaSpace).  cv2 is not a dependency of this project; the device path (csrc/enhance.hip) must
match this module bit for bit, stage by stage.  Every transcendental function is evaluated once, in double precision, into a table;
per pixel everything is integer arithmetic or a table lookup, except the CLAHE interpolation and the bilateral sums, which are float32
with the operation order written below and no contraction.

DESCALE(v, n) = (v + 2^(n-1)) >> n.   reflect(i, n) = BORDER_REFLECT_101: p = 2 (n - 1); i = i mod p; i >= n -> p - i.

(a) BGR -> Lab, 8 bit, sRGB gamma, D65 (OpenCV's integer path RGB2Lab_b; gamma_shift 3, lab_shift 12, lab_shift2 15):
    gtab[i] = sat_u16(rint(255 * 8 * g(i / 255))), i < 256, g(x) = x <= 0.04045 ? x / 12.92 : ((x + 0.055) / 1.055)^2.4
    ctab[i] = sat_u16(rint(2^15 * (x < 0.008856 ? 7.787 x + 0.13793103448275862 : cbrt(x)))), x = i / (255 * 8), i < 3072
    C[r][c] = rint(4096 * M[r][c] / white[r]), M = sRGB -> XYZ, white = D65 (every row of C sums to 4096)
    R', G', B' = gtab[r], gtab[g], gtab[b]
    fX = ctab[DESCALE(R' C00 + G' C01 + B' C02, 12)], fY and fZ alike from rows 1 and 2
    L = DESCALE(296 fY - (16 * 255 * 2^15 + 50) / 100, 15)          (integer division)
    a = DESCALE(500 (fX - fY) + 128 * 2^15, 15);  b = DESCALE(200 (fY - fZ) + 128 * 2^15, 15);  each clamped to 0..255

(b) CLAHE on L (OpenCV's clahe.cpp, 8 bit, 256 bins).  If w % tilesX == 0 and h % tilesY == 0 the tiles cover the crop; otherwise the
    crop is extended by tilesX - w % tilesX columns on the right and tilesY - h % tilesY rows at the bottom (BOTH, whenever either
    fails: a side that divides gets a whole `tiles` of padding) with reflect().  tile = extended size / grid.  Per tile:
    the histogram of the extended image's tile; if clipLimit > 0: clip = max((int)(clipLimit * area / 256), 1) (double), clipped =
    sum of the excess over clip, every bin capped at clip, every bin += clipped / 256, residual = clipped % 256 and, if non-zero,
    step = max(256 / residual, 1); for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++.
    lut[i] = sat_u8(rint((float) cumsum[i] * lutScale)), lutScale = 255.0f / area in float32, rint = half to even.
    Per pixel (x, y) of the crop, float32:  txf = x * (1.0f / tileW) - 0.5f; tx1 = floor(txf); tx2 = tx1 + 1; xa = txf - tx1;
    xa1 = 1 - xa; then tx1 = max(tx1, 0), tx2 = min(tx2, tilesX - 1); alike in y;
    res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 + (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya
    L' = sat_u8(rint(res)).

(c) Lab -> BGR, 8 bit: this project's own table-driven integer design (Q = 12, S = 255 * 64):
    fy = T_L[L] = rint(2^12 (L * 100 / 255 + 16) / 116); fx = fy + T_a[a], T_a[a] = rint(2^12 (a - 128) / 500);
    fz = fy - T_b[b], T_b[b] = rint(2^12 (b - 128) / 200)
    X, Y, Z = F[fx - fmin], F[fy - fmin], F[fz - fmin];  F[k] = rint(S * finv((fmin + k) / 2^12)) over the reachable range
    [fmin, fmax] (8754 entries), finv(t) = t > 6/29 ? t^3 : (t - 16/116) / 7.787
    channel = gi[clamp(DESCALE(Ci[r][0] X + Ci[r][1] Y + Ci[r][2] Z, 12), 0, S)], Ci = rint(2^12 * inverse(M) * white[column]),
    gi[v] = sat_u8(rint(255 * igamma(v / S))), v <= S (16321 entries), igamma(x) = x <= 0.0031308 ? 12.92 x : 1.055 x^(1/2.4) - 0.055

(d) Bilateral filter on the BGR image of (c): radius = d / 2 for d > 0, else rint(1.5 sigma_space); at least 1; sigmas <= 0 become 1.
    Taps: the offsets (i, j) with i^2 + j^2 <= radius^2 in raster order, i (rows) outer (49 for d = 9);
    space_w = (float) exp((i^2 + j^2) * (-0.5 / sigma_space^2)); color_w[k] = (float) exp(k^2 * (-0.5 / sigma_color^2)), k = 0..768.
    Per pixel, float32, taps in that order with the centre in its place, border = reflect() of the CROP:
    w = space_w[t] * color_w[|db| + |dg| + |dr|]; sum_c = sum_c + c * w per channel; wsum = wsum + w (all from 0);
    inv = 1.0f / wsum (correctly rounded); out_c = sat_u8(rint(sum_c * inv)).

`enhance` and its stage functions run this vectorised; the `scalar_*` functions are literal per-pixel transcriptions (tiny crops only)
that check them.

Points restated from memory of OpenCV that could not be checked against cv2 here (it is not installed and no OpenCV source is on
this machine; where cv2 is importable tests/test_enhance_host.py compares):
1. That the integer forward path (RGB2Lab_b with the constants above), not an IPP or OpenCL one, runs on the deployment host; and the
   table construction (gamma table from doubles rather than floats, the rounding of C).
2. OpenCV's own Lab -> BGR fixed-point tables: (c) is this project's design and can differ from them by a code value or so.
3. CLAHE: the padding rule, the (int) truncation of the clip limit in double, the residual loop, float32 lutScale and the
   interpolation order; that tileGridSize is (tilesX, tilesY).
4. Whether the bilateral scalar path handles the centre tap separately, and its summation order in the SIMD build (lanes of partial
   sums would change the float32 order).
5. sum * (1 / wsum) against sum / wsum, and that the space weight is computed from the integer i^2 + j^2 rather than sqrt() squared.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

F32 = np.float32
GAMMA_SHIFT, LAB_SHIFT, LAB_SHIFT2 = 3, 12, 15
M_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
WHITE = np.array([0.950456, 1.0, 1.088754])
Q, S = 12, 255 * 64
MIN_SIDE, MAX_TILES, MAX_RADIUS, MAX_CROPS = 16, 16, 7, 64      # the limits of include/rtdetr_mi355.h


def descale(v, n):
    return (v + (1 << (n - 1))) >> n


def reflect(i, n):
    """BORDER_REFLECT_101 for any integer (array) i"""
    if n == 1:
        return i * 0
    p = 2 * (n - 1)
    i = i % p
    return np.where(i >= n, p - i, i) if isinstance(i, np.ndarray) else (p - i if i >= n else i)


def _gamma(x: float) -> float:
    return x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4)


def _igamma(x: float) -> float:
    return x * 12.92 if x <= 0.0031308 else 1.055 * math.pow(x, 1 / 2.4) - 0.055


def _finv(t: float) -> float:
    return t * t * t if t > 6 / 29 else (t - 16 / 116) / 7.787


def _rint(x: float) -> int:
    return int(np.rint(x))


@lru_cache(maxsize=None)
def tables() -> Dict[str, np.ndarray]:
    """every table of (a) and (c), int64"""
    gtab = np.array([min(max(_rint(255.0 * 8 * _gamma(i / 255.0)), 0), 65535) for i in range(256)], np.int64)
    x = np.arange(3072) / float(255 * 8)
    ctab = np.clip(np.rint((1 << LAB_SHIFT2) * np.where(x < 0.008856, x * 7.787 + 0.13793103448275862, np.cbrt(x))), 0, 65535).astype(np.int64)
    C = np.rint((1 << LAB_SHIFT) * M_XYZ / WHITE[:, None]).astype(np.int64)
    t_l = np.array([_rint((1 << Q) * ((i * 100 / 255.0 + 16) / 116)) for i in range(256)], np.int64)
    t_a = np.array([_rint((1 << Q) * (i - 128) / 500.0) for i in range(256)], np.int64)
    t_b = np.array([_rint((1 << Q) * (i - 128) / 200.0) for i in range(256)], np.int64)
    fmin = int(min(t_l.min() + t_a.min(), t_l.min() - t_b.max()))
    fmax = int(max(t_l.max() + t_a.max(), t_l.max() - t_b.min()))
    finv = np.array([_rint(S * _finv(k / float(1 << Q))) for k in range(fmin, fmax + 1)], np.int64)
    Ci = np.rint((1 << Q) * np.linalg.inv(M_XYZ) * WHITE[None, :]).astype(np.int64)
    gi = np.array([min(max(_rint(255 * _igamma(v / float(S))), 0), 255) for v in range(S + 1)], np.int64)
    return {"gtab": gtab, "ctab": ctab, "C": C, "t_l": t_l, "t_a": t_a, "t_b": t_b, "fmin": np.int64(fmin), "finv": finv, "Ci": Ci, "gi": gi}


L_SCALE = (116 * 255 + 50) // 100
L_SHIFT = -((16 * 255 * (1 << LAB_SHIFT2) + 50) // 100)


# ---------------------------------------------------------------------------------------------------------------------- (a), (c)
def bgr_to_lab(bgr: np.ndarray) -> np.ndarray:
    """[..., 3] uint8 BGR -> [..., 3] uint8 Lab"""
    t = tables()
    v = np.asarray(bgr).astype(np.int64)
    B, G, R = t["gtab"][v[..., 0]], t["gtab"][v[..., 1]], t["gtab"][v[..., 2]]
    C = t["C"]
    fX, fY, fZ = (t["ctab"][descale(R * C[r, 0] + G * C[r, 1] + B * C[r, 2], LAB_SHIFT)] for r in range(3))
    L = descale(L_SCALE * fY + L_SHIFT, LAB_SHIFT2)
    a = descale(500 * (fX - fY) + 128 * (1 << LAB_SHIFT2), LAB_SHIFT2)
    b = descale(200 * (fY - fZ) + 128 * (1 << LAB_SHIFT2), LAB_SHIFT2)
    return np.clip(np.stack([L, a, b], -1), 0, 255).astype(np.uint8)


def lab_to_bgr(lab: np.ndarray) -> np.ndarray:
    """[..., 3] uint8 Lab -> [..., 3] uint8 BGR"""
    t = tables()
    v = np.asarray(lab).astype(np.int64)
    fy = t["t_l"][v[..., 0]]
    fx = fy + t["t_a"][v[..., 1]]
    fz = fy - t["t_b"][v[..., 2]]
    X, Y, Z = t["finv"][fx - t["fmin"]], t["finv"][fy - t["fmin"]], t["finv"][fz - t["fmin"]]
    Ci = t["Ci"]
    out = [t["gi"][np.clip(descale(Ci[r, 0] * X + Ci[r, 1] * Y + Ci[r, 2] * Z, Q), 0, S)] for r in (2, 1, 0)]
    return np.stack(out, -1).astype(np.uint8)


def lab_fp64(bgr: np.ndarray) -> np.ndarray:
    """the definition in double, unrounded: 8-bit scaled (L * 255 / 100, a + 128, b + 128)"""
    g = lambda x: np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    f = lambda t: np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16 / 116)
    rgb = g(np.asarray(bgr, np.float64)[..., ::-1] / 255.0)
    xyz = rgb @ M_XYZ.T / WHITE
    fx, fy, fz = f(xyz[..., 0]), f(xyz[..., 1]), f(xyz[..., 2])
    Y = xyz[..., 1]
    L = np.where(Y > 0.008856, 116 * fy - 16, 903.3 * Y)
    return np.stack([L * 255 / 100, 500 * (fx - fy) + 128, 200 * (fy - fz) + 128], -1)


def bgr_fp64(lab: np.ndarray) -> np.ndarray:
    """the inverse definition in double, unrounded, from 8-bit scaled Lab"""
    lab = np.asarray(lab, np.float64)
    L, a, b = lab[..., 0] * 100 / 255.0, lab[..., 1] - 128.0, lab[..., 2] - 128.0
    fy = (L + 16) / 116
    hi = L > 903.3 * 0.008856
    Y = np.where(hi, fy ** 3, L / 903.3)
    fy = np.where(hi, fy, 7.787 * Y + 16 / 116)
    fx, fz = fy + a / 500, fy - b / 200
    fi = lambda t: np.where(t > 6 / 29, t ** 3, (t - 16 / 116) / 7.787)
    xyz = np.stack([fi(fx) * WHITE[0], Y, fi(fz) * WHITE[2]], -1)
    rgb = np.clip(xyz @ np.linalg.inv(M_XYZ).T, 0, 1)
    rgb = np.where(rgb <= 0.0031308, rgb * 12.92, 1.055 * rgb ** (1 / 2.4) - 0.055)
    return (rgb * 255)[..., ::-1]


# ---------------------------------------------------------------------------------------------------------------------- (b)
def clahe_geometry(h: int, w: int, tiles_x: int, tiles_y: int) -> Tuple[int, int, int, int]:
    """(extended h, extended w, tile h, tile w)"""
    if w % tiles_x == 0 and h % tiles_y == 0:
        eh, ew = h, w
    else:
        eh, ew = h + tiles_y - h % tiles_y, w + tiles_x - w % tiles_x
    return eh, ew, eh // tiles_y, ew // tiles_x


def clip_of(clip_limit: float, area: int) -> int:
    """the integer clip of a tile; 0 = no clipping"""
    return max(int(float(clip_limit) * area / 256), 1) if clip_limit > 0 else 0


def lut_of_hist(hist: np.ndarray, clip: int, area: int) -> np.ndarray:
    """[..., 256] int histograms -> [..., 256] uint8 LUTs"""
    hist = hist.astype(np.int64)
    if clip > 0:
        clipped = np.maximum(hist - clip, 0).sum(-1, keepdims=True)
        hist = np.minimum(hist, clip) + clipped // 256
        residual = clipped % 256
        step = np.maximum(256 // np.maximum(residual, 1), 1)
        i = np.arange(256)
        hist = hist + ((i % step == 0) & (i // step < residual))
    scale = F32(255.0) / F32(area)
    return np.clip(np.rint(np.cumsum(hist, -1).astype(F32) * scale), 0, 255).astype(np.uint8)


def clahe_luts(L: np.ndarray, clip_limit: float, tiles_x: int, tiles_y: int) -> np.ndarray:
    """[h, w] uint8 -> [tiles_y, tiles_x, 256] uint8"""
    h, w = L.shape
    eh, ew, th, tw = clahe_geometry(h, w, tiles_x, tiles_y)
    ext = L[reflect(np.arange(eh), h)][:, reflect(np.arange(ew), w)]
    tiles = ext.reshape(tiles_y, th, tiles_x, tw).transpose(0, 2, 1, 3).reshape(tiles_y * tiles_x, th * tw)
    hist = np.stack([np.bincount(t, minlength=256) for t in tiles]).reshape(tiles_y, tiles_x, 256)
    return lut_of_hist(hist, clip_of(clip_limit, th * tw), th * tw)


def _interp_axis(n: int, tile: int, tiles: int):
    f = np.arange(n).astype(F32) * (F32(1.0) / F32(tile)) - F32(0.5)
    t1 = np.floor(f).astype(np.int64)
    a = f - t1.astype(F32)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, F32(1.0) - a


def clahe_apply(L: np.ndarray, luts: np.ndarray) -> np.ndarray:
    h, w = L.shape
    tiles_y, tiles_x = luts.shape[:2]
    _, _, th, tw = clahe_geometry(h, w, tiles_x, tiles_y)
    tx1, tx2, xa, xa1 = _interp_axis(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = _interp_axis(h, th, tiles_y)
    v = L.astype(np.int64)
    lf = luts.astype(F32)
    g = lambda ty, tx: lf[ty[:, None], tx[None, :], v]
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (g(ty1, tx1) * xa1 + g(ty1, tx2) * xa) * ya1 + (g(ty2, tx1) * xa1 + g(ty2, tx2) * xa) * ya
    assert res.dtype == F32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe(L: np.ndarray, clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8) -> np.ndarray:
    return clahe_apply(L, clahe_luts(L, clip_limit, tiles_x, tiles_y))


# ---------------------------------------------------------------------------------------------------------------------- (d)
def bilateral_radius(d: int, sigma_space: float) -> int:
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    return max(d // 2 if d > 0 else int(np.rint(ss * 1.5)), 1)


@lru_cache(maxsize=None)
def bilateral_weights(d: int, sigma_color: float, sigma_space: float):
    """(radius, [(i, j)] taps in raster order, space_w float32 [taps], color_w float32 [769])"""
    sc = float(sigma_color) if sigma_color > 0 else 1.0
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    r = bilateral_radius(d, sigma_space)
    gc, gs = -0.5 / (sc * sc), -0.5 / (ss * ss)
    taps = [(i, j) for i in range(-r, r + 1) for j in range(-r, r + 1) if i * i + j * j <= r * r]
    space_w = np.array([math.exp((i * i + j * j) * gs) for i, j in taps], np.float64).astype(F32)
    color_w = np.array([math.exp(k * k * gc) for k in range(769)], np.float64).astype(F32)
    return r, taps, space_w, color_w


def bilateral(img: np.ndarray, d: int = 9, sigma_color: float = 75, sigma_space: float = 75) -> np.ndarray:
    r, taps, space_w, color_w = bilateral_weights(int(d), float(sigma_color), float(sigma_space))
    h, w, _ = img.shape
    ys, xs = reflect(np.arange(-r, h + r), h), reflect(np.arange(-r, w + r), w)
    pad = img[ys][:, xs].astype(np.int64)
    c0 = img.astype(np.int64)
    acc = np.zeros((h, w, 3), F32)
    wsum = np.zeros((h, w), F32)
    for (i, j), sw in zip(taps, space_w):
        nb = pad[r + i:r + i + h, r + j:r + j + w]
        wt = sw * color_w[np.abs(nb - c0).sum(-1)]
        acc = acc + nb.astype(F32) * wt[..., None]
        wsum = wsum + wt
    inv = F32(1.0) / wsum
    assert acc.dtype == F32 and inv.dtype == F32
    return np.clip(np.rint(acc * inv[..., None]), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------- whole
def stages(bgr: np.ndarray, clip_limit: float = 2.0, tile_grid_size=(8, 8), bilateral_d: int = 9, sigma_color: float = 75,
           sigma_space: float = 75) -> Dict[str, np.ndarray]:
    """every stage of one crop: lab [h, w, 3], luts [ty, tx, 256], bgr (before the bilateral filter), out"""
    bgr = np.ascontiguousarray(bgr, np.uint8)
    assert bgr.ndim == 3 and bgr.shape[2] == 3
    tiles_x, tiles_y = int(tile_grid_size[0]), int(tile_grid_size[1])
    lab = bgr_to_lab(bgr)
    luts = clahe_luts(lab[..., 0], clip_limit, tiles_x, tiles_y)
    lab2 = lab.copy()
    lab2[..., 0] = clahe_apply(lab[..., 0], luts)
    mid = lab_to_bgr(lab2)
    return {"lab": lab, "luts": luts, "bgr": mid, "out": bilateral(mid, bilateral_d, sigma_color, sigma_space)}


def enhance(bgr: np.ndarray, **params) -> np.ndarray:
    return stages(bgr, **params)["out"]


# ---------------------------------------------------------------------------------------------------------------------- scalar
def scalar_lab(px) -> Tuple[int, int, int]:
    t = tables()
    B, G, R = (int(t["gtab"][int(c)]) for c in px)
    f = []
    for r in range(3):
        C = [int(c) for c in t["C"][r]]
        f.append(int(t["ctab"][(R * C[0] + G * C[1] + B * C[2] + (1 << 11)) >> 12]))
    fX, fY, fZ = f
    L = (296 * fY - (16 * 255 * 32768 + 50) // 100 + (1 << 14)) >> 15
    a = (500 * (fX - fY) + 128 * 32768 + (1 << 14)) >> 15
    b = (200 * (fY - fZ) + 128 * 32768 + (1 << 14)) >> 15
    return tuple(min(max(v, 0), 255) for v in (L, a, b))


def scalar_bgr(lab) -> Tuple[int, int, int]:
    t = tables()
    fy = int(t["t_l"][int(lab[0])])
    fx, fz = fy + int(t["t_a"][int(lab[1])]), fy - int(t["t_b"][int(lab[2])])
    fmin = int(t["fmin"])
    X, Y, Z = (int(t["finv"][k - fmin]) for k in (fx, fy, fz))
    out = []
    for r in (2, 1, 0):
        Ci = [int(c) for c in t["Ci"][r]]
        v = (Ci[0] * X + Ci[1] * Y + Ci[2] * Z + (1 << 11)) >> 12
        out.append(int(t["gi"][min(max(v, 0), S)]))
    return tuple(out)


def scalar_enhance(bgr: np.ndarray, clip_limit: float = 2.0, tile_grid_size=(8, 8), bilateral_d: int = 9, sigma_color: float = 75,
                   sigma_space: float = 75) -> Dict[str, np.ndarray]:
    """the same stages, one pixel at a time with Python integers and numpy float32 scalars (tiny crops only)"""
    h, w, _ = bgr.shape
    tiles_x, tiles_y = int(tile_grid_size[0]), int(tile_grid_size[1])
    lab = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            lab[y, x] = scalar_lab(bgr[y, x])
    # ---- (b)
    if w % tiles_x == 0 and h % tiles_y == 0:
        eh, ew = h, w
    else:
        eh, ew = h + (tiles_y - h % tiles_y), w + (tiles_x - w % tiles_x)
    th, tw = eh // tiles_y, ew // tiles_x
    area = th * tw
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    lut_scale = F32(255.0) / F32(area)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hist = [0] * 256
            for ey in range(ty * th, (ty + 1) * th):
                for ex in range(tx * tw, (tx + 1) * tw):
                    hist[int(lab[reflect(ey, h), reflect(ex, w), 0])] += 1
            if clip_limit > 0:
                clip = max(int(float(clip_limit) * area / 256), 1)
                clipped = 0
                for i in range(256):
                    if hist[i] > clip:
                        clipped += hist[i] - clip
                        hist[i] = clip
                batch, residual = clipped // 256, clipped % 256
                for i in range(256):
                    hist[i] += batch
                if residual != 0:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:
                        hist[i] += 1
                        i += step
                        residual -= 1
            s = 0
            for i in range(256):
                s += hist[i]
                luts[ty, tx, i] = min(max(int(np.rint(F32(s) * lut_scale)), 0), 255)
    lab2 = lab.copy()
    inv_tw, inv_th = F32(1.0) / F32(tw), F32(1.0) / F32(th)
    for y in range(h):
        tyf = F32(y) * inv_th - F32(0.5)
        ty1 = int(np.floor(tyf))
        ya = tyf - F32(ty1)
        ya1 = F32(1.0) - ya
        ty1c, ty2c = max(ty1, 0), min(ty1 + 1, tiles_y - 1)
        for x in range(w):
            txf = F32(x) * inv_tw - F32(0.5)
            tx1 = int(np.floor(txf))
            xa = txf - F32(tx1)
            xa1 = F32(1.0) - xa
            tx1c, tx2c = max(tx1, 0), min(tx1 + 1, tiles_x - 1)
            v = int(lab[y, x, 0])
            p = lambda a, b: F32(luts[a, b, v])
            res = (p(ty1c, tx1c) * xa1 + p(ty1c, tx2c) * xa) * ya1 + (p(ty2c, tx1c) * xa1 + p(ty2c, tx2c) * xa) * ya
            lab2[y, x, 0] = min(max(int(np.rint(res)), 0), 255)
    mid = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            mid[y, x] = scalar_bgr(lab2[y, x])
    # ---- (d)
    r, taps, space_w, color_w = bilateral_weights(int(bilateral_d), float(sigma_color), float(sigma_space))
    out = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            b0, g0, r0 = (int(c) for c in mid[y, x])
            sb = sg = sr = ws = F32(0.0)
            for t, (i, j) in enumerate(taps):
                b, g, rr = (int(c) for c in mid[reflect(y + i, h), reflect(x + j, w)])
                wt = space_w[t] * color_w[abs(b - b0) + abs(g - g0) + abs(rr - r0)]
                sb = sb + F32(b) * wt
                sg = sg + F32(g) * wt
                sr = sr + F32(rr) * wt
                ws = ws + wt
            inv = F32(1.0) / ws
            out[y, x] = [min(max(int(np.rint(s * inv)), 0), 255) for s in (sb, sg, sr)]
    return {"lab": lab, "luts": luts, "bgr": mid, "out": out}


# ---------------------------------------------------------------------------------------------------------------------- test crops
def content(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """the test contents: seeded noise, a smooth ramp with flat bands (heavy clipping with a residual), all zero, all 255"""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "zero":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "full":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        g = (x * 255 // max(w - 1, 1) + y * 40 // max(h - 1, 1)) % 256
        g = np.where((x // 11) % 3 == 0, 90, g)                     # flat bands
        return np.stack([g, (g * 3 // 4 + 20) % 256, 255 - g], -1).astype(np.uint8)
    raise ValueError(kind)
