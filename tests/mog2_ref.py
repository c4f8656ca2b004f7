"""Numpy restatement of the reference's motion filter (src/motion_filter.py MotionFilter.has_motion_in_bbox) on 8-bit frames, as
OpenCV 4.x computes it: cv2.createBackgroundSubtractorMOG2(history, varThreshold, detectShadows).apply(frame) on the CPU path
(bgfg_gaussmix2.cpp, MOG2Invoker; the 8-bit input is converted exactly to float32), threshold(mask, 200), GaussianBlur(k x k, 0),
threshold(25), countNonZero over the box.  cv2 is not a dependency of this project; the device filter (csrc/mog2.hip) must match this
bit for bit, and the tests compare the whole model after every call, the foreground masks and the counts.

The model: 5 modes per pixel kept sorted by weight (weight, variance, C means), the modes-used count, and nframes.  Defaults of
createBackgroundSubtractorMOG2: backgroundRatio TB = 0.9f, varThresholdGen Tg = 9f, varInit 15, varMin 4, varMax 75,
fCT = 0.05f, shadow tau = 0.5f, shadow value 127.  All zeros on the first apply and on a change of frame size or type.

Per apply: ++nframes; lr = 1.0 / min(2 nframes, history) in double; alphaT = (float) lr, alpha1 = 1 - alphaT,
prune = (float)(-lr * fCT), Tb = (float) varThreshold.  Per pixel (float32, each expression evaluated left to right, no contraction):

    background = fits = false; total = 0; n = modes_used
    for m = 0; m < n; m++:                                        # n shrinks inside the loop
        w = alpha1 * W[m] + prune; swaps = 0
        if !fits:
            d_c = mean[m][c] - x_c; dist2 = d_0 * d_0 + d_1 * d_1 + d_2 * d_2    (C = 1: 0 + d_0 * d_0)
            if total < TB and dist2 < Tb * var[m]: background = true
            if dist2 < Tg * var[m]:
                fits = true; w = w + alphaT; k = alphaT / w
                mean[m][c] = mean[m][c] - k * d_c; var[m] = min(max(var[m] + k * (dist2 - var[m]), 4), 75)
                for i = m .. 1: if w < W[i - 1]: break; swap modes i, i - 1; swaps++
        if w < -prune: w = 0; n--
        W[m - swaps] = w; total = total + w
    inv = |total| > FLT_EPSILON ? 1 / total : 0;  W[0 .. n) *= inv
    if !fits and alphaT > 0:
        m = n == 5 ? 4 : n++
        if n == 1: W[m] = 1  else: W[m] = alphaT; W[0 .. n - 1) *= alpha1
        mean[m] = x; var[m] = 15
        for i = n - 1 .. 1: if alphaT < W[i - 1]: break; swap modes i, i - 1
    modes_used = n
    mask = background ? 0 : (shadows and shadow(x) ? 127 : 255)
    shadow(x), on the updated model, tw = 0: for m < n: num = sum_c x_c mean_c, den = sum_c mean_c^2 (each from 0, in channel order);
        den == 0 -> false; if num <= den and num >= tau * den: a = num / den;
        if sum_c (a mean_c - x_c)^2 < Tb * var * a * a -> true;  tw = tw + W[m]; if tw > TB -> false

`Mog2` runs this vectorised over pixels (loops over modes and sorting steps, exactly the predicated form the kernel uses);
`Mog2Scalar` is a literal per-pixel transcription of the C++ loop (tiny frames only) that checks it.

Points restated from memory of bgfg_gaussmix2.cpp that could not be checked against cv2 here (it is not installed; where it is,
tests/test_mog2_host.py compares):
1. The in-loop `n--` on a pruned mode shortens the mode loop (the last mode is dropped, the pruned one keeps its slot with weight 0).
2. The FLT_EPSILON guard of the renormalisation (older releases divided by the total unconditionally).
3. The shadow test runs after the update, on the updated and re-sorted model with the new modes-used count.
4. The operator order of every expression above, including that dist2 of 3 channels does not start from 0 and the variance clamp is
   MAX then MIN; and that the CPU path, not an OpenCL or IPP one, runs on the deployment host.
5. That the learning rate is 1 / min(2 nframes, history) with the default learningRate = -1 also on the first frame, and prune uses
   fCT promoted from float to double.
The mask blur is tests/motion_ref.py's bit-exact 8-bit GaussianBlur; its own unchecked points are listed there.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import motion_ref

F32 = np.float32
NM = 5
TB, TG = F32(0.9), F32(9.0)
VAR_INIT, VAR_MIN, VAR_MAX = F32(15.0), F32(4.0), F32(75.0)
TAU, FCT = F32(0.5), F32(0.05)
FLT_EPSILON = F32(np.finfo(np.float32).eps)
SHADOW = 127
MASK_THRESHOLD = 25


def rates(nframes: int, history: int) -> Tuple[np.float32, np.float32, np.float32]:
    """(alphaT, alpha1, prune) of the update that makes the model's nframes-th frame"""
    lr = 1.0 / min(2 * nframes, history)
    alpha_t = F32(lr)
    return alpha_t, F32(1.0) - alpha_t, F32(-lr * float(FCT))


def as_hwc(frame) -> np.ndarray:
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise ValueError(f"frames must be uint8, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"frames must be HxW or HxWxC with C = 1 or 3, got shape {a.shape}")
    return a


class Mog2:
    """The background model, vectorised over pixels.  Arrays: W, V [5, P], M [5, C, P] float32, N [P] int, plus nframes."""

    def __init__(self, history: int = 500, var_threshold=16, detect_shadows: bool = True):
        self.history = int(history)
        self.tb = F32(var_threshold)
        self.shadows = bool(detect_shadows)
        self.shape: Optional[tuple] = None
        self.nframes = 0

    def _init(self, shape):
        H, W_, C = shape
        P = H * W_
        self.shape = shape
        self.W = np.zeros((NM, P), F32)
        self.V = np.zeros((NM, P), F32)
        self.M = np.zeros((NM, C, P), F32)
        self.N = np.zeros(P, np.int64)
        self.nframes = 0

    def _swap(self, sel, i, j):
        for arr in (self.W, self.V, self.M):
            a, b = arr[i].copy(), arr[j].copy()
            s = sel if arr.ndim == 2 else sel[None, :]
            arr[i] = np.where(s, b, a)
            arr[j] = np.where(s, a, b)

    def apply(self, frame) -> np.ndarray:
        """one update; the foreground mask (0 / 127 / 255) [H, W]"""
        f = as_hwc(frame)
        if self.shape != f.shape or self.nframes == 0:
            self._init(f.shape)
        H, W_, C = f.shape
        x = f.reshape(-1, C).T.astype(F32)                # [C, P]
        self.nframes += 1
        alpha_t, alpha1, prune = rates(self.nframes, self.history)
        tb = self.tb
        W, V, M = self.W, self.V, self.M
        n = self.N.copy()
        P = x.shape[1]
        background = np.zeros(P, bool)
        fits = np.zeros(P, bool)
        total = np.zeros(P, F32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for m in range(NM):
                act = m < n
                wm = alpha1 * W[m] + prune
                chk = act & ~fits
                d = M[m] - x
                dist2 = d[0] * d[0] if C == 3 else F32(0.0) + d[0] * d[0]
                for c in range(1, C):
                    dist2 = dist2 + d[c] * d[c]
                var = V[m].copy()
                background |= chk & (total < TB) & (dist2 < tb * var)
                fit = chk & (dist2 < TG * var)
                fits |= fit
                wm = np.where(fit, wm + alpha_t, wm)
                k = alpha_t / wm
                M[m] = np.where(fit[None, :], M[m] - k * d, M[m])
                vn = var + k * (dist2 - var)
                vn = np.where(vn < VAR_MIN, VAR_MIN, vn)
                vn = np.where(vn > VAR_MAX, VAR_MAX, vn)
                V[m] = np.where(fit, vn, var)
                wsort = wm
                pruned = act & (wm < -prune)
                wm = np.where(pruned, F32(0.0), wm)
                n = n - pruned
                W[m] = np.where(act, wm, W[m])
                go = fit.copy()
                for i in range(m, 0, -1):
                    go &= ~(wsort < W[i - 1])
                    self._swap(go, i, i - 1)
                total = np.where(act, total + wm, total)
            inv = np.where(np.abs(total) > FLT_EPSILON, F32(1.0) / total, F32(0.0))
            for m in range(NM):
                W[m] = np.where(m < n, W[m] * inv, W[m])
            new = ~fits if alpha_t > 0 else np.zeros(P, bool)
            mn = np.where(n == NM, NM - 1, n)
            n = np.where(new & (n < NM), n + 1, n)
            for m in range(NM):
                sel = new & (mn == m)
                W[m] = np.where(sel, np.where(n == 1, F32(1.0), alpha_t), W[m])
                V[m] = np.where(sel, VAR_INIT, V[m])
                M[m] = np.where(sel[None, :], x, M[m])
                W[m] = np.where(new & ~sel & (n != 1) & (m < n - 1), W[m] * alpha1, W[m])
            go = new.copy()
            for i in range(NM - 1, 0, -1):
                inside = i <= n - 1
                g2 = go & ~(alpha_t < W[i - 1])
                self._swap(new & inside & g2, i, i - 1)
                go = np.where(inside, g2, go)
            self.N = n
            sh = self._shadow(x, n) if self.shadows else np.zeros(P, bool)
        mask = np.where(background, 0, np.where(sh, SHADOW, 255)).astype(np.uint8)
        return mask.reshape(H, W_)

    def _shadow(self, x, n):
        W, V, M = self.W, self.V, self.M
        C, P = x.shape
        tw = np.zeros(P, F32)
        done = np.zeros(P, bool)
        res = np.zeros(P, bool)
        for m in range(NM):
            live = ~done & (m < n)
            num = np.zeros(P, F32)
            den = np.zeros(P, F32)
            for c in range(C):
                num = num + x[c] * M[m][c]
                den = den + M[m][c] * M[m][c]
            zero = live & (den == 0)
            done |= zero
            live &= ~zero
            cond = live & (num <= den) & (num >= TAU * den)
            a = num / den
            d2 = np.zeros(P, F32)
            for c in range(C):
                dd = a * M[m][c] - x[c]
                d2 = d2 + dd * dd
            hit = cond & (d2 < self.tb * V[m] * a * a)
            res |= hit
            done |= hit
            live &= ~hit
            tw = np.where(live, tw + W[m], tw)
            done |= live & (tw > TB)
        return res

    def model(self) -> Dict[str, np.ndarray]:
        """the canonical layout of rtd_debug_mog2_model"""
        H, W_, C = self.shape
        return {"weight": self.W.T.reshape(H, W_, NM), "variance": self.V.T.reshape(H, W_, NM),
                "mean": self.M.transpose(2, 0, 1).reshape(H, W_, NM, C), "modes_used": self.N.astype(np.uint8).reshape(H, W_),
                "nframes": self.nframes}


class Mog2Scalar:
    """A literal per-pixel transcription of MOG2Invoker's loop (dynamic mode indices, swap counts, early breaks): for tiny frames."""

    def __init__(self, history: int = 500, var_threshold=16, detect_shadows: bool = True):
        self.history = int(history)
        self.tb = F32(var_threshold)
        self.shadows = bool(detect_shadows)
        self.shape = None
        self.nframes = 0

    def apply(self, frame) -> np.ndarray:
        f = as_hwc(frame)
        if self.shape != f.shape or self.nframes == 0:
            H, W_, C = f.shape
            self.shape = f.shape
            self.w = [[F32(0)] * NM for _ in range(H * W_)]
            self.v = [[F32(0)] * NM for _ in range(H * W_)]
            self.mu = [[[F32(0)] * C for _ in range(NM)] for _ in range(H * W_)]
            self.n = [0] * (H * W_)
            self.nframes = 0
        H, W_, C = f.shape
        self.nframes += 1
        alpha_t, alpha1, prune = rates(self.nframes, self.history)
        mask = np.zeros(H * W_, np.uint8)
        for p, px in enumerate(f.reshape(-1, C)):
            mask[p] = self._pixel(p, [F32(v) for v in px], alpha_t, alpha1, prune)
        return mask.reshape(H, W_)

    def _pixel(self, p, x, alpha_t, alpha1, prune) -> int:
        gw, gv, mean = self.w[p], self.v[p], self.mu[p]
        C = len(x)
        tb = self.tb

        def swap(i, j):
            gw[i], gw[j] = gw[j], gw[i]
            gv[i], gv[j] = gv[j], gv[i]
            mean[i], mean[j] = mean[j], mean[i]

        background = fits = False
        nmodes = self.n[p]
        total = F32(0)
        mode = 0
        while mode < nmodes:
            weight = alpha1 * gw[mode] + prune
            swap_count = 0
            if not fits:
                var = gv[mode]
                dd = [mean[mode][c] - x[c] for c in range(C)]
                if C == 3:
                    dist2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]
                else:
                    dist2 = F32(0)
                    for c in range(C):
                        dist2 = dist2 + dd[c] * dd[c]
                if total < TB and dist2 < tb * var:
                    background = True
                if dist2 < TG * var:
                    fits = True
                    weight = weight + alpha_t
                    k = alpha_t / weight
                    mean[mode] = [mean[mode][c] - k * dd[c] for c in range(C)]
                    varnew = var + k * (dist2 - var)
                    varnew = VAR_MIN if varnew < VAR_MIN else varnew
                    varnew = VAR_MAX if varnew > VAR_MAX else varnew
                    gv[mode] = varnew
                    for i in range(mode, 0, -1):
                        if weight < gw[i - 1]:
                            break
                        swap_count += 1
                        swap(i, i - 1)
            if weight < -prune:
                weight = F32(0)
                nmodes -= 1
            gw[mode - swap_count] = weight
            total = total + weight
            mode += 1
        inv = F32(1) / total if abs(total) > FLT_EPSILON else F32(0)
        for m in range(nmodes):
            gw[m] = gw[m] * inv
        if not fits and alpha_t > 0:
            if nmodes == NM:
                mode = NM - 1
            else:
                mode = nmodes
                nmodes += 1
            if nmodes == 1:
                gw[mode] = F32(1)
            else:
                gw[mode] = alpha_t
                for i in range(nmodes - 1):
                    gw[i] = gw[i] * alpha1
            mean[mode] = list(x)
            gv[mode] = VAR_INIT
            for i in range(nmodes - 1, 0, -1):
                if alpha_t < gw[i - 1]:
                    break
                swap(i, i - 1)
        self.n[p] = nmodes
        if background:
            return 0
        return SHADOW if self.shadows and self._shadow(x, nmodes, gw, gv, mean) else 255

    def _shadow(self, x, nmodes, gw, gv, mean) -> bool:
        tw = F32(0)
        for m in range(nmodes):
            num, den = F32(0), F32(0)
            for c in range(len(x)):
                num = num + x[c] * mean[m][c]
                den = den + mean[m][c] * mean[m][c]
            if den == 0:
                return False
            if num <= den and num >= TAU * den:
                a = num / den
                d2 = F32(0)
                for c in range(len(x)):
                    dd = a * mean[m][c] - x[c]
                    d2 = d2 + dd * dd
                if d2 < self.tb * gv[m] * a * a:
                    return True
            tw = tw + gw[m]
            if tw > TB:
                return False
        return False

    def model(self) -> Dict[str, np.ndarray]:
        H, W_, C = self.shape
        return {"weight": np.array(self.w, F32).reshape(H, W_, NM), "variance": np.array(self.v, F32).reshape(H, W_, NM),
                "mean": np.array(self.mu, F32).reshape(H, W_, NM, C), "modes_used": np.array(self.n, np.uint8).reshape(H, W_),
                "nframes": self.nframes}


def motion_map(mask: np.ndarray, k: int) -> np.ndarray:
    """threshold(mask, 200) -> GaussianBlur(k, 0) -> threshold(25): the pixels that count as motion (bool [H, W])"""
    fg = np.where(mask == 255, 255, 0).astype(np.uint8)
    return motion_ref.blur(fg, k) > MASK_THRESHOLD


def box_count(moving: np.ndarray, rect) -> int:
    x1, y1, x2, y2 = rect
    if x2 <= x1 or y2 <= y1:
        return 0
    return int(moving[y1:y2, x1:x2].sum())


class RefBackend:
    """Numpy stand-in for telescope_cam_detection_amd.motion_filter.DeviceBackend (same methods)."""

    def __init__(self, history: int = 500, var_threshold=16, detect_shadows: bool = True):
        self.mog = Mog2(history, var_threshold, detect_shadows)
        self.calls = 0
        self.updates = 0
        self.configures = 0
        self.closed = False

    def configure(self, history: int, var_threshold, detect_shadows: bool) -> None:
        self.configures += 1
        self.mog = Mog2(history, var_threshold, detect_shadows)

    def apply(self, frame, on_device: bool, rects: Sequence[Tuple[int, int, int, int]], blur_size: int) -> List[int]:
        self.calls += 1
        f = frame.cpu().numpy() if on_device else frame
        out = []
        for r in rects:
            mask = self.mog.apply(f)
            self.updates += 1
            out.append(box_count(motion_map(mask, blur_size), r))
        return out

    def wait_stream(self, stream) -> None:
        pass

    def model(self):
        return self.mog.model() if self.mog.shape is not None and self.mog.nframes else None

    def close(self) -> None:
        self.closed = True


def sequence(h: int, w: int, C: int, n: int, seed: int = 0) -> List[np.ndarray]:
    """A test scene: a static textured background with +-3 noise, a bright block moving across it and a region darkened to 0.6 (a
    shadow) from the middle of the sequence on; a flat region at 0.3 of the background (not a shadow) in every third frame."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (60 + 40 * np.sin(yy / 7.0) + 40 * np.cos(xx / 11.0) + rng.integers(0, 60, (h, w))).astype(np.int16)
    base = np.repeat(base[:, :, None], C, axis=2) + (np.arange(C, dtype=np.int16) * 17)[None, None, :]
    out = []
    for t in range(n):
        f = base + rng.integers(-3, 4, base.shape)
        bh, bw = max(1, h // 4), max(1, w // 5)
        y0, x0 = (t * max(1, h // 9)) % max(1, h - bh + 1), (t * max(1, w // 7)) % max(1, w - bw + 1)
        f[y0:y0 + bh, x0:x0 + bw] = 235
        if t >= n // 2:
            f[h // 2:, : w // 2] = (f[h // 2:, : w // 2] * 0.6).astype(np.int16)
        if t % 3 == 2:
            f[: h // 3, w // 2:] = (base[: h // 3, w // 2:] * 0.3).astype(np.int16)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out
