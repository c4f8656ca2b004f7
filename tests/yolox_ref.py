"""YOLOX post-processing restated in numpy (fp32 and fp64): upstream's yolox.utils.postprocess(prediction, num_classes, conf_thre, nms_thre,
class_agnostic=False) with torchvision's batched_nms in its per-class form, and the head's grid decode - the rules rtd_yolox_post_run
follows (include/rtdetr_mi355.h).  Neither yolox nor torchvision is importable here: this file restates their public source, and the host
tests hold it against two independently written versions.

Also the input generators the host and GPU tests share, `RefBackend` (the surface of yolox_detector.DeviceBackend on numpy) and the
stand-in network of the detector tests."""
import numpy as np

STRIDES = (8, 16, 32)
ROW = 7            # x1, y1, x2, y2, obj, class_conf, class_id


def anchors(in_h, in_w):
    return sum((in_h // s) * (in_w // s) for s in STRIDES)


def grids(in_h, in_w):
    """per anchor: x, y of its cell and its stride; levels in stride order, row-major over (y, x) within a level"""
    gx, gy, gs = [], [], []
    for s in STRIDES:
        hs, ws = in_h // s, in_w // s
        yv, xv = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
        gx.append(xv.reshape(-1)), gy.append(yv.reshape(-1)), gs.append(np.full(hs * ws, s))
    return np.concatenate(gx), np.concatenate(gy), np.concatenate(gs)


def decode(pred, in_hw, dtype):
    """the head's raw output [A][5 + C] -> cx, cy, w, h rows in `dtype` (YOLOXHead.decode_outputs)"""
    gx, gy, gs = (g.astype(dtype) for g in grids(*in_hw))
    p = np.array(pred, dtype=dtype)
    p[:, 0] = (p[:, 0] + gx) * gs
    p[:, 1] = (p[:, 1] + gy) * gs
    p[:, 2] = np.exp(p[:, 2]) * gs
    p[:, 3] = np.exp(p[:, 3]) * gs
    return p


def corners(p):
    half_w, half_h = p[:, 2] / 2, p[:, 3] / 2
    return np.stack([p[:, 0] - half_w, p[:, 1] - half_h, p[:, 0] + half_w, p[:, 1] + half_h], 1)


def iou_one_to_many(box, area, boxes, areas):
    """torchvision's nms arithmetic, in the dtype of its arguments"""
    zero = boxes.dtype.type(0)
    iw = np.maximum(zero, np.minimum(box[2], boxes[:, 2]) - np.maximum(box[0], boxes[:, 0]))
    ih = np.maximum(zero, np.minimum(box[3], boxes[:, 3]) - np.maximum(box[1], boxes[:, 1]))
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area + areas - inter)


def class_max(cls):
    """torch.max over the class scores: the largest and the lowest index that holds it; a NaN anywhere gives NaN"""
    cid = np.argmax(np.where(np.isnan(cls), -np.inf, cls), 1)
    conf = cls[np.arange(len(cls)), cid]
    return np.where(np.isnan(cls).any(1), cls.dtype.type(np.nan), conf), cid


def candidates(pred, conf, dtype=np.float32, in_hw=None, class_keep=None, max_candidates=None):
    """(boxes [m][4], obj, class_conf, class_id, score, anchor) of the rows that pass, ranked (score descending, anchor ascending) and cut
    to the best max_candidates; and how many passed"""
    p = decode(pred, in_hw, dtype) if in_hw is not None else np.asarray(pred, dtype=dtype)
    cconf, cid = class_max(p[:, 5:])
    score = p[:, 4] * cconf
    with np.errstate(invalid="ignore"):
        ok = score >= dtype(np.float32(conf))
    if class_keep is not None:
        ok &= np.isin(cid, np.asarray(sorted(class_keep), dtype=np.int64))
    idx = np.nonzero(ok)[0]
    score_ok = score[idx] + dtype(0)                     # (-0 and +0 are one score)
    order = np.lexsort((idx, -score_ok))
    passed = len(idx)
    idx = idx[order][:max_candidates]
    return corners(p[idx]), p[idx, 4], cconf[idx], cid[idx], score[idx], idx, passed


def greedy(boxes, cid, nms):
    """ranks kept by the greedy per-class walk over ranked boxes"""
    thr = boxes.dtype.type(np.float32(nms))
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    kept = []
    for i in range(len(boxes)):
        same = [j for j in kept if cid[j] == cid[i]]
        if same:
            iou = iou_one_to_many(boxes[i], area[i], boxes[same], area[same])
            if (iou > thr).any():                        # (NaN > thr is False: the row stays)
                continue
        kept.append(i)
    return kept


def postprocess(pred, conf, nms, dtype=np.float32, in_hw=None, class_keep=None, max_candidates=None):
    """one image: (rows [kept][7] in `dtype`, passed, anchors of the kept rows)"""
    boxes, obj, cconf, cid, score, idx, passed = candidates(pred, conf, dtype, in_hw, class_keep, max_candidates)
    kept = greedy(boxes, cid, nms)
    rows = np.concatenate([boxes[kept], obj[kept, None], cconf[kept, None], cid[kept, None].astype(dtype)], 1).reshape(-1, ROW)
    return rows, passed, idx[kept]


def margins(pred, conf, nms, in_hw=None, class_keep=None, max_candidates=None):
    """in fp64: (min |IoU - nms| over ALL same-class candidate pairs - the bit matrix evaluates every one, the greedy walk only some -,
    min |score - conf| over all rows)"""
    boxes, obj, cconf, cid, score, idx, passed = candidates(pred, conf, np.float64, in_hw, class_keep, max_candidates)
    p = decode(pred, in_hw, np.float64) if in_hw is not None else np.asarray(pred, np.float64)
    all_conf, _ = class_max(p[:, 5:])
    all_score = p[:, 4] * all_conf
    all_score = all_score[~np.isnan(all_score)]
    d_score = float(np.abs(all_score - float(np.float32(conf))).min()) if len(all_score) else np.inf
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    d_iou = np.inf
    for i in range(len(boxes) - 1):
        same = np.nonzero(cid[i + 1:] == cid[i])[0] + i + 1
        if len(same):
            iou = iou_one_to_many(boxes[i], area[i], boxes[same], area[same])
            iou = iou[~np.isnan(iou)]
            if len(iou):
                d_iou = min(d_iou, float(np.abs(iou - float(np.float32(nms))).min()))
    return d_iou, d_score


class RefBackend:
    """yolox_detector.DeviceBackend's surface on numpy: run() returns (rows [n][max_candidates][7] float32, counts [n][2] int32); rows
    past `kept` are zero here (the device leaves them unwritten)"""

    def __init__(self, device=0, num_classes=80, max_batch=8, max_anchors=8400, max_candidates=2048):
        self.num_classes, self.max_batch, self.max_anchors, self.max_candidates = num_classes, max_batch, max_anchors, max_candidates
        self.calls = []

    def run(self, pred, conf, nms, decode=False, in_hw=None, class_keep=None):
        pred = np.asarray(pred.detach().cpu() if hasattr(pred, "detach") else pred, np.float32)
        n, A, F = pred.shape
        assert 1 <= n <= self.max_batch and 1 <= A <= self.max_anchors and F == 5 + self.num_classes
        self.calls.append((float(conf), float(nms), bool(decode), in_hw, None if class_keep is None else tuple(sorted(class_keep))))
        rows = np.zeros((n, self.max_candidates, ROW), np.float32)
        counts = np.zeros((n, 2), np.int32)
        for i in range(n):
            r, passed, _ = postprocess(pred[i], conf, nms, np.float32, in_hw if decode else None, class_keep, self.max_candidates)
            rows[i, :len(r)] = r
            counts[i] = len(r), passed
        return rows, counts

    def close(self):
        pass


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def clusters(seed, A, C, n_obj, dup, n=1):
    """[n][A][5 + C] fp32 rows (cx, cy, w, h, obj, class scores): per image n_obj boxes, each seen by `dup` jittered anchors of one class
    (obj and class score in 0.7..0.99: a score of 0.49 or more), over a background whose scores stay below 0.09.  Coordinates stay
    below 200."""
    rng = np.random.default_rng(seed)
    assert n_obj * dup <= A
    pred = np.empty((n, A, 5 + C), np.float32)
    for i in range(n):
        p = pred[i]
        p[:, 0:2] = rng.uniform(10, 180, (A, 2))
        p[:, 2:4] = rng.uniform(4, 40, (A, 2))
        p[:, 4] = rng.uniform(0.0, 0.3, A)
        p[:, 5:] = rng.uniform(0.0, 0.3, (A, C))
        where = rng.permutation(A)[:n_obj * dup].reshape(n_obj, dup)
        for o in range(n_obj):
            centre, size, cls = rng.uniform(30, 160, 2), rng.uniform(12, 40, 2), int(rng.integers(0, C))
            for a in where[o]:
                p[a, 0:2] = centre + rng.uniform(-3, 3, 2)
                p[a, 2:4] = size * rng.uniform(0.8, 1.2, 2)
                p[a, 4] = rng.uniform(0.7, 0.99)
                p[a, 5 + cls] = rng.uniform(0.7, 0.99)
    return pred


def head_clusters(seed, in_hw, C, n_obj, n=1):
    """[n][anchors][5 + C] fp32 head output (decode = 1): t2, t3 in [-1, 2] everywhere; per image n_obj objects, each seen by the four
    cells of a 2 x 2 block of one level"""
    rng = np.random.default_rng(seed)
    in_h, in_w = in_hw
    A = anchors(in_h, in_w)
    first = np.cumsum([0] + [(in_h // s) * (in_w // s) for s in STRIDES])
    pred = np.empty((n, A, 5 + C), np.float32)
    for i in range(n):
        p = pred[i]
        p[:, 0:2] = rng.uniform(-0.5, 1.5, (A, 2))
        p[:, 2:4] = rng.uniform(-1.0, 2.0, (A, 2))
        p[:, 4] = rng.uniform(0.0, 0.3, A)
        p[:, 5:] = rng.uniform(0.0, 0.3, (A, C))
        used = set()
        for o in range(n_obj):
            lvl = int(rng.integers(0, 3))
            s, hs, ws = STRIDES[lvl], in_h // STRIDES[lvl], in_w // STRIDES[lvl]
            gx, gy = int(rng.integers(0, ws - 1)), int(rng.integers(0, hs - 1))
            if (lvl, gx, gy) in used:
                continue
            used.add((lvl, gx, gy))
            centre = np.array([gx + 1.0, gy + 1.0]) + rng.uniform(-0.2, 0.2, 2)          # in cells
            size, cls = rng.uniform(0.6, 1.7, 2), int(rng.integers(0, C))               # log of the size in cells
            for dy in (0, 1):
                for dx in (0, 1):
                    a = first[lvl] + (gy + dy) * ws + gx + dx
                    p[a, 0:2] = centre - (gx + dx, gy + dy) + rng.uniform(-0.08, 0.08, 2)
                    p[a, 2:4] = size + rng.uniform(-0.1, 0.1, 2)
                    p[a, 4] = rng.uniform(0.7, 0.99)
                    p[a, 5:] = rng.uniform(0.0, 0.3, C)
                    p[a, 5 + cls] = rng.uniform(0.7, 0.99)
    return pred


# the seeded inputs of the GPU tests at conf 0.25, NMS threshold 0.45: (name, A, C, objects, duplicates, images, seed).  The host tests
# assert the margin conditions for every one.
CONF, NMS = 0.25, 0.45
SEEDED = [("a126_c80", 126, 80, 6, 5, 2, 11), ("a126_c3", 126, 3, 8, 12, 3, 12), ("a504_c80", 504, 80, 30, 10, 1, 13),
          ("a126_cut", 126, 80, 10, 10, 1, 14)]           # the last one: 100 rows pass, for a handle with max_candidates = 64
CUT = 64
HEAD_SEEDED = [("h64x96", (64, 96), 80, 5, 2, 21), ("h160x160", (160, 160), 80, 12, 1, 22)]      # (name, in_hw, C, objects, images, seed)


def seeded(name):
    _, A, C, n_obj, dup, n, seed = next(s for s in SEEDED if s[0] == name)
    return clusters(seed, A, C, n_obj, dup, n)


def head_seeded(name):
    _, in_hw, C, n_obj, n, seed = next(s for s in HEAD_SEEDED if s[0] == name)
    return head_clusters(seed, in_hw, C, n_obj, n), in_hw


def wildlife_variant(pred, wildlife_ids):
    """`pred` with every other object row's class moved to one of `wildlife_ids`, so that a wildlife filter keeps some rows and drops
    others (the detector tests)"""
    pred = pred.copy()
    wl = list(wildlife_ids)
    for img in pred:
        for a in np.nonzero(img[:, 4] > 0.5)[0][::2]:
            c, w = int(img[a, 5:].argmax()), wl[a % len(wl)]
            img[a, 5 + c], img[a, 5 + w] = img[a, 5 + w], img[a, 5 + c]
    return pred


class StandInModel:
    """a network stand-in: whatever [B, 3, H, W] batch comes in, the rows of `pred` ([B_max][A][5 + C]) for its first B images, on the
    input's device"""

    def __init__(self, pred):
        self.pred = pred
        self.shapes = []

    def __call__(self, x):
        import torch
        self.shapes.append(tuple(x.shape))
        return torch.from_numpy(self.pred[:x.shape[0]]).to(x.device)
