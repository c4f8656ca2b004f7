"""Shared helpers for the parity tests (fixtures -> inputs, order-tolerant comparators)."""
import os

import numpy as np
import torch

from telescope_cam_detection_amd.arch import ARCHS
from telescope_cam_detection_amd.synth import make_frame
from telescope_cam_detection_amd.weights import synth_weights

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixture name -> arch (the .npz carries seeds / sizes / frame list itself)
CASE_ARCH = {
    "c1_r18_640_bs1": "r18", "c1_r18_640_scene": "r18", "c1_r18_640_resize": "r18",
    "c2_r50_640_bs8": "r50", "c2_r50_640_scene_bs2": "r50", "c3_r101_1280_bs1": "r101", "c3_r101_1280_bs4": "r101", "c4_r18_1920_bs1": "r18",
    "t_tiny_160": "tiny", "t_tiny_160x224": "tiny", "t_tinyb_192x128": "tinyb", "t_tinyc_160x224": "tinyc",
}


def load_case(name):
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    arch = ARCHS[CASE_ARCH[name]]
    wseed, ih, iw, n = (int(v) for v in g["meta"])
    kind = str(g["kind"])
    frames = [make_frame(kind, int(s), int(h), int(w)) for s, h, w in g["frames"]]
    return arch, wseed, (ih, iw), frames, g


_WCACHE = {}


def weights_for(arch, seed):
    key = (arch, seed)          # the frozen Arch itself: two replace() variants may share a name, never their weights
    if key not in _WCACHE:
        _WCACHE[key] = synth_weights(arch, seed)
    return _WCACHE[key]


def to64(w, x):
    """the weight dict and the input cast to double: the oracle then runs end to end in fp64 (integer tensors pass through)"""
    w64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in w.items()}
    return w64, x.double()


def sample(t, n=2048):
    f = torch.as_tensor(t).detach().float().flatten()
    step = max(1, f.numel() // n)
    return f[::step][:n].numpy()


def match_detections(ref_labels, ref_boxes, ref_scores, labels, boxes, scores, score_tol, box_tol, return_unmatched=False):
    """Order-tolerant comparison of two (labels, boxes, scores) triples for ONE frame.

    torch.topk's tie order is unspecified and equal / near-equal scores exist even in fp32
    (SURVEY.md §7 "hard parts"), so rows are matched greedily: same label, |dscore| <= score_tol,
    max|dbox| <= box_tol.  Returns (n_matched, n_ref, worst_score_err, worst_box_err over matches)
    [+ the indices of the reference rows left without a partner when return_unmatched].
    """
    ref_labels, labels = np.asarray(ref_labels), np.asarray(labels)
    ref_boxes, boxes = np.asarray(ref_boxes, np.float64), np.asarray(boxes, np.float64)
    ref_scores, scores = np.asarray(ref_scores, np.float64), np.asarray(scores, np.float64)
    used = np.zeros(len(labels), bool)
    matched, ws, wb = 0, 0.0, 0.0
    unmatched = []
    for i in range(len(ref_labels)):
        cand = np.where((labels == ref_labels[i]) & ~used & (np.abs(scores - ref_scores[i]) <= score_tol))[0]
        if len(cand) == 0:
            unmatched.append(i)
            continue
        d = np.abs(boxes[cand] - ref_boxes[i]).max(axis=1)
        j = int(np.argmin(d))
        if d[j] <= box_tol:
            used[cand[j]] = True
            matched += 1
            ws = max(ws, abs(scores[cand[j]] - ref_scores[i]))
            wb = max(wb, d[j])
        else:
            unmatched.append(i)
    if return_unmatched:
        return matched, len(ref_labels), ws, wb, unmatched
    return matched, len(ref_labels), ws, wb


# ---- which way k_topk goes for one image (csrc/ops.hip), restated on the CPU ----
def topk_path(keys_1d, K):
    """"fast", "general/all-ties" or "general/in-order" for one image's fp32 keys: the kernel orders keys as sign-flipped uint32, throws
    them into 1024 bags by a hash of their index, and takes the fast path when at most 1024 keys reach L, the K-th largest bag maximum
    (empty bags count as 0).  Otherwise, with T the K-th largest key, the tie group at T is either wholly taken or walked in index order."""
    u = np.ascontiguousarray(np.asarray(keys_1d, dtype=np.float32)).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    bag = ((np.arange(key.size, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)
    maxima = np.zeros(1024, np.uint32)
    np.maximum.at(maxima, bag.astype(np.int64), key)
    L = np.sort(maxima)[::-1][K - 1]
    if int((key >= L).sum()) <= 1024:
        return "fast"
    T = np.sort(key)[::-1][K - 1]
    return "general/all-ties" if int((key == T).sum()) == K - int((key > T).sum()) else "general/in-order"


def plateau_keys(B, N, K):
    """[B, N] keys that are all 1.0 but for K // 3 at 3.0 and K - K // 3 at 2.0 in random places: the special keys collide in bags, so the
    bag bound falls to 1.0 and every key is a candidate; the K-th largest is 2.0 and its whole tie group is taken ("general/all-ties")"""
    g = torch.Generator().manual_seed(N * 7 + K)
    keys = torch.ones(B, N)
    for b in range(B):
        perm = torch.randperm(N, generator=g)
        keys[b, perm[:K // 3]] = 3.0
        keys[b, perm[K // 3:K]] = 2.0
    return keys


# ---- the tolerance rule of the kernel-level fp64 comparisons (tests/test_gpu_decoder_ops.py) ----
FACTOR = 4.0


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def error_figures(got, ref64, ref32):
    """(err, e_ref, ulp) of within(): max |got - ref64|, the fp32 reference's own loss max |ref32 - ref64|, one fp32 ulp of max |ref64|"""
    got, ref64, ref32 = (torch.as_tensor(t).double().reshape(-1) for t in (got, ref64, ref32))
    assert torch.isfinite(ref64).all(), "the reference itself must be finite"
    return (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item(), ulp32(ref64.abs().max().item())


def within(family, name, got, ref64, ref32, factor=FACTOR):
    """|got - ref64| <= factor * (e_ref + ulp(max |ref64|)) with e_ref = max |ref32 - ref64|; prints the figures first"""
    got = torch.as_tensor(got).double().reshape(-1)
    err, e_ref, ulp = error_figures(got, ref64, ref32)
    print(f"[{family}] {name}: kernel err {err:.3e}, e_ref {e_ref:.3e}, ulp {ulp:.3e}, ratio {err / (e_ref + ulp):.2f} (allowed {factor})")
    assert torch.isfinite(got).all(), (family, name)
    assert err <= factor * (e_ref + ulp), (family, name, err, e_ref, ulp)
