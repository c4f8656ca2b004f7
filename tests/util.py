"""Shared helpers for the parity tests (fixtures -> inputs, a case's oracle runs and whether they are well posed, order-tolerant
comparators)."""
import os

import numpy as np
import torch

from oracle import rtdetr_oracle as orc
from oracle.make_golden import CASES
from telescope_cam_detection_amd.arch import ARCHS
from telescope_cam_detection_amd.synth import make_frame
from telescope_cam_detection_amd.weights import synth_weights

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    """(arch, weight seed, input size, frames, npz) of a fixture; the arch comes from the generator's table, and the seeds, sizes and
    frame list the file carries must be that table's row"""
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    arch_name, wseed, input_size, frame_specs, kind = CASES[name]
    assert ([int(v) for v in g["meta"]], [tuple(int(v) for v in f) for f in g["frames"]], str(g["kind"])) == \
        ([wseed, *input_size, len(frame_specs)], frame_specs, kind), name
    return ARCHS[arch_name], wseed, input_size, [make_frame(kind, *f) for f in frame_specs], g


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


def threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))


def oracle_run(arch, w, frames, input_size, double=False):
    """one oracle run on a case's frames, in fp32 or with weights and input cast to double -> ((labels, boxes, scores), the collected
    stages with the network input under "input")"""
    threads()
    x = torch.cat([orc.preprocess(f, input_size)[0] for f in frames], 0)
    if double:
        w, x = to64(w, x)
    col = {}
    out = orc.model_forward(arch, w, x, [(f.shape[1], f.shape[0]) for f in frames], collect=col)
    col["input"] = x
    return out, col


_RUNS = {}


def reference_runs(name, arch, w, frames, input_size):
    """a case's frames and its fp32 and fp64 oracle runs, computed once per session and never changed (check_fp32_engine and x3_check of
    tests/test_gpu_parity.py read this layout: "col" is the fp64 run's stages)"""
    if (name, arch) not in _RUNS:
        out32, col32 = oracle_run(arch, w, frames, input_size)
        out64, col64 = oracle_run(arch, w, frames, input_size, double=True)
        _RUNS[name, arch] = dict(name=name, arch=arch, w=w, frames=frames, sizes=[(f.shape[1], f.shape[0]) for f in frames], x=col32["input"],
                                 input_size=input_size, out32=[t.numpy() for t in out32], out64=[t.numpy() for t in out64], col32=col32, col=col64)
    return _RUNS[name, arch]


def cut_gap(values, Q):
    """the gap between rank Q and rank Q + 1 of one frame's keys"""
    v = np.sort(np.asarray(values, np.float64).ravel())[::-1]
    return float(v[Q - 1] - v[Q])


def by_token(topk_b, rows_b):
    """a frame's query rows in token order, so that two runs with one token set line up whatever order their top-k gave"""
    return np.asarray(rows_b)[np.argsort(np.asarray(topk_b), kind="stable")]


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def well_posed(d):
    """the three conditions under which a case's reference_runs may judge an engine -> (ok, [reason, ...]); prints every figure"""
    name, Q, c32, c64 = d["name"], d["arch"].num_queries, d["col32"], d["col"]
    (l32, b32, s32), (l64, b64, s64) = d["out32"], d["out64"]
    tk32, tk64 = c32["topk"].numpy(), c64["topk"].numpy()
    mx32, mx64 = c32["enc_cls_max"].numpy().astype(np.float64), c64["enc_cls_max"].numpy()
    e_sel = float(np.abs(mx32 - mx64).max())
    bad = []
    for b in range(len(d["frames"])):
        # 1. no selection flip inside the reference
        if set(tk32[b].tolist()) != set(tk64[b].tolist()):
            bad.append(f"[{b}] the fp32 oracle selects other tokens than the fp64 oracle")
            continue
        # 2. every row of the fp32 oracle at the north-star tolerance: the reference alone spends none of the engines' allowances
        m, n, ws, wb = match_detections(l64[b], b64[b], s64[b], l32[b], b32[b], s32[b], 1e-3, 1e-2)
        print(f"{name}[{b}] fp32 oracle vs fp64 oracle: matched {m}/{n} worst dscore={ws:.2e} dbox={wb:.2e}px")
        if not m == n == Q:
            bad.append(f"[{b}] fp32 oracle rows matched {m}/{n}")
        # 3. both cuts are at least 10 x the fp32 oracle's own worst error on the quantity that is cut
        sc32, sc64 = sig(by_token(tk32[b], c32["logits"][b].numpy())), sig(by_token(tk64[b], c64["logits"][b].numpy()))
        e_post = float(np.abs(sc32 - sc64).max())
        g_sel, g_post = cut_gap(mx64[b], Q), cut_gap(sc64, Q)
        print(f"{name}[{b}] selection cut gap {g_sel:.2e} (fp32 oracle err {e_sel:.2e}), post cut gap {g_post:.2e} (err {e_post:.2e})")
        if g_sel < 10 * e_sel:
            bad.append(f"[{b}] selection cut gap {g_sel:.2e} < 10 x {e_sel:.2e}")
        if g_post < 10 * e_post:
            bad.append(f"[{b}] post cut gap {g_post:.2e} < 10 x {e_post:.2e}")
    return not bad, bad


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
