"""rtd_yolox_post_run on the GPU against tests/yolox_ref.py.

With decode = 0 every operation involved (obj * class_conf, cx -+ w / 2, the areas, the IoU) is a single correctly rounded fp32 operation,
so rows are compared with the fp32 restatement BIT FOR BIT, in order, and the counts exactly.  The seeded inputs meet the margin
conditions tests/test_yolox_host.py asserts (no same-class candidate pair's IoU within 1e-5 of the threshold, no score within 1e-5 of the
confidence threshold), the hand-built ones are exact by construction."""
import ctypes as C

import numpy as np
import pytest

from telescope_cam_detection_amd import _capi, yolox_detector as yd
from telescope_cam_detection_amd.coco_constants import WILDLIFE_CLASSES
from tests import yolox_ref as ref

pytestmark = pytest.mark.gpu
CONF, NMS = ref.CONF, ref.NMS
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def be80():
    be = yd.DeviceBackend(0, 80, 4, 8400, 2048)
    yield be
    be.close()


@pytest.fixture(scope="module")
def be3():
    be = yd.DeviceBackend(0, 3, 4, 1024, 256)
    yield be
    be.close()


def run(be, pred, conf=CONF, nms=NMS, **kw):
    """(rows, counts) as numpy; rows and counts start as SENTINEL / -7 so that what the call left unwritten shows"""
    import torch
    t = pred if hasattr(pred, "is_cuda") else torch.from_numpy(np.ascontiguousarray(pred, np.float32)).cuda()
    n = t.shape[0]
    rows = torch.full((n, be.max_candidates, ref.ROW), SENTINEL, dtype=torch.float32, device="cuda")
    counts = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    be.run(t, conf, nms, out=(rows, counts), **kw)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), counts.cpu().numpy()


def check(be, pred, conf=CONF, nms=NMS, class_keep=None, device_pred=None):
    """the call's rows and counts against the fp32 restatement, bit for bit; returns the restatement's kept anchors per image"""
    rows, counts = run(be, pred if device_pred is None else device_pred, conf, nms, class_keep=class_keep)
    kept_all = []
    for i, img in enumerate(np.asarray(pred, np.float32)):
        want, passed, kept = ref.postprocess(img, conf, nms, np.float32, class_keep=class_keep, max_candidates=be.max_candidates)
        assert tuple(counts[i]) == (len(want), passed), (i, counts[i], len(want), passed)
        got = rows[i, :len(want)]
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), (i, np.abs(got - want).max())
        assert (rows[i, len(want):] == SENTINEL).all()                       # rows past `kept` are not written
        kept_all.append(list(kept))
    return kept_all


@pytest.mark.parametrize("name", ["a126_c80", "a126_c3", "a504_c80"])
def test_seeded_clusters_bit_for_bit(name, be80, be3):
    pred = ref.seeded(name)
    kept = check(be3 if pred.shape[2] == 8 else be80, pred)
    assert all(6 <= len(k) <= 42 for k in kept)


def rows_by_rank(ranked, A, C, seed):
    """`ranked`: (cx, cy, w, h, class) in the order the scores shall rank them; scattered over A anchors, the rest never passes"""
    rng = np.random.default_rng(seed)
    pred = np.zeros((1, A, 5 + C), np.float32)
    pred[0, :, 0:4] = 5.0
    where = rng.permutation(A)[:len(ranked)]
    for rank, (a, (cx, cy, w, h, cls)) in enumerate(zip(where, ranked)):
        pred[0, a, 0:4] = cx, cy, w, h
        pred[0, a, 4] = 0.99 - 0.001 * rank
        pred[0, a, 5 + cls] = 0.9
    return pred, where


def test_a_chain_across_a_chunk_boundary(be3):
    """a suppresses b, b alone would suppress c, IoU(a, c) is below the threshold: a and c stay.  b and c at ranks 63 and 64, a second
    chain at ranks 126, 127 and 129; the other 124 rows are disjoint boxes of other classes."""
    K = 130
    chain = {10: (50, 50), 63: (53, 50), 64: (56, 50), 126: (50, 100), 127: (53, 100), 129: (56, 100)}       # IoU 7/13, 7/13, 4/16
    ranked = [(chain[r][0], chain[r][1], 10, 10, 0) if r in chain else (200 + 12 * (r % 16), 12 * (r // 16), 10, 10, 1 + r % 2) for r in range(K)]
    pred, where = rows_by_rank(ranked, 200, 3, 5)
    kept = check(be3, pred)[0]
    assert len(kept) == K - 2
    assert {int(where[r]) for r in (10, 64, 126, 129)} <= set(kept) and not {int(where[63]), int(where[127])} & set(kept)


def row(cx, cy, w, h, obj, *cls):
    return [cx, cy, w, h, obj, *cls]


def test_tie_rules(be3):
    pred = np.array([[
        row(20, 20, 8, 8, 0.9, 0.8, 0.1, 0.1), row(20, 20, 8, 8, 0.8, 0.1, 0.8, 0.1),      # 0, 1: one box, two classes: both stay
        row(60, 20, 8, 8, 0.7, 0.1, 0.1, 0.9), row(60, 20, 8, 8, 0.9, 0.1, 0.1, 0.9),      # 2, 3: one box, one class: the lower score goes
        row(20, 60, 8, 8, 0.6, 0.9, 0.1, 0.1), row(20, 60, 8, 8, 0.6, 0.9, 0.1, 0.1),      # 4, 5: equal scores: the lower anchor stays
        row(60, 60, 8, 8, 0.5, 0.8, 0.2, 0.8),                                              # 6: two equal class maxima: class 0
        row(90, 90, 8, 8, 0.6, 0.1, 0.9, 0.1), row(120, 90, 8, 8, 0.6, 0.1, 0.9, 0.1),     # 7, 8: equal scores, apart: anchor order
    ]], np.float32)
    kept = check(be3, pred, 0.25, 0.5)[0]
    assert kept == [3, 0, 1, 4, 7, 8, 6]
    rows, counts = run(be3, pred, 0.25, 0.5)
    assert rows[0, 6, 6] == 0.0 and tuple(counts[0]) == (7, 9)


def test_greater_or_equal_and_strictly_greater(be3):
    pred = np.array([[
        row(2, 2, 4, 4, 0.5, 0.5, 0, 0), row(2, 1, 4, 2, 0.9, 0.9, 0, 0),                  # score exactly 0.25; IoU exactly 0.5: both stay
        row(50, 50, 0, 0, 0.9, 0, 0.9, 0), row(50, 50, 0, 0, 0.8, 0, 0.9, 0),              # zero area, 0 / 0: both stay
    ]], np.float32)
    assert check(be3, pred, 0.25, 0.5)[0] == [1, 2, 3, 0]


def test_nothing_passing_and_nan(be3):
    full = ref.seeded("a126_c3")
    empty = np.full_like(full[0], 0.1)
    kept = check(be3, np.stack([full[0], empty, full[1]]))
    assert len(kept[0]) > 0 and kept[1] == [] and len(kept[2]) > 0
    assert check(be3, empty[None]) == [[]]
    nan = full[:1].copy()
    objects = np.nonzero(nan[0, :, 4] > 0.5)[0]
    nan[0, objects[0::3], 4] = np.nan                                                      # NaN obj
    nan[0, objects[1::3], 5 + 1] = np.nan                                                  # a NaN class score
    kept = check(be3, nan)[0]
    assert 0 < len(kept) and not set(kept) & (set(objects[0::3]) | set(objects[1::3]))


def test_more_rows_pass_than_max_candidates():
    be = yd.DeviceBackend(0, 80, 1, 126, ref.CUT)
    try:
        pred = ref.seeded("a126_cut")
        check(be, pred)                                                                     # (the restatement is cut to be.max_candidates)
        rows, counts = run(be, pred)
        assert counts[0][1] == 100 and 0 < counts[0][0] <= ref.CUT
    finally:
        be.close()


def test_class_keep(be80):
    pred = ref.wildlife_variant(ref.seeded("a126_c80"), sorted(WILDLIFE_CLASSES))
    keep = sorted(WILDLIFE_CLASSES)
    kept = check(be80, pred, class_keep=keep)
    everything = check(be80, pred)
    for k, e, img in zip(kept, everything, pred):
        assert 0 < len(k) < len(e)
        assert k == [a for a in e if int(img[a, 5:].argmax()) in WILDLIFE_CLASSES]         # the filter before the NMS = the filter after it


def test_rows_at_any_4_byte_address(be80):
    import torch
    pred = ref.seeded("a126_c80")
    big = torch.zeros(pred.size + 1, dtype=torch.float32, device="cuda")
    view = big[1:].view(pred.shape)
    view.copy_(torch.from_numpy(pred))
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    check(be80, pred, device_pred=view)


def test_a_small_call_after_a_large_one(be80):
    check(be80, ref.seeded("a504_c80"))
    check(be80, ref.seeded("a126_c80"))


@pytest.mark.parametrize("name", ["h64x96", "h160x160"])
def test_decode_against_fp64(name, be80):
    """decode = 1: the same kept rows in the same order as the fp64 restatement; obj, class_conf and class_id exact; each coordinate
    within 4 * 2^-23 * m of fp64, m = max(|cx|, |cy|) + max(w, h) of that row: one ulp for expf and one rounding each for the
    add, the half-width and the corner (no other bound for expf was found in the installed ROCm; the worst measured is 0.43 x 2^-23 m)."""
    pred, in_hw = ref.head_seeded(name)
    rows, counts = run(be80, pred, decode=True, in_hw=in_hw)
    for i, img in enumerate(pred):
        want, passed, kept = ref.postprocess(img, CONF, NMS, np.float64, in_hw=in_hw)
        assert tuple(counts[i]) == (len(want), passed)
        got = rows[i, :len(want)]
        assert np.array_equal(got[:, 4:].astype(np.float64), want[:, 4:])
        box = ref.decode(img, in_hw, np.float64)[kept, :4]
        m = np.maximum(np.abs(box[:, 0]), np.abs(box[:, 1])) + np.maximum(box[:, 2], box[:, 3])
        err = np.abs(got[:, :4].astype(np.float64) - want[:, :4])
        print(f"{name}[{i}]: {len(want)} rows, worst coordinate error {float((err / m[:, None]).max()) / 2 ** -23:.2f} x 2^-23 m")
        assert (err <= 4 * 2.0 ** -23 * m[:, None]).all()


def test_refused_calls_between_two_valid_ones():
    import torch
    be = yd.DeviceBackend(0, 80, 2, 126, 128)
    try:
        pred_np = ref.seeded("a126_c80")
        pred = torch.from_numpy(pred_np).cuda()
        first = run(be, pred)
        rows = torch.full((3, 128, ref.ROW), SENTINEL, dtype=torch.float32, device="cuda")
        counts = torch.full((3, 2), -7, dtype=torch.int32, device="cuda")
        three = torch.cat([pred, pred[:1]])
        ok, dec = be.params(CONF, NMS), be.params(CONF, NMS, True, (64, 64))               # a 64 x 64 input has 84 anchors, not 126
        refused = [(3, three.data_ptr(), 126, ok, b"max_batch"), (2, pred.data_ptr(), 126, dec, b"84 anchors"), (2, None, 126, ok, b"null"),
                   (2, pred.data_ptr(), 126, be.params(1.5, NMS), b"conf_threshold"), (2, pred.data_ptr(), 127, ok, b"max_anchors")]
        for n, ptr, A, params, msg in refused:
            rc = be.run_raw(n, ptr, A, params, rows.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == _capi.RTD_E_INVALID
            assert msg in (be._fn("last_error")(be._h) or b""), be._fn("last_error")(be._h)
        torch.cuda.synchronize()
        assert (rows == SENTINEL).all() and (counts == -7).all()
        with pytest.raises(_capi.RtdError, match="nms_threshold"):
            be.run(pred, CONF, float("nan"))
        second = run(be, pred)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    finally:
        be.close()
    assert not be._h.value


def test_detector_on_the_device_back_end_equals_the_numpy_one():
    import torch
    pred = ref.wildlife_variant(ref.seeded("a126_c80"), sorted(WILDLIFE_CLASSES))
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda() for s in ((48, 80, 3), (120, 100, 3))]
    for wildlife_only in (True, False):
        dev = yd.YOLOXDetector(device="cuda:0", input_size=(64, 96), model=ref.StandInModel(pred), wildlife_only=wildlife_only)
        host = yd.YOLOXDetector(device="cuda:0", input_size=(64, 96), model=ref.StandInModel(pred), wildlife_only=wildlife_only,
                                backend=ref.RefBackend(max_anchors=126))
        try:
            assert dev.load_model() and host.load_model() and isinstance(dev._backend, yd.DeviceBackend)
            got, want = dev.detect_batch(frames), host.detect_batch(frames)
            assert got == want and all(len(d) > 0 for d in want)
            assert dev.detect(frames[1]) == host.detect(frames[1])
        finally:
            dev.close()
