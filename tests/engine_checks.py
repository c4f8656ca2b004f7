"""GPU-side checks that more than one test file runs on its own cases (tests/test_gpu_head_configs.py, tests/test_gpu_variants.py): an
engine for a case, the path its plan took, and four bodies - the f16x3 stage bounds, the fused against the per-op decoder, graph replay
with batch invariance, and the side-stream plan against the serial one.  A case `d` is the dict of tests.util.reference_runs (or any
dict with arch, w, frames and input_size).  Every tolerance is one tests/test_gpu_parity.py already has."""
import numpy as np

from tests.util import by_token, match_detections

FUSED, PER_OP, THREE = "fused", "per-op", "three-launch"


def make_engine(d, precision, frames=None, use_graph=False, profile=0):
    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.weights import fold_weights, pack_blob
    if "blob" not in d:
        d["blob"] = pack_blob(fold_weights(d["arch"], d["w"]))
    return _capi.Engine(d["arch"], d["blob"], device=0, precision=_capi.precision_code(precision), max_batch=len(frames or d["frames"]),
                        input_size=d["input_size"], use_graph=use_graph, profile=profile)


def plan_paths(eng, n):
    """(decoder, post-processor, AIFI) paths of the plan of batch size n, read from its launch names"""
    names = [p["name"] for p in eng.profile(n, 1)]
    fused = "dec.prologue" in names and "dec.l0.fused" in names
    per_op = "dec.l0.ca.sample" in names
    assert fused != per_op, names
    post_fused = "post.fused" in names
    three = all(x in names for x in ("post.sigmoid", "post.topk", "post.gather"))
    assert post_fused != three, names
    return (FUSED if fused else PER_OP, FUSED if post_fused else THREE, FUSED if "enc.aifi.layer" in names else PER_OP)


def assert_same(a, b, what):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=what)


def oracle64_refs(d):
    l64, b64, s64 = d["out64"]
    return [("oracle64", l64, b64, s64)]


def check_f16x3_stages(eng, d):
    """one infer_raw of an f16x3 engine on the case's frames: bit-exact input, then the stage bounds of
    test_gpu_parity.test_f16x3_engine_matches_oracle_and_golden against the fp64 oracle's stages"""
    from tests.test_gpu_parity import nchw, rel_err
    name, col = d["name"], d["col"]
    eng.infer_raw(d["frames"])
    np.testing.assert_array_equal(nchw(eng.debug_tensor("input"))[:, :3], col["input"].numpy())
    for i in range(3):
        e = rel_err(nchw(eng.debug_tensor(f"backbone{i}")), col[f"backbone{i}"].numpy())
        print(f"{name} backbone{i} rel l2 err {e:.2e}")
        assert e < 4e-5, (f"backbone{i}", e)
    for i in range(3):
        e = rel_err(nchw(eng.debug_tensor(f"enc{i}")), col[f"enc{i}"].numpy())
        print(f"{name} enc{i} rel l2 err {e:.2e}")
        assert e < 1e-4, (f"enc{i}", e)
    mx = eng.debug_tensor("enc_cls_max")[:, :, 0, 0]
    print(f"{name} enc score max abs err {np.abs(mx - col['enc_cls_max'].numpy()).max():.2e}")
    np.testing.assert_allclose(mx, col["enc_cls_max"].numpy(), atol=5e-4)


def check_fused_decoder_equals_per_op(d, precision):
    """dec_fused 1 against 0 at the bounds of test_gpu_parity.test_fused_decoder_equals_per_op_decoder.  The per-op kernels are each held
    to fp64 at kernel level (test_gpu_ops.py, test_gpu_decoder_ops.py), so a difference here is the row kernel's.

    Two passes per engine.  Free-running: dec_fused = 0 also swaps the selection chain for its per-op form, whose scores differ in the
    last bits, so two tokens of near-equal score may trade ranks - the same query set in another row order (seen: 2 or 4 rows of q320,
    q1024 and c512_ffn512).  The pass asserts exactly that - both engines select one token set on every frame - and compares hs and ref
    token by token (by_token) and the final rows order-tolerantly.  Then both engines run on the reference's selection in its order, and
    hs and ref are compared row by row as the original test does."""
    from telescope_cam_detection_amd import _capi
    name, arch, frames = d["name"], d["arch"], d["frames"]
    last = f"dec{arch.dec_layers - 1}.hs"
    free, forced = [], []
    try:
        for fused in (0, 1):
            _capi.debug_option("dec_fused", fused)
            eng = make_engine(d, precision)
            try:
                rows = eng.infer_raw(frames)
                free.append(rows + (eng.debug_tensor(last)[:, :, 0, :], eng.debug_tensor("ref")[:, :, 0, :4],
                                    eng.debug_tensor("topk")[:, :, 0, 0].astype(np.int64)))
                eng.force_topk(d["col"]["topk"].numpy())
                forced.append(eng.infer_raw(frames) + (eng.debug_tensor(last), eng.debug_tensor("ref")))
                eng.force_topk(None)
                np.testing.assert_array_equal(eng.debug_tensor("topk")[:, :, 0, 0].astype(np.int64), d["col"]["topk"].numpy())
                assert plan_paths(eng, len(frames))[0] == (FUSED if fused else PER_OP)
            finally:
                eng.close()
    finally:
        _capi.debug_option("reset", 0)

    def rows_match(tag, l0, b0, s0, l1, b1, s1):
        for b in range(len(frames)):
            m, n, ws, wb = match_detections(l0[b], b0[b], s0[b], l1[b], b1[b], s1[b], 1e-5, 2e-3)
            print(f"{name} {precision} fused vs per-op, {tag} [{b}]: matched {m}/{n} worst dscore={ws:.2e} dbox={wb:.2e}px")
            assert m == n, (tag, b, m, n, ws, wb)

    (l0, b0, s0, h0, r0, t0), (l1, b1, s1, h1, r1, t1) = free
    for b in range(len(frames)):
        assert set(t0[b].tolist()) == set(t1[b].tolist()), (name, b, "the two selection chains chose different token sets")
        print(f"{name} {precision} free-running [{b}]: {int((t0[b] != t1[b]).sum())} of {t0.shape[1]} ranks hold another token")
        ha, hb, ra, rb = by_token(t0[b], h0[b]), by_token(t1[b], h1[b]), by_token(t0[b], r0[b]), by_token(t1[b], r1[b])
        print(f"{name} {precision} free-running [{b}]: max |dhs| {np.abs(hb - ha).max():.3e}, max |dref| {np.abs(rb - ra).max():.3e}")
        np.testing.assert_allclose(hb, ha, atol=5e-5, rtol=1e-4)
        np.testing.assert_allclose(rb, ra, atol=2e-6)
    rows_match("free-running", l0, b0, s0, l1, b1, s1)
    (l0, b0, s0, h0, r0), (l1, b1, s1, h1, r1) = forced
    print(f"{name} {precision} fused vs per-op: max |dhs| {np.abs(h1 - h0).max():.3e}, max |dref| {np.abs(r1[..., :4] - r0[..., :4]).max():.3e}")
    np.testing.assert_allclose(h1, h0, atol=5e-5, rtol=1e-4)
    np.testing.assert_allclose(r1[..., :4], r0[..., :4], atol=2e-6)
    rows_match("reference selection", l0, b0, s0, l1, b1, s1)


def check_graph_replay_and_batch_invariance(d):
    """graph replay equals eager, and frame i of the bs-2 call equals its bs-1 call, bit for bit: a block's GEMM rotation depends on its
    row tile inside its image only, at every tile count"""
    from telescope_cam_detection_amd import _capi
    frames = d["frames"]
    e1, e2 = make_engine(d, "f16x3", use_graph=False), make_engine(d, "f16x3", use_graph=True)
    try:
        a = e1.infer_raw(frames)
        for _ in range(3):                      # build, then two replays
            g = e2.infer_raw(frames)
        assert_same(a, g, "graph replay vs eager")
        for eng in (e1, e2):
            for i, f in enumerate(frames):
                one = eng.infer_raw([f])
                assert_same([t[i:i + 1] for t in a], one, f"frame {i} of the bs-2 call vs its bs-1 call")
    finally:
        e1.close(); e2.close()
        _capi.debug_option("reset", 0)


def check_side_stream_equals_serial(d):
    from telescope_cam_detection_amd import _capi
    frames, got = d["frames"], {}
    try:
        for v in (0, 7):
            _capi.debug_option("side_stream", v)
            eng = make_engine(d, "f16x3", use_graph=True)
            try:
                for _ in range(3):
                    got[v] = eng.infer_raw(frames)
            finally:
                eng.close()
    finally:
        _capi.debug_option("reset", 0)
    assert_same(got[0], got[7], "side_stream 0 vs 7")
