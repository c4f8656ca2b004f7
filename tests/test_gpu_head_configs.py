"""Engines at every decoder-head shape rtd_create accepts, against the fp64 oracle.

A case is a dataclasses.replace() of ARCHS["r18"] (basic blocks, 3 decoder layers: the smallest trunk with the full-width decoder) on two
320 x 320 frames (one scene, one noise): 40^2 + 20^2 + 10^2 = 2100 memory tokens, 100 AIFI tokens.  Each case exists for one path of
decoder.hip's row kernel or of the plan builder that the suite's two other head shapes (Q = 300 / 50, C = 80) never reach, and asserts
from the plan's launch names that it took that path.

The reference is the oracle in fp64 (weights and input cast to double, tests/util.to64); the fp32 oracle of the same case gives the
reference's own loss.  The CPU tests below assert per case that the data is well posed before any engine is judged on it: the fp32 oracle
selects the fp64 oracle's tokens, all its rows match at 1e-3 / 1e-2 px, and both top-k cuts are at least 10 x wider than the fp32 oracle's
own error there.  The seeds of a case were searched on the CPU for those three conditions (nothing else) and are part of the table.

Every tolerance of the GPU tests is one the suite already has (test_gpu_parity.py: check_fp32_engine, x3_check and the stage bounds of
test_f16x3_engine_matches_oracle_and_golden, test_fused_decoder_equals_per_op_decoder).  Measured figures: DESIGN.md, "Head configurations"."""
import os
from dataclasses import dataclass, replace

import numpy as np
import pytest
import torch

from oracle import rtdetr_oracle as orc
from telescope_cam_detection_amd.arch import ARCHS
from telescope_cam_detection_amd.synth import noise_frame, scene_frame
from tests.util import error_figures, match_detections, to64, weights_for

SIZE = (320, 320)
FUSED, PER_OP, THREE = "fused", "per-op", "three-launch"


@dataclass(frozen=True)
class HeadCase:
    name: str
    changes: tuple           # ((Arch field, value), ...) on ARCHS["r18"]
    seeds: tuple             # (weights, scene frame, noise frame)
    decoder: str             # the path the plan must take: FUSED (dec.prologue + dec.l<i>.fused) or PER_OP (dec.l<i>.ca.sample)
    post: str                # FUSED (post.fused) or THREE (post.sigmoid, post.topk, post.gather)
    aifi: str                # FUSED (enc.aifi.layer) or PER_OP
    why: str

    @property
    def arch(self):
        return replace(ARCHS["r18"], name="r18_" + self.name, **dict(self.changes))


def _case(name, why, seeds, decoder=FUSED, post=FUSED, aifi=FUSED, **changes):
    return HeadCase(name, tuple(sorted(changes.items())), seeds, decoder, post, aifi, why)


CASES = [
    _case("q320", "20 row tiles: even, the last one full - no clamp, no zeroed partner, no masked row", (3, 5, 6), num_queries=320),
    _case("q100_c12", "7 tiles, the last with 4 rows; the class head is one column tile", (3, 5, 6), num_queries=100, num_classes=12),
    _case("q16_c4", "one tile per image; smallest class head (column tiles < waves)", (3, 5, 6), num_queries=16, num_classes=4),
    _case("q1_c92", "one valid row and one key; partial class column tile", (3, 5, 6), num_queries=1, num_classes=92),
    # (frame seeds 5 / 6 .. 19 / 20 leave a cut gap of 2e-6 .. 3e-5 on one frame or the other: 1024 of 2100 tokens is the dense middle)
    _case("q1024", "largest Q: 64 tiles; Q * C = 81 920 -> three-launch post-processor, top-k with K = 1024", (3, 21, 22), post=THREE,
          num_queries=1024),
    _case("c512_ffn512", "widest class head the fused kernel takes; half-width FFN; three-launch post-processor", (3, 5, 6), post=THREE,
          num_classes=512, dec_ffn=512),
    _case("layers1_q96", "prologue, then at once the last-layer mode; 6 full tiles", (3, 5, 6), dec_layers=1, num_queries=96),
    # dec_ffn % 64 != 0: the row kernel walks K in 64-wide steps and was never meant to take it (its filter packer refuses the K):
    # dec_fused() declines the shape, which this case asserts, and the per-op decoder runs it
    _case("ffn480", "dec_ffn % 64 != 0: the fused kernel declines, per-op decoder", (3, 5, 6), decoder=PER_OP, dec_ffn=480),
    _case("c516", "first C that dec_fused() declines: per-op decoder at d_model 256", (3, 5, 6), decoder=PER_OP, post=THREE, num_classes=516),
    _case("ffn2048_q100", "dec_ffn > 1024: per-op decoder", (3, 5, 6), decoder=PER_OP, dec_ffn=2048, num_queries=100),
    _case("np1", "per-op decoder, sampler at the low end of n_points", (3, 5, 6), decoder=PER_OP, n_points=1, num_queries=100),
    _case("np8", "per-op decoder, sampler at the high end of n_points", (3, 5, 6), decoder=PER_OP, n_points=8, num_queries=100),
    _case("encffn512", "fused AIFI with a narrower FFN", (3, 5, 6), enc_ffn=512),
    _case("encffn2048", "enc_ffn > 1024: un-fused AIFI at enc_dim 256", (3, 5, 6), aifi=PER_OP, enc_ffn=2048),
    # enc_ffn % 64 != 0: the AIFI half of ffn480's refusal.  On f16x3 the per-op fc1 hands fc2 a pair tensor of 480 channels = 15 groups of
    # 32, an odd number of 64-wide K steps
    _case("encffn480", "enc_ffn % 64 != 0: the fused AIFI declines, per-op AIFI with an odd count of 32-channel groups", (3, 5, 6), aifi=PER_OP,
          enc_ffn=480),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
FUSED_NAMES = [c.name for c in CASES if c.decoder == FUSED]
POST_FUSED_NAMES = [c.name for c in CASES if c.post == FUSED]

_DATA = {}


def _threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))


def head_data(name):
    """a case's frames and its fp64 and fp32 oracle runs, computed once per session and never changed"""
    if name not in _DATA:
        case = BY_NAME[name]
        arch, (wseed, sseed, nseed) = case.arch, case.seeds
        w = weights_for(arch, wseed)
        frames = [scene_frame(sseed, *SIZE), noise_frame(nseed, *SIZE)]
        _threads()
        xs, sizes = zip(*[orc.preprocess(f, SIZE) for f in frames])
        x = torch.cat(xs, 0)
        col32, col64 = {}, {}
        out32 = orc.model_forward(arch, w, x, list(sizes), collect=col32)
        w64, x64 = to64(w, x)
        out64 = orc.model_forward(arch, w64, x64, list(sizes), collect=col64)
        col64["input"] = x64
        _DATA[name] = dict(name=name, case=case, arch=arch, w=w, frames=frames, sizes=list(sizes), x=x, input_size=SIZE,
                           out32=[t.numpy() for t in out32], out64=[t.numpy() for t in out64], col32=col32, col=col64)
    return _DATA[name]


def forced32(d):
    """the fp32 oracle under the fp64 oracle's selection, in its query order: row for row the e_ref of the chain ratios"""
    if "forced32" not in d:
        _threads()
        col = {}
        orc.model_forward(d["arch"], d["w"], d["x"], d["sizes"], collect=col, force_topk=d["col"]["topk"].numpy())
        d["forced32"] = col
    return d["forced32"]


def cut_gap(values, Q):
    """the gap between rank Q and rank Q + 1 of one frame's keys"""
    v = np.sort(np.asarray(values, np.float64).ravel())[::-1]
    return float(v[Q - 1] - v[Q])


def by_token(topk_b, rows_b):
    """a frame's query rows in token order, so that two runs with one token set line up whatever order their top-k gave"""
    return np.asarray(rows_b)[np.argsort(np.asarray(topk_b), kind="stable")]


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


# ------------------------------------------------------------------------------------------ CPU: the data is well posed
@pytest.mark.parametrize("name", NAMES)
def test_reference_is_well_posed(name):
    d = head_data(name)
    Q, c32, c64 = d["arch"].num_queries, d["col32"], d["col"]
    (l32, b32, s32), (l64, b64, s64) = d["out32"], d["out64"]
    tk32, tk64 = c32["topk"].numpy(), c64["topk"].numpy()
    mx32, mx64 = c32["enc_cls_max"].numpy().astype(np.float64), c64["enc_cls_max"].numpy()
    e_sel = float(np.abs(mx32 - mx64).max())
    for b in range(len(d["frames"])):
        # 1. no selection flip inside the reference
        assert set(tk32[b].tolist()) == set(tk64[b].tolist()), (name, b)
        # 2. every row of the fp32 oracle at the north-star tolerance: the reference alone spends none of the engines' allowances
        m, n, ws, wb = match_detections(l64[b], b64[b], s64[b], l32[b], b32[b], s32[b], 1e-3, 1e-2)
        print(f"{name}[{b}] fp32 oracle vs fp64 oracle: matched {m}/{n} worst dscore={ws:.2e} dbox={wb:.2e}px")
        assert m == n == Q, (name, b, m, n)
        # 3. both cuts are at least 10 x the fp32 oracle's own worst error on the quantity that is cut
        sc32 = sig(by_token(tk32[b], c32["logits"][b].numpy()))
        sc64 = sig(by_token(tk64[b], c64["logits"][b].numpy()))
        e_post = float(np.abs(sc32 - sc64).max())
        g_sel, g_post = cut_gap(mx64[b], Q), cut_gap(sc64, Q)
        print(f"{name}[{b}] selection cut gap {g_sel:.2e} (fp32 oracle err {e_sel:.2e}), post cut gap {g_post:.2e} (err {e_post:.2e})")
        assert g_sel >= 10 * e_sel, (name, b, g_sel, e_sel)
        assert g_post >= 10 * e_post, (name, b, g_post, e_post)


def test_case_table_covers_the_paths_it_names():
    """bookkeeping of the table only (the engine's path is asserted on the GPU, assert_paths): each path of each part has a case"""
    assert {c.decoder for c in CASES} == {FUSED, PER_OP} and {c.post for c in CASES} == {FUSED, THREE} and {c.aifi for c in CASES} == {FUSED, PER_OP}


# ------------------------------------------------------------------------------------------ GPU
def make_engine(d, precision, frames=None, use_graph=False):
    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.weights import fold_weights, pack_blob
    if "blob" not in d:
        d["blob"] = pack_blob(fold_weights(d["arch"], d["w"]))
    return _capi.Engine(d["arch"], d["blob"], device=0, precision=_capi.precision_code(precision), max_batch=len(frames or d["frames"]),
                        input_size=SIZE, use_graph=use_graph)


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


def assert_paths(eng, d):
    case = d["case"]
    got = plan_paths(eng, len(d["frames"]))
    print(f"{case.name}: decoder {got[0]}, post-processor {got[1]}, AIFI {got[2]}")
    assert got == (case.decoder, case.post, case.aifi), (case.name, got)


def oracle64_refs(d):
    l64, b64, s64 = d["out64"]
    return [("oracle64", l64, b64, s64)]


def print_chain_ratios(eng, d, tag):
    """with the selection forced to the reference's: err / (e_ref + ulp) of tests.util.within for every decoder layer's hidden state, the
    final reference boxes and the logits against the fp64 oracle, e_ref from the fp32 oracle under the same selection.  Printed and
    recorded, not bounded: nobody has measured these over a whole decoder chain yet."""
    arch, c64, c32 = d["arch"], d["col"], forced32(d)
    eng.force_topk(c64["topk"].numpy())
    eng.infer_raw(d["frames"])
    eng.force_topk(None)
    last = arch.dec_layers - 1
    pairs = [(f"dec{i}.hs", eng.debug_tensor(f"dec{i}.hs")[:, :, 0, :], f"dec{i}.hs") for i in range(arch.dec_layers)]
    pairs += [("ref", eng.debug_tensor("ref")[:, :, 0, :4], f"dec{last}.ref"), ("logits", eng.debug_tensor("logits")[:, :, 0, :], "logits")]
    worst = 0.0
    for label, got, key in pairs:
        err, e_ref, ulp = error_figures(got, c64[key], c32[key])
        ratio = err / (e_ref + ulp)
        worst = max(worst, ratio)
        print(f"[chain] {d['name']} {tag} {label}: err {err:.3e}, e_ref {e_ref:.3e}, ulp {ulp:.3e}, ratio {ratio:.2f}")
    print(f"[chain] {d['name']} {tag} worst ratio {worst:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fp32_engine_matches_the_fp64_oracle(name):
    from telescope_cam_detection_amd import _capi
    from tests.test_gpu_parity import check_fp32_engine
    d = head_data(name)
    eng = make_engine(d, "fp32")
    try:
        check_fp32_engine(eng, d, refs=[r + (d["col"]["enc_cls_max"].numpy(),) for r in oracle64_refs(d)])
        assert_paths(eng, d)
        print_chain_ratios(eng, d, "fp32")
    finally:
        eng.close()
        _capi.debug_option("reset", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_f16x3_engine_matches_the_fp64_oracle(name):
    """the stage bounds of test_gpu_parity.test_f16x3_engine_matches_oracle_and_golden, then x3_check (free-running and with the
    reference's selection) against the fp64 oracle"""
    from telescope_cam_detection_amd import _capi
    from tests.test_gpu_parity import nchw, rel_err, x3_check
    d = head_data(name)
    col, frames = d["col"], d["frames"]
    eng = make_engine(d, "f16x3")
    try:
        eng.infer_raw(frames)
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
        x3_check(name, d["arch"], d["w"], SIZE, eng, frames, col["topk"].numpy(), col["enc_cls_max"].numpy(), oracle64_refs(d), 5e-4)
        assert_paths(eng, d)
        print_chain_ratios(eng, d, "f16x3")
    finally:
        eng.close()
        _capi.debug_option("reset", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", FUSED_NAMES)
def test_fused_decoder_equals_per_op_decoder(name, precision):
    """dec_fused 1 against 0 at the bounds of test_gpu_parity.test_fused_decoder_equals_per_op_decoder.  The per-op kernels are each held
    to fp64 at kernel level (test_gpu_ops.py, test_gpu_decoder_ops.py), so a difference here is the row kernel's.

    Two passes per engine.  Free-running: dec_fused = 0 also swaps the selection chain for its per-op form, whose scores differ in the
    last bits, so two tokens of near-equal score may trade ranks - the same query set in another row order (seen: 2 or 4 rows of q320,
    q1024 and c512_ffn512).  The pass asserts exactly that - both engines select one token set on every frame - and compares hs and ref
    token by token (by_token) and the final rows order-tolerantly.  Then both engines run on the reference's selection in its order, and
    hs and ref are compared row by row as the original test does."""
    from telescope_cam_detection_amd import _capi
    d = head_data(name)
    arch, frames = d["arch"], d["frames"]
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


def assert_same(a, b, what):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_f16x3_graph_replay_and_batch_invariance(name):
    """graph replay equals eager, and frame i of the bs-2 call equals its bs-1 call, bit for bit: a block's GEMM rotation depends on its
    row tile inside its image only, at every tile count"""
    from telescope_cam_detection_amd import _capi
    d = head_data(name)
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", POST_FUSED_NAMES)
def test_f16x3_one_launch_post_processor_equals_three_launches(name):
    from telescope_cam_detection_amd import _capi
    d = head_data(name)
    frames, got = d["frames"], {}
    try:
        for fused in (0, 1):
            _capi.debug_option("post_fused", fused)
            eng = make_engine(d, "f16x3", use_graph=True)
            try:
                for _ in range(2):
                    got[fused] = eng.infer_raw(frames)
                assert plan_paths(eng, len(frames))[1] == (FUSED if fused else THREE)
            finally:
                eng.close()
    finally:
        _capi.debug_option("reset", 0)
    assert_same(got[0], got[1], "post_fused 0 vs 1")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_f16x3_side_stream_plan_equals_the_serial_plan(name):
    from telescope_cam_detection_amd import _capi
    d = head_data(name)
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


@pytest.mark.gpu
def test_more_queries_than_memory_tokens_is_refused_when_the_weights_load():
    """rtd_create cannot know S; rtd_load_weights does: Q = 1024 at 192 x 192 has 24^2 + 12^2 + 6^2 = 756 memory tokens"""
    from telescope_cam_detection_amd import _capi
    from telescope_cam_detection_amd.weights import fold_weights, pack_blob
    arch = BY_NAME["q1024"].arch
    blob = pack_blob(fold_weights(arch, weights_for(arch, 3)))
    try:
        with pytest.raises(_capi.RtdError, match="num_queries exceeds the number of memory tokens") as ei:
            _capi.Engine(arch, blob, device=0, precision=_capi.PREC_F16X3, max_batch=1, input_size=(192, 192), use_graph=False)
        assert ei.value.code == _capi.RTD_E_INVALID
    finally:
        _capi.debug_option("reset", 0)
