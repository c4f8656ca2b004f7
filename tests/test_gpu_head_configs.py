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
from dataclasses import dataclass, replace

import pytest

from oracle import rtdetr_oracle as orc
from telescope_cam_detection_amd.arch import ARCHS
from telescope_cam_detection_amd.synth import noise_frame, scene_frame
from tests.engine_checks import (FUSED, PER_OP, THREE, assert_same, check_f16x3_stages, check_fused_decoder_equals_per_op,
                                 check_graph_replay_and_batch_invariance, check_side_stream_equals_serial, make_engine, oracle64_refs, plan_paths)
from tests.util import error_figures, reference_runs, threads, weights_for, well_posed

SIZE = (320, 320)


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


def head_data(name):
    """a case's frames and its fp64 and fp32 oracle runs"""
    case = BY_NAME[name]
    arch, (wseed, sseed, nseed) = case.arch, case.seeds
    d = reference_runs(name, arch, weights_for(arch, wseed), [scene_frame(sseed, *SIZE), noise_frame(nseed, *SIZE)], SIZE)
    d["case"] = case
    return d


def forced32(d):
    """the fp32 oracle under the fp64 oracle's selection, in its query order: row for row the e_ref of the chain ratios"""
    if "forced32" not in d:
        threads()
        col = {}
        orc.model_forward(d["arch"], d["w"], d["x"], d["sizes"], collect=col, force_topk=d["col"]["topk"].numpy())
        d["forced32"] = col
    return d["forced32"]


# ------------------------------------------------------------------------------------------ CPU: the data is well posed
@pytest.mark.parametrize("name", NAMES)
def test_reference_is_well_posed(name):
    ok, reasons = well_posed(head_data(name))
    assert ok, (name, reasons)


def test_case_table_covers_the_paths_it_names():
    """bookkeeping of the table only (the engine's path is asserted on the GPU, assert_paths): each path of each part has a case"""
    assert {c.decoder for c in CASES} == {FUSED, PER_OP} and {c.post for c in CASES} == {FUSED, THREE} and {c.aifi for c in CASES} == {FUSED, PER_OP}


# ------------------------------------------------------------------------------------------ GPU
def assert_paths(eng, d):
    case = d["case"]
    got = plan_paths(eng, len(d["frames"]))
    print(f"{case.name}: decoder {got[0]}, post-processor {got[1]}, AIFI {got[2]}")
    assert got == (case.decoder, case.post, case.aifi), (case.name, got)


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
    from tests.test_gpu_parity import x3_check
    d = head_data(name)
    col, frames = d["col"], d["frames"]
    eng = make_engine(d, "f16x3")
    try:
        check_f16x3_stages(eng, d)
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
    check_fused_decoder_equals_per_op(head_data(name), precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_f16x3_graph_replay_and_batch_invariance(name):
    """graph replay equals eager, and frame i of the bs-2 call equals its bs-1 call, bit for bit: a block's GEMM rotation depends on its
    row tile inside its image only, at every tile count"""
    check_graph_replay_and_batch_invariance(head_data(name))


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
    check_side_stream_equals_serial(head_data(name))


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
