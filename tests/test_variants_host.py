"""CPU: the r50vd_m and sp1 / sp2 / sp3 variants without a GPU - what selects them (config path and YAML -> Arch, checkpoint shapes -> Arch),
the oracle against the HF fixtures oracle/make_golden.py wrote, and that the data of every GPU case of tests/test_gpu_variants.py
is well posed before an engine is judged on it (tests.util.well_posed)."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import rtdetr_oracle as orc
from telescope_cam_detection_amd import _capi
from telescope_cam_detection_amd import checkpoint as ck
from telescope_cam_detection_amd.arch import ARCHS, UnsupportedVariant, arch_from_config_path
from telescope_cam_detection_amd.weights import synth_weights
from tests import variants_ref as vr
from tests.util import match_detections, sample, weights_for, well_posed

UPSTREAM = "RT-DETR/rtdetrv2_pytorch/configs/rtdetrv2/"
NEW_ARCHS = ["r50_m", "r50_m_dsp", "r18_sp1", "r18_sp2", "r18_sp3"]
OLD_ARCHS = [n for n in ARCHS if n not in NEW_ARCHS]


# ------------------------------------------------------------------------------------------ arch table
def test_new_entries_come_after_every_existing_one_and_differ_as_upstream_says():
    names = list(ARCHS)
    assert names[-len(NEW_ARCHS):] == NEW_ARCHS and OLD_ARCHS == ["r18", "r34", "r50", "r101", "tiny", "tinyb", "tinyc", "r18_dsp", "r34_dsp",
                                                                   "r50_dsp", "r101_dsp", "tinyc_dsp"]
    assert dataclasses.replace(ARCHS["r50_m"], name="r50", expansion=1.0, dec_layers=6) == ARCHS["r50"]
    assert ARCHS["r50_m"].csp_hidden == 128 and ARCHS["r50_m"].dec_layers == 3
    assert dataclasses.replace(ARCHS["r50_m_dsp"], name="r50_m", dec_method="default") == ARCHS["r50_m"]
    for k in (1, 2, 3):
        assert dataclasses.replace(ARCHS[f"r18_sp{k}"], name="r18", n_points=4) == ARCHS["r18"]
        assert _capi.cfg_for(ARCHS[f"r18_sp{k}"]).n_points == k
    assert [n for n in ARCHS if ARCHS[n].n_points != 4] == ["r18_sp1", "r18_sp2", "r18_sp3"]      # no sp twin of another backbone, no sp + dsp


# ------------------------------------------------------------------------------------------ names
@pytest.mark.parametrize("fname,want", [
    ("rtdetrv2_r50vd_m_7x_coco.yml", "r50_m"), ("rtdetrv2_r50vd_m_dsp_3x_coco.yml", "r50_m_dsp"),
    ("rtdetrv2_r18vd_sp1_120e_coco.yml", "r18_sp1"), ("rtdetrv2_r18vd_sp2_120e_coco.yml", "r18_sp2"), ("rtdetrv2_r18vd_sp3_120e_coco.yml", "r18_sp3"),
    ("rtdetrv2_r18vd_sp4_120e_coco.yml", "r18"),              # four points are the base model
    ("rtdetrv2_r50vd_medium_coco.yml", "r50"), ("rtdetrv2_r18vd_sp2x_coco.yml", "r18"), ("rtdetrv2_r18vd_wasp2_coco.yml", "r18"),   # whole tokens only
    # every row of the two existing tables (tests/test_host_logic.py, tests/test_dsp_oracle.py)
    ("rtdetrv2_r18vd_120e_coco.yml", "r18"), ("rtdetrv2_r50vd_6x_coco.yml", "r50"), ("rtdetrv2_r101vd_6x_coco.yml", "r101"),
    ("rtdetrv2_r18vd_dsp_3x_coco.yml", "r18_dsp"), ("rtdetrv2_r34vd_dsp_1x_coco.yml", "r34_dsp"), ("rtdetrv2_r34vd_120e_coco.yml", "r34"),
    ("rtdetrv2_r50vd_dsp_1x_coco.yml", "r50_dsp"), ("rtdetrv2_r101vd_dsp_1x_coco.yml", "r101_dsp"),
    ("rtdetrv2_r18vd_dspace_120e_coco.yml", "r18"), ("rtdetrv2_r50vd_mdsp_coco.yml", "r50"),
    ("rtdetrv2_tinyc_dsp.yml", "tinyc_dsp"), ("rtdetrv2_tinyc.yml", "tinyc"), ("rtdetrv2_tinyb_dsp.yml", "tinyb"),
])
def test_config_path_selects_the_variant_by_file_name(fname, want):
    a = arch_from_config_path(UPSTREAM + fname)
    assert a.name == want and a is ARCHS[want]


def test_existing_short_paths_resolve_as_before():
    assert arch_from_config_path("configs/rtdetrv2/rtdetrv2_r50vd_6x_coco.yml") is ARCHS["r50"]
    assert arch_from_config_path("configs/rtdetrv2/rtdetrv2_r101vd_6x_coco.yml") is ARCHS["r101"]
    with pytest.raises(ValueError):
        arch_from_config_path("yolox_s.py")
    with pytest.raises(ValueError):
        arch_from_config_path("yolox_s_dsp.py")


@pytest.mark.parametrize("fname,word", [
    ("rtdetrv2_r34vd_sp2_120e_coco.yml", "sp"), ("rtdetrv2_r50vd_sp1_coco.yml", "sp"), ("rtdetrv2_r101vd_sp3_coco.yml", "sp"),
    ("rtdetrv2_r50vd_m_sp2_coco.yml", "sp"), ("rtdetrv2_r18vd_sp5_coco.yml", "5"), ("rtdetrv2_r18vd_sp2_dsp_coco.yml", "discrete"),
    ("rtdetrv2_r18vd_m_120e_coco.yml", "`m`"), ("rtdetrv2_r34vd_m_dsp_coco.yml", "`m`"), ("rtdetrv2_r101vd_m_coco.yml", "`m`"),
])
def test_markers_on_a_backbone_without_such_a_model_are_refused(fname, word):
    with pytest.raises(ValueError, match=word) as ei:
        arch_from_config_path(UPSTREAM + fname)
    assert isinstance(ei.value, UnsupportedVariant)           # a refusal: the detector does not fall back to the checkpoint's shapes


HEAD = "__include__: [\n  '../dataset/coco_detection.yml',\n]\n\nPResNet:\n  depth: 18\n\nRTDETRTransformerv2:\n  num_layers: 3\n"


@pytest.mark.parametrize("k", [1, 2, 3])
def test_yaml_num_points_selects_the_sp_entry(tmp_path, k):
    p = tmp_path / "rtdetrv2_r18vd_custom.yml"
    p.write_text(HEAD + f"  num_points: [{k}, {k}, {k}]\n")
    assert arch_from_config_path(str(p)) is ARCHS[f"r18_sp{k}"]
    p50 = tmp_path / "rtdetrv2_r50vd_custom.yml"
    p50.write_text(HEAD + f"  num_points: [{k}, {k}, {k}]   # fewer points\n")
    with pytest.raises(UnsupportedVariant):
        arch_from_config_path(str(p50))


def test_yaml_num_points_beats_the_file_name_and_comments_do_not_count(tmp_path):
    base = tmp_path / "rtdetrv2_r18vd_sp2_120e_coco.yml"
    base.write_text(HEAD + "  num_points: [4, 4, 4]\n")
    assert arch_from_config_path(str(base)) is ARCHS["r18"]
    four = tmp_path / "rtdetrv2_r50vd_m_custom.yml"
    four.write_text(HEAD + "  num_points: [4,4,4]\n")
    assert arch_from_config_path(str(four)) is ARCHS["r50_m"]
    commented = tmp_path / "rtdetrv2_r18vd_custom3.yml"
    commented.write_text(HEAD + "  # num_points: [2, 2, 2]\n")
    assert arch_from_config_path(str(commented)) is ARCHS["r18"]
    commented2 = tmp_path / "rtdetrv2_r18vd_sp3_custom.yml"
    commented2.write_text(HEAD + "  #num_points: [2, 2, 2]\n")
    assert arch_from_config_path(str(commented2)) is ARCHS["r18_sp3"]       # the name decides where the YAML says nothing
    both = tmp_path / "rtdetrv2_r18vd_custom4.yml"
    both.write_text(HEAD + "  num_points: [2, 2, 2]\n  cross_attn_method: discrete\n")
    with pytest.raises(UnsupportedVariant, match="discrete"):
        arch_from_config_path(str(both))


@pytest.mark.parametrize("lst", ["[4, 2, 1]", "[3, 6, 3]", "[2, 2, 3]"])
def test_yaml_with_per_level_point_counts_is_refused_and_names_the_list(tmp_path, lst):
    p = tmp_path / "rtdetrv2_r18vd_custom.yml"
    p.write_text(HEAD + f"  num_points: {lst}\n")
    with pytest.raises(UnsupportedVariant) as ei:
        arch_from_config_path(str(p))
    assert lst.strip("[]") in str(ei.value)


def test_detector_refuses_an_unsupported_config_instead_of_serving_the_files_shapes(tmp_path):
    """[3, 6, 3] has the sampling-head shapes of [4, 4, 4]: the checkpoint cannot tell, so the config's refusal must reach the caller"""
    from telescope_cam_detection_amd.rtdetr_detector import RTDETRDetector
    p = tmp_path / "rtdetrv2_r18vd_custom.yml"
    p.write_text(HEAD + "  num_points: [3, 6, 3]\n")
    det = RTDETRDetector(config_path=str(p), model_path=str(tmp_path / "absent.pth"))
    with pytest.raises(UnsupportedVariant):
        det._blob()


# ------------------------------------------------------------------------------------------ checkpoints
def upstream_state(arch, w, prefix="module."):
    """the state dict as upstream's training script saves it (tests/test_checkpoint.py)"""
    up, fused = {}, {}
    for mine, key in ck.upstream_key_map(arch).items():
        if "#" in key:
            base, part = key.split("#")
            fused.setdefault(base, {})[part] = w[mine]
        else:
            up[prefix + key] = w[mine]
    for base, parts in fused.items():
        up[prefix + base] = torch.cat([parts["q"], parts["k"], parts["v"]], 0)
    return up


def layouts(arch, w):
    return {"upstream": upstream_state(arch, w), "hf": {hf: w[mine] for mine, hf in ck.hf_key_map(arch).items()}, "native": dict(w)}


@pytest.mark.parametrize("name", ["r18_sp1", "r18_sp2", "r18_sp3", "r50_m"])
def test_guess_arch_names_the_new_variants_in_every_layout(name):
    arch = ARCHS[name]
    w = weights_for(arch, 1)
    heads = arch.dec_heads * arch.n_levels * arch.n_points
    assert tuple(w["dec.l0.ca.off.w"].shape) == (heads * 2, 256) and tuple(w["dec.l0.ca.aw.w"].shape) == (heads, 256)
    for layout, state in layouts(arch, w).items():
        assert ck.sniff_layout(state) == layout
        assert ck.guess_arch(state, layout) == name, layout


@pytest.mark.parametrize("name", OLD_ARCHS)
def test_existing_archs_are_still_guessed_as_before(name):
    """the first fit, recorded as it was before the new entries: a dsp twin's file is its plain entry's (the shapes cannot tell the
    sampler), and an r34 file is r18's - every tensor r18 maps exists in an r34 file with r18's shape (blocks 0..1 of 0..2/3/5, decoder
    layers 0..2 of 0..3), the converters pick only the keys they map, and r18 comes first.  That answer is not right, and it is not this
    table's to change: nothing appended after the existing entries may alter it."""
    arch = ARCHS[name]
    w = weights_for(arch, 1)
    want = {"r34": "r18", "r34_dsp": "r18"}.get(name, name[:-len("_dsp")] if name.endswith("_dsp") else name)
    for layout, state in layouts(arch, w).items():
        assert ck.guess_arch(state, layout) == want, layout


def six_layer_upstream_state(seed):
    """an upstream-layout r50_m state as upstream's file stores it: 6 trained decoder layers with their 6 heads (eval_idx 2 reads 0..2).
    Returns (state, the 3-layer weights that must come out)."""
    arch = ARCHS["r50_m"]
    w = synth_weights(arch, seed)
    six = dataclasses.replace(arch, dec_layers=6)
    w6 = synth_weights(six, seed + 1)
    extra = {k: v for k, v in w6.items() if k.startswith(("dec.l3.", "dec.l4.", "dec.l5.", "dec.bbox.3.", "dec.bbox.4.", "dec.bbox.5.", "dec.cls.3.",
                                                          "dec.cls.4.", "dec.cls.5."))}
    assert len(extra) == 3 * len([k for k in w if k.startswith(("dec.l0.", "dec.bbox.0.", "dec.cls.0."))])
    return upstream_state(six, {**w, **extra}), w


def test_r50_m_file_with_six_stored_decoder_layers_converts_to_the_three_that_run():
    state, w = six_layer_upstream_state(4)
    assert any(k.startswith("module.decoder.decoder.layers.5.") for k in state) and "module.decoder.dec_score_head.5.weight" in state
    assert ck.guess_arch(state, "upstream") == "r50_m"
    got = ck.convert_upstream_state(state, ARCHS["r50_m"])
    assert set(got) == set(w) and all(torch.equal(got[k], w[k]) for k in w)
    assert not [k for k in got if k.startswith(("dec.l3", "dec.bbox.3", "dec.cls.3"))]
    # the HF converter picks its keys the same way
    six = dataclasses.replace(ARCHS["r50_m"], dec_layers=6)
    w6 = {**synth_weights(six, 5), **w}
    got = ck.convert_hf_state({hf: w6[mine] for mine, hf in ck.hf_key_map(six).items()}, ARCHS["r50_m"])
    assert set(got) == set(w) and all(torch.equal(got[k], w[k]) for k in w)


def test_synthetic_model_paths_name_the_new_variants():
    from telescope_cam_detection_amd.rtdetr_detector import load_state
    for name in ("r18_sp2", "r50_m"):
        state, got = load_state(f"synthetic:{name}:2")
        assert got == name and all(torch.equal(state[k], v) for k, v in synth_weights(ARCHS[name], 2).items())


# ------------------------------------------------------------------------------------------ oracle against the HF fixtures
@pytest.mark.parametrize("name", vr.POINTS_CASES)
def test_oracle_matches_the_hf_fixture(name):
    """tests/test_oracle_golden.py's test_oracle_matches_golden on the new files, same bounds"""
    d = vr.fixture_data(name)
    g, col, x = d["g"], d["col32"], d["x"]
    labels, boxes, scores = d["out32"]
    assert d["arch"].n_points == {"p1": 1, "p2": 2, "p3": 3, "m1": 4}[name[:2]]
    assert sum(h * w for h, w in d["arch"].level_shapes(*d["input_size"])) == 735 and [f.shape[:2] for f in d["frames"]] == [(160, 224), (200, 150)]
    np.testing.assert_allclose(sample(x), g["input_sample"], atol=0, rtol=0)
    for i in range(3):
        for key in (f"backbone{i}", f"enc{i}"):
            want = g["s_" + key]
            np.testing.assert_allclose(sample(col[key]), want, atol=max(2e-4, 5e-6 * float(np.abs(want).max())), rtol=1e-4)
    np.testing.assert_allclose(col["enc_cls_max"].numpy(), g["enc_cls_max"], atol=1e-4)
    mine, gold = np.sort(col["topk"].numpy(), 1), np.sort(g["topk"], 1)
    assert np.array_equal(mine, gold)
    om, og = np.argsort(col["topk"].numpy(), 1), np.argsort(g["topk"], 1)
    for b in range(len(d["frames"])):
        np.testing.assert_allclose(col["logits"][b].numpy()[om[b]], g["logits"][b][og[b]], atol=1e-4)
        np.testing.assert_allclose(col["pred_boxes"][b].numpy()[om[b]], g["pred_boxes"][b][og[b]], atol=1e-5)
        m, n, ws, wb = match_detections(g["labels"][b], g["boxes"][b], g["scores"][b], labels[b], boxes[b], scores[b], 1e-3, 1e-2)
        assert m == n, (m, n, ws, wb)
    assert f"s_dec{d['arch'].dec_layers - 1}.hs" in g.files and f"s_dec{d['arch'].dec_layers}.hs" not in g.files


def test_yardstick_leaves_no_allowance():
    y = vr.yardstick()
    assert set(y) == set(vr.POINTS_CASES)
    for name, rec in y.items():
        assert rec["fp32_vs_fp64_rows_outside_1e-3_1e-2px"] == [0, 0], name
        assert rec["hf_vs_restatement"]["max_abs_dlogit"] <= 1e-4 and rec["hf_vs_restatement"]["max_abs_dbox"] <= 1e-5, name


def test_the_point_count_shows_in_the_fixtures():
    """the fixtures tell the variants apart: the 4-point oracle cannot even load an sp checkpoint, and sp2 weights run at another count of
    the same head width do not exist - so compare the sp fixtures' rows with each other: same trunk seeds, other decoder, other rows"""
    a, b = vr.fixture_data("p2_r18sp2_160x224")["g"], vr.fixture_data("p3_r18sp3_160x224")["g"]
    assert np.abs(a["scores"] - b["scores"]).max() > 1e-2


# ------------------------------------------------------------------------------------------ the GPU cases' data
@pytest.mark.parametrize("name", list(vr.ENGINE_CASES))
def test_engine_case_is_well_posed(name):
    d = vr.engine_data(name)
    assert sum(h * w for h, w in d["arch"].level_shapes(*vr.SIZE)) == 2100 and d["arch"].num_queries == 300 == 18 * 16 + 12
    ok, bad = well_posed(d)
    assert ok, bad


@pytest.mark.parametrize("name", vr.POINTS_CASES)
def test_fixture_case_is_well_posed(name):
    ok, bad = well_posed(vr.fixture_data(name))
    assert ok, bad
