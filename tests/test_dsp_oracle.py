"""CPU: the discrete-sampling ("dsp") variants without a GPU - the oracle against the HF fixtures oracle/make_golden.py wrote, under
the arch's own sampler and under the bilinear one ("patched" / "unpatched" in the test names: the oracle once had to be patched to sample
discretely), what selects the sampler (config path -> Arch -> rtd_config), the new test entry point's declaration, and the inputs of the
kernel-level GPU test: which items the comparison leaves out, and that the fp32 restatement picks the fp64 taps on all others."""
import dataclasses
import os
import re

import pytest
import torch

from telescope_cam_detection_amd import _capi
from telescope_cam_detection_amd.arch import ARCHS, arch_from_config_path
from tests import dsp_ref
from tests.dsp_ref import MSD_CASES, MSD_DELTA, discrete_taps, msd_inputs, msdeform_discrete_ref, near_boundary_items
from tests.util import load_case, oracle_run, weights_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSP_CASES = ["d1_r18dsp_160x224", "d2_tinycdsp_160x224"]


def per_token_deltas(name, discrete):
    """max |dlogit|, max |dbox| between the oracle (with the case's own Arch when `discrete`, else with its bilinear twin) and the HF
    fixture, per selected token: query ORDER is decided by near-ties of the encoder scores (oracle/make_golden.py)"""
    arch, wseed, input_size, frames, g = load_case(name)
    assert arch.dec_method == "discrete"
    w = weights_for(arch, wseed)
    if not discrete:
        arch = dataclasses.replace(arch, dec_method="default")
    _, col = oracle_run(arch, w, frames, input_size)
    so, sh = torch.sort(col["topk"], 1), torch.sort(torch.as_tensor(g["topk"]).long(), 1)
    assert torch.equal(so.values, sh.values)
    gat = lambda t, idx: t.gather(1, idx.unsqueeze(-1).expand(-1, -1, t.shape[-1]))
    d_logit = (gat(col["logits"], so.indices) - gat(torch.as_tensor(g["logits"]), sh.indices)).abs().max().item()
    d_box = (gat(col["pred_boxes"], so.indices) - gat(torch.as_tensor(g["pred_boxes"]), sh.indices)).abs().max().item()
    print(f"[{name}] {'discrete' if discrete else 'bilinear'} oracle vs HF fixture: max|dlogit| {d_logit:.3e}, max|dbox| {d_box:.3e}")
    return d_logit, d_box


@pytest.mark.parametrize("name", DSP_CASES)
def test_patched_oracle_meets_the_hf_fixture(name):
    """the gates oracle/make_golden.py asserts before it writes a fixture"""
    d_logit, d_box = per_token_deltas(name, True)
    assert d_logit <= 1e-4 and d_box <= 1e-5


@pytest.mark.parametrize("name", DSP_CASES)
def test_unpatched_oracle_misses_the_hf_fixture(name):
    """the fixture tells the two samplers apart"""
    d_logit, _ = per_token_deltas(name, False)
    assert d_logit > 1e-2


def test_fixtures_have_the_shapes_the_gpu_tests_rely_on():
    arch, _, input_size, frames, g = load_case("d1_r18dsp_160x224")
    assert arch.d_model == 256 and arch.dec_heads == 8 and (arch.n_levels, arch.n_points) == (3, 4)      # the fused decoder kernel's shape
    assert sum(h * w for h, w in arch.level_shapes(*input_size)) == 735 >= arch.num_queries == 300
    assert [f.shape[:2] for f in frames] == [(160, 224), (200, 150)]
    arch2, _, _, _, _ = load_case("d2_tinycdsp_160x224")
    assert arch2.d_model != 256                                                                          # the per-op decoder
    y = dsp_ref.yardstick()
    for name in DSP_CASES:
        assert y[name]["hf_vs_restatement"]["max_abs_dlogit"] <= 1e-4 and y[name]["default_vs_discrete_max_abs_dlogit"] > 1e-2
        assert len(y[name]["fp32_vs_fp64_rows_outside_1e-3_1e-2px"]) == 2


UPSTREAM = "RT-DETR/rtdetrv2_pytorch/configs/rtdetrv2/"


@pytest.mark.parametrize("fname,want", [
    ("rtdetrv2_r18vd_dsp_3x_coco.yml", "r18_dsp"), ("rtdetrv2_r18vd_120e_coco.yml", "r18"),
    ("rtdetrv2_r34vd_dsp_1x_coco.yml", "r34_dsp"), ("rtdetrv2_r34vd_120e_coco.yml", "r34"),
    ("rtdetrv2_r50vd_dsp_1x_coco.yml", "r50_dsp"), ("rtdetrv2_r50vd_6x_coco.yml", "r50"),
    ("rtdetrv2_r101vd_dsp_1x_coco.yml", "r101_dsp"), ("rtdetrv2_r101vd_6x_coco.yml", "r101"),
    ("rtdetrv2_r18vd_dspace_120e_coco.yml", "r18"),          # `dsp` only inside another word
    ("rtdetrv2_r50vd_mdsp_coco.yml", "r50"),
    ("rtdetrv2_tinyc_dsp.yml", "tinyc_dsp"), ("rtdetrv2_tinyc.yml", "tinyc"),
    ("rtdetrv2_tinyb_dsp.yml", "tinyb"),                     # no dsp entry: the default architecture, as before
])
def test_config_path_selects_the_sampler_by_file_name(fname, want):
    a = arch_from_config_path(UPSTREAM + fname)
    assert a.name == want and a is ARCHS[want]
    assert a.dec_method == ("discrete" if want.endswith("_dsp") else "default")


def test_config_path_selects_the_sampler_by_the_yaml_key(tmp_path):
    head = "__include__: [\n  '../dataset/coco_detection.yml',\n]\n\nPResNet:\n  depth: 18\n\nRTDETRTransformerv2:\n  num_layers: 3\n"
    plain = tmp_path / "rtdetrv2_r18vd_custom.yml"
    plain.write_text(head)
    assert arch_from_config_path(str(plain)).name == "r18"
    disc = tmp_path / "rtdetrv2_r18vd_custom2.yml"
    disc.write_text(head + "  cross_attn_method: discrete\n")
    assert arch_from_config_path(str(disc)).name == "r18_dsp"
    commented = tmp_path / "rtdetrv2_r18vd_custom3.yml"
    commented.write_text(head + "  # cross_attn_method: discrete\n  cross_attn_method: default\n")
    assert arch_from_config_path(str(commented)).name == "r18"
    with pytest.raises(ValueError):
        arch_from_config_path("yolox_s_dsp.py")


def test_dsp_entries_differ_from_their_twins_in_name_and_sampler_only():
    for n in ("r18", "r34", "r50", "r101", "tinyc"):
        assert dataclasses.replace(ARCHS[n + "_dsp"], name=n, dec_method="default") == ARCHS[n]
        assert ARCHS[n].dec_method == "default"


def test_config_struct_carries_the_method_and_create_checks_it():
    assert _capi.cfg_for(ARCHS["r18_dsp"]).dec_method == 1 and _capi.cfg_for(ARCHS["r18"]).dec_method == 0
    lib = _capi.lib()
    import ctypes as C
    h = C.c_void_p()
    cfg = _capi.cfg_for(ARCHS["r18_dsp"], precision=_capi.PREC_F16X3, max_batch=8, use_graph=True)
    assert lib.rtd_create(C.byref(cfg), C.byref(h)) == _capi.RTD_OK          # (allocates nothing on the device)
    lib.rtd_destroy(h)
    cfg.dec_method = 2
    assert lib.rtd_create(C.byref(cfg), C.byref(h)) == _capi.RTD_E_INVALID and b"dec_method" in lib.rtd_last_error(None)
    cfg = _capi.cfg_for(ARCHS["r18_dsp"], precision=_capi.PREC_BF16, max_batch=8, use_graph=True)
    assert lib.rtd_create(C.byref(cfg), C.byref(h)) == _capi.RTD_E_INVALID
    msg = lib.rtd_last_error(None)
    assert b"bf16" in msg and b"discrete" in msg


def test_new_entry_point_is_declared_exported_and_built():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtdetr_mi355_test.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtd_[a-z0-9_]+)\s*\(", code))
    sym = "rtd_op_msdeform_discrete_view"
    assert sym in declared and sym in _capi.TEST_EXPORTS and sym not in _capi.EXPORTS and hasattr(_capi.lib(), sym)
    assert declared == set(_capi.TEST_EXPORTS)
    assert "RTD_DEC_DISCRETE = 1" in open(os.path.join(ROOT, "include", "rtdetr_mi355.h")).read()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", MSD_CASES)
def test_kernel_test_inputs_leave_few_items_out_and_fp32_picks_the_fp64_taps(case, dt):
    """delta = 1e-4 px: 24 coordinates per item x 2e-4 = 0.5 % of the items expected; the fp32 error of a coordinate at |c| <= 32 is a
    few ulps of 4e-6, far inside delta.  2 % is a cap on what may be left out, not a measurement."""
    B, Q, heads, shapes, n_points, _ = case
    value, _, offaw, ref = msd_inputs(case, dt)
    _, c64 = msdeform_discrete_ref(value, offaw, ref, heads, 32, shapes, n_points, 0.5, torch.float64)
    _, c32 = msdeform_discrete_ref(value, offaw, ref, heads, 32, shapes, n_points, 0.5, torch.float32)
    near = near_boundary_items(c64, shapes, MSD_DELTA)
    print(f"{case} {dt}: {int(near.sum())} of {near.numel()} items left out")
    assert near.sum().item() <= 0.02 * near.numel()
    same = (discrete_taps(c64, shapes, n_points) == discrete_taps(c32, shapes, n_points)).all(-1)
    assert same[~near].all()
    # the exact-boundary grid is kept, and it does sit on boundaries: integer and half-integer coordinates, equal in both precisions
    npts = min(len(dsp_ref.boundary_locations(shapes)), Q - 8)
    assert not near[:, :npts].any()
    grid = c64[:, :npts]
    assert torch.equal(grid, c32[:, :npts].double()) and (grid == torch.round(grid)).any() and ((grid * 2) % 2 == 1).any()
    lo, hi = grid.min().item(), grid.max().item()
    assert lo <= -1.0 and hi >= max(max(s) for s in shapes)                  # both clamps are exercised


def test_rounding_order_inputs_tell_op_by_op_from_fused():
    """the inputs of the GPU test that pins the ROUNDING ORDER of the tap coordinate: on every query the fp32 restatement (torch, op by
    op, as HF computes it) picks the tap the op-by-op emulation predicts, and one fused multiply-add picks its neighbour"""
    value, offaw, ref, want_op, want_fused = dsp_ref.rounding_order_inputs()
    assert len(want_op) >= 12                                               # (18 of the 78 tap boundaries of the three maps)
    out32, _ = msdeform_discrete_ref(value, offaw, ref, 1, 32, dsp_ref.ROUNDING_SHAPES, dsp_ref.ROUNDING_POINTS, dsp_ref.ROUNDING_OFFSET_SCALE,
                                     torch.float32)
    assert (out32[0, :, :3] - want_op).abs().max().item() < 1e-6
    assert ((want_op - want_fused).abs().max(1).values == 1.0).all()
    assert {int(l) for l in want_op[:, 2]} >= {0, 1}                        # more than one map size
