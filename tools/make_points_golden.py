"""Generate the fixtures of the r50vd_m and sp1 / sp2 / sp3 variants, tests/golden/p*.npz and m1*.npz, and tests/golden/points_yardstick.json
by running HuggingFace transformers' RT-DETRv2 with decoder_n_points = 1, 2, 3 (R18) and with hidden_expansion 0.5 on R50 on the CPU.

    python tools/make_points_golden.py            write the fixtures
    python tools/make_points_golden.py --check    recompute them and compare every array with the committed files, exactly
    python tools/make_points_golden.py --search   how the seeds of tests/variants_ref.py were found (prints candidates, writes nothing)

Modelled on tools/make_dsp_golden.py and, like it, reusing oracle/make_golden.py: its run_case() writes the file (same keys as the c* / t* /
d* fixtures) and asserts, before it does, that the restatement agrees with HF per selected token (1e-4 logits, 1e-5 boxes).  The model
builder is swapped in for the run: make_golden's build_hf takes no point count, so its config call is restated here with decoder_n_points.
Only data is stored.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg  # noqa: E402
from oracle import rtdetr_oracle as orc  # noqa: E402
from telescope_cam_detection_amd.arch import ARCHS  # noqa: E402
from telescope_cam_detection_amd.checkpoint import hf_key_map  # noqa: E402
from telescope_cam_detection_amd.synth import make_frame, noise_frame, scene_frame  # noqa: E402
from telescope_cam_detection_amd.weights import synth_weights  # noqa: E402
from tests import variants_ref as vr  # noqa: E402
from tests.util import match_detections  # noqa: E402


def build_hf_with_points(arch, w):
    """make_golden.build_hf with the decoder's point count, CSP width and layer count taken from the arch"""
    from transformers import RTDetrV2Config, RTDetrV2ForObjectDetection
    from transformers.models.rt_detr.configuration_rt_detr_resnet import RTDetrResNetConfig

    bb = RTDetrResNetConfig(depths=list(arch.depths), layer_type=arch.layer_type, hidden_sizes=list(arch.hidden_sizes),
                            embedding_size=arch.embedding_size, out_indices=[2, 3, 4])
    cfg = RTDetrV2Config(
        backbone_config=bb, encoder_in_channels=list(arch.backbone_out_channels), encoder_hidden_dim=arch.enc_dim,
        encoder_ffn_dim=arch.enc_ffn, encoder_attention_heads=arch.enc_heads, hidden_expansion=arch.expansion,
        d_model=arch.d_model, decoder_in_channels=[arch.enc_dim] * 3, decoder_ffn_dim=arch.dec_ffn,
        decoder_attention_heads=arch.dec_heads, decoder_layers=arch.dec_layers, num_queries=arch.num_queries,
        num_labels=arch.num_classes, anchor_image_size=None, eval_size=None, tie_word_embeddings=False,
        decoder_method=arch.dec_method, decoder_n_points=arch.n_points)
    cfg._attn_implementation = "eager"
    model = RTDetrV2ForObjectDetection(cfg).eval()
    km = hf_key_map(arch)
    missing, unexpected = model.load_state_dict({hf: w[mine] for mine, hf in km.items()}, strict=False)
    ok_missing = ("model.decoder.class_embed", "model.decoder.bbox_embed", "model.denoising_class_embed", "n_points_scale", "num_batches_tracked")
    bad = [k for k in missing if not any(s in k for s in ok_missing)]
    assert not bad and not unexpected and set(km) == set(w), (bad[:10], unexpected[:10])
    points = [tuple(m.n_points_list) for m in model.modules() if hasattr(m, "method") and hasattr(m, "n_points_list")]
    assert len(points) == arch.dec_layers and set(points) == {(arch.n_points,) * arch.n_levels}, points   # every cross-attention module
    assert len(model.model.decoder.layers) == arch.dec_layers
    return model


def write_case(name, out_dir):
    saved = mg.build_hf, mg.GOLDEN_DIR
    mg.CASES[name] = vr.POINTS_CASES[name]
    mg.build_hf, mg.GOLDEN_DIR = build_hf_with_points, out_dir
    try:
        mg.run_case(name)
    finally:
        mg.build_hf, mg.GOLDEN_DIR = saved
        del mg.CASES[name]


@torch.no_grad()
def yardstick_of(name, g):
    """what the tests may ask of an implementation on this case, measured on the restatement itself (the format of dsp_yardstick.json)"""
    arch_name, wseed, input_size, frames, kind = vr.POINTS_CASES[name]
    arch = ARCHS[arch_name]
    w = synth_weights(arch, wseed)
    xs, sizes = zip(*[orc.preprocess(make_frame(kind, fs, fh, fw), input_size) for fs, fh, fw in frames])
    x, sizes = torch.cat(xs, 0), list(sizes)
    col, col64 = {}, {}
    l32, b32, s32 = orc.model_forward(arch, w, x, sizes, collect=col)
    # the same restatement in fp64, on the fp32 run's selection (a near-tie at the rank-Q cut must not count as decoder error)
    w64 = {k: v.double() for k, v in w.items()}
    l64, b64, s64 = orc.model_forward(arch, w64, x.double(), sizes, collect=col64, force_topk=col["topk"])
    so, sh = torch.sort(col["topk"], 1), torch.sort(torch.as_tensor(g["topk"]).long(), 1)
    assert torch.equal(so.values, sh.values), name
    gat = lambda t, idx: t.gather(1, idx.unsqueeze(-1).expand(-1, -1, t.shape[-1]))
    d_logit = (gat(col["logits"], so.indices) - gat(torch.as_tensor(g["logits"]), sh.indices)).abs().max().item()
    d_box = (gat(col["pred_boxes"], so.indices) - gat(torch.as_tensor(g["pred_boxes"]), sh.indices)).abs().max().item()
    rows_off = []
    for i in range(len(frames)):
        m, n, _, _ = match_detections(l64[i].numpy(), b64[i].numpy(), s64[i].numpy(), l32[i].numpy(), b32[i].numpy(), s32[i].numpy(), 1e-3, 1e-2)
        rows_off.append(n - m)
    return {
        "hf_vs_restatement": {"max_abs_dlogit": d_logit, "max_abs_dbox": d_box},
        "fp32_vs_fp64_rows_outside_1e-3_1e-2px": rows_off,          # per frame, of the restatement against its fp64 self
    }


def search(argv):
    """candidates for the seeds of tests/variants_ref.py: the first (weight seed, frame seeds) of a fixed walk that meet
    variants_ref.well_posed - nothing else is looked at"""
    from tests.util import weights_for
    names = [a for a in argv if not a.startswith("--")] or list(vr.POINTS_CASES) + list(vr.ENGINE_CASES)
    for name in names:
        found = None
        for wseed in range(0, 6):
            for k in range(0, 6):
                if name in vr.POINTS_CASES:
                    arch_name, _, input_size, frames, kind = vr.POINTS_CASES[name]
                    arch = ARCHS[arch_name]
                    fr = [(6100 + 2 * k, 160, 224), (6101 + 2 * k, 200, 150)]
                    d = vr.oracle_runs(name, arch, weights_for(arch, wseed), [make_frame(kind, *f) for f in fr], input_size)
                    seeds = (wseed, fr)
                else:
                    arch = vr.ENGINE_CASES[name][0]
                    s, n = 5 + 2 * k, 6 + 2 * k
                    d = vr.oracle_runs(name, arch, weights_for(arch, wseed), [scene_frame(s, *vr.SIZE), noise_frame(n, *vr.SIZE)], vr.SIZE)
                    seeds = (wseed, s, n)
                ok, bad = vr.well_posed(d, verbose=False)
                print(f"[search] {name} seeds {seeds}: {'well posed' if ok else '; '.join(bad)}", flush=True)
                if ok:
                    found = seeds
                    break
            if found:
                break
        print(f"[search] {name}: {found}", flush=True)


def main(argv):
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    if "--search" in argv:
        return search(argv)
    check = "--check" in argv
    names = [a for a in argv if not a.startswith("--")] or list(vr.POINTS_CASES)
    out_dir = tempfile.mkdtemp() if check else mg.GOLDEN_DIR
    ys = {}
    for name in names:
        write_case(name, out_dir)
        g = np.load(os.path.join(out_dir, name + ".npz"))
        if check:
            ref = np.load(os.path.join(mg.GOLDEN_DIR, name + ".npz"))
            assert sorted(g.files) == sorted(ref.files), name
            for k in g.files:
                assert np.array_equal(g[k], ref[k]), (name, k)
            print(f"[{name}] {len(g.files)} arrays equal the committed file")
        ys[name] = yardstick_of(name, g)
        print(f"[{name}] {json.dumps(ys[name])}")
    path = os.path.join(mg.GOLDEN_DIR, vr.YARDSTICK)
    if check:
        with open(path) as fh:
            committed = json.load(fh)
        for name in names:
            assert committed[name] == ys[name], (name, committed[name], ys[name])
        print("yardstick equals the committed file")
    else:
        if os.path.exists(path) and set(names) != set(vr.POINTS_CASES):
            with open(path) as fh:
                ys = {**json.load(fh), **ys}
        with open(path, "w") as fh:
            json.dump(ys, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
