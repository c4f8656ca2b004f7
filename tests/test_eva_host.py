"""Host side of the EVA02 classifier: the restatement against its own fp64 run and the recorded yardstick, the RoPE table against a
literal loop, the checkpoint converter (both qkv forms, both fc1 forms, both pools, the folds and pads, the refusals), the blob cache,
rtd_eva_create's refusals before any HIP call, and install() on a stand-in SpeciesClassifier.  No GPU."""
import ctypes as C
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import eva_ref as ref
from tests.standins import StandInSpeciesClassifier
from telescope_cam_detection_amd import _capi, classifier
from telescope_cam_detection_amd import eva_checkpoint as ck
from telescope_cam_detection_amd.weights import unpack_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARD = json.load(open(os.path.join(ROOT, "tests", "golden", "eva_yardstick.json")))


# ------------------------------------------------------------------------------------------------------------ restatement + yardstick
@pytest.mark.parametrize("name", list(ref.CASES))
def test_fp32_restatement_agrees_with_fp64_within_the_yardstick_and_the_seed_conditions_hold(name):
    y = YARD["cases"][name]
    assert y["weight_seed"] == YARD["weight_seed"][y["arch"]] and YARD["init_rule"] == ref.INIT_RULE
    rec = ref.measure_case(name, y["weight_seed"])
    arch, sd, _ = ref.case_inputs(name, y["weight_seed"])
    for n in map(str, ref.BATCHES):
        r, w = rec[n], y["n"][n]
        # another CPU's BLAS sums in another order: the fp32 error is a draw from the same spread, held to 2 x the recorded one
        assert r["fp32_logits_err"] <= 2 * w["fp32_logits_err"], (n, r["fp32_logits_err"], w["fp32_logits_err"])
        for st, e in r["fp32_stage_err"].items():
            assert e <= 2 * w["fp32_stage_err"][st], (n, st, e)
        assert r["top6_index"] == w["top6_index"]
        assert np.allclose(r["top6_logit"], w["top6_logit"], rtol=0, atol=1e-9)
        # the three conditions the seed was chosen by
        assert w["top6_min_gap"] >= 100 * w["fp32_logits_err"]
        assert 2.0 / arch.tokens < r["attn_max_mean"] < 0.9
    for k, v in sd.items():
        if "norm" in k and v.dim() == 1:
            assert not bool(((v == 0) | (v == 1)).any()), k


def test_module_form_equals_the_function():
    arch, sd, x = ref.case_inputs("t2_126", 0)
    with torch.no_grad():
        assert torch.equal(ref.EvaModule(sd, arch)(x[:1]), ref.forward(sd, x[:1], arch))


# ------------------------------------------------------------------------------------------------------------ RoPE
def test_rope_table_equals_a_literal_loop():
    G, ref_feat = 9, 16
    sin, cos = ck.rope_table(G, ref_feat)
    assert sin.shape == cos.shape == (G * G, 64)
    for gy in range(G):
        for gx in range(G):
            for c in range(64):
                axis, i = divmod(c // 2, 16)                              # y fills the first 32 channels, x the rest; every value twice
                pos = (gy if axis == 0 else gx) * ref_feat / G
                a = pos * 10000.0 ** -(i / 16)
                assert sin[gy * G + gx, c].item() == pytest.approx(math.sin(a), abs=1e-15)
                assert cos[gy * G + gx, c].item() == pytest.approx(math.cos(a), abs=1e-15)
    # rotation of one pair by hand
    t = torch.arange(64, dtype=torch.float64).reshape(1, 1, 1, 64) + 1
    r = ref.rope(t, sin[5:6], cos[5:6])[0, 0, 0]
    assert r[2].item() == pytest.approx(3 * cos[5, 2].item() - 4 * sin[5, 2].item()) and r[3].item() == pytest.approx(4 * cos[5, 3].item() + 3 * sin[5, 3].item())
    arch = ref.case_arch("t1_56")
    assert ck.rope_table(arch.grid)[0].shape[0] == arch.tokens - 1      # one row per PATCH token


def test_forward_rotates_the_patch_tokens_of_q_and_k_and_never_the_cls_token():
    """block 0's attention probabilities of the restatement against a literal per-token, per-pair loop that rotates tokens 1.. and
    leaves token 0 alone; the same loop WITH token 0 rotated (by any row of the table) must differ, or the check could not tell"""
    import torch.nn.functional as F
    name = "t1_56"
    arch, sd, x = ref.case_inputs(name, YARD["cases"][name]["weight_seed"])
    st, probs = {}, []
    with torch.no_grad():
        ref.forward(sd, x[:1].double(), arch, st, probs)
    y = F.layer_norm(st["tokens"][0], (arch.dim,), sd["blocks.0.norm1.weight"].double(), sd["blocks.0.norm1.bias"].double(), 1e-6)
    q = y @ sd["blocks.0.attn.q_proj.weight"].double().T + sd["blocks.0.attn.q_proj.bias"].double()
    k = y @ sd["blocks.0.attn.k_proj.weight"].double().T
    sin, cos = ck.rope_table(arch.grid, arch.ref_feat)

    def by_hand(rotate_cls):
        out = torch.zeros(arch.heads, arch.tokens, arch.tokens, dtype=torch.float64)
        for h in range(arch.heads):
            qs, ks = [], []
            for t in range(arch.tokens):
                a, b = q[t, 64 * h:64 * h + 64].clone(), k[t, 64 * h:64 * h + 64].clone()
                row = t - 1 if t > 0 else (3 if rotate_cls else None)
                if row is not None:
                    for v in (a, b):
                        for i in range(0, 64, 2):
                            e, o = v[i].item(), v[i + 1].item()
                            v[i] = e * cos[row, i] - o * sin[row, i]
                            v[i + 1] = o * cos[row, i + 1] + e * sin[row, i + 1]
                qs.append(a)
                ks.append(b)
            out[h] = torch.softmax(torch.stack(qs) @ torch.stack(ks).T / 8.0, -1)
        return out

    assert (by_hand(False) - probs[0][0]).abs().max().item() < 1e-12
    assert (by_hand(True) - probs[0][0]).abs().max().item() > 1e-3


# ------------------------------------------------------------------------------------------------------------ converter
@pytest.mark.parametrize("name,qkv,fc1", [("t1_56", "separate", "separate"), ("t2_126", "fused", "separate"), ("t1_126", "fused", "fused")])
def test_converter_folds_and_pads(name, qkv, fc1):
    arch = ref.case_arch(name)
    sd = ref.synth_state(arch, 3, qkv=qkv, fc1=fc1)
    assert ck.guess_arch(sd, heads=arch.heads) == arch and ck.guess_arch(sd) == arch
    out = ck.fold_state(sd, arch)
    D, H, Hp = arch.dim, arch.hidden, ck.pad32(arch.hidden)
    assert (Hp, out["patch_embed.weight"].shape, out["head.weight"].shape) == (352, (D, 608), (64, D))
    assert all(v.dtype == torch.float32 for v in out.values())
    same = ref.synth_state(arch, 3)                                       # the separate forms of the same seed: one blob whatever the form
    for k, v in ck.fold_state(same, arch).items():
        assert torch.equal(v, out[k]), k
    b = "blocks.1."
    w = out[b + "attn.qkv.weight"]
    assert torch.equal(w[:D], same[b + "attn.q_proj.weight"] * 0.125)     # exact: a power of two
    assert torch.equal(w[D:2 * D], same[b + "attn.k_proj.weight"]) and torch.equal(w[2 * D:], same[b + "attn.v_proj.weight"])
    bias = out[b + "attn.qkv.bias"]
    assert torch.equal(bias[:D], same[b + "attn.q_proj.bias"] * 0.125) and not bias[D:2 * D].any() and torch.equal(bias[2 * D:], same[b + "attn.v_proj.bias"])
    f1 = out[b + "mlp.fc1.weight"]
    assert f1.shape == (2 * Hp, D)
    assert torch.equal(f1[:H], same[b + "mlp.fc1_g.weight"]) and torch.equal(f1[Hp:Hp + H], same[b + "mlp.fc1_x.weight"])
    assert not f1[H:Hp].any() and not f1[Hp + H:].any() and not out[b + "mlp.fc1.bias"][H:Hp].any() and not out[b + "mlp.fc1.bias"][Hp + H:].any()
    assert not out[b + "mlp.fc2.weight"][:, H:].any() and torch.equal(out[b + "mlp.fc2.weight"][:, :H], same[b + "mlp.fc2.weight"])
    if arch.scale_mlp:
        assert not out[b + "mlp.norm.weight"][H:].any() and not out[b + "mlp.norm.bias"][H:].any()
    else:
        assert b + "mlp.norm.weight" not in out
    assert (b + "attn.norm.weight" in out) == arch.scale_attn_inner
    assert not out["patch_embed.weight"][:, 588:].any() and not out["head.weight"][arch.classes:].any() and not out["head.bias"][arch.classes:].any()
    assert torch.equal(out["final_norm.weight"], sd["fc_norm.weight" if arch.pool == "avg" else "norm.weight"])
    assert out["rope_sin"].shape == (arch.tokens - 1, 64)


def refused(fn, *words):
    with pytest.raises(_capi.RtdError) as e:
        fn()
    assert e.value.code == _capi.RTD_E_WEIGHTS and all(w in str(e.value) for w in words), str(e.value)


def test_converter_refusals():
    arch = ref.case_arch("t1_56")
    sd = ref.synth_state(arch, 0)
    refused(lambda: ck.fold_state(sd, ck.EvaArch(**dict(ck.asdict(arch), heads=4))), "head dim 32")
    refused(lambda: ck.fold_state(sd, ck.guess_arch(sd, heads=4)), "head dim 32")
    refused(lambda: ck.fold_state(sd, ck.EvaArch(**dict(ck.asdict(arch), img=126))), "no resampling")
    refused(lambda: ck.guess_arch(dict(sd, **{"blocks.0.post_norm.weight": sd["blocks.0.norm1.weight"]})), "use_post_norm")
    refused(lambda: ck.guess_arch(sd, model_args={"use_post_norm": True}), "use_post_norm")
    odd = dict(sd)
    odd["blocks.0.mlp.fc1.weight"] = torch.zeros(arch.hidden + 5, arch.dim)
    del odd["blocks.0.mlp.fc1_g.weight"]
    refused(lambda: ck.guess_arch(odd), "fc1")
    short = dict(sd)
    del short["blocks.1.attn.proj.bias"]
    refused(lambda: ck.fold_state(short, arch), "blocks.1.attn.proj.bias")
    refused(lambda: ck.guess_arch({"foo": torch.zeros(1)}), "missing tensor")


def test_checkpoint_files_and_the_blob_cache_round_trip(tmp_path, monkeypatch):
    arch = ref.case_arch("t2_126")
    sd = ref.synth_state(arch, 1, qkv="fused")
    want = ck.make_blob(sd)[1]
    # a torch.save state dict under model_state_dict (src/species_classifier.py:266-267)
    pt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": sd, "epoch": 3}, pt)
    # timm's model.safetensors, written by hand: 8-byte header length, JSON table, raw data
    table, data = {"__metadata__": {"format": "pt"}}, b""
    for k, v in sd.items():
        raw = v.contiguous().numpy().tobytes()
        table[k] = {"dtype": "F32", "shape": list(v.shape), "data_offsets": [len(data), len(data) + len(raw)]}
        data += raw
    head = json.dumps(table).encode()
    st = tmp_path / "model.safetensors"
    st.write_bytes(len(head).to_bytes(8, "little") + head + data)
    monkeypatch.setenv("RTD_BLOB_CACHE", str(tmp_path / "cache"))
    for path in (pt, st):
        a1, b1 = ck.cached_blob(path)
        files = sorted(os.listdir(tmp_path / "cache"))
        a2, b2 = ck.cached_blob(path)                                    # from the cache
        assert a1 == a2 == arch and b1 == b2 == want and sorted(os.listdir(tmp_path / "cache")) == files
    assert len(os.listdir(tmp_path / "cache")) == 4                      # blob + arch per file
    got = unpack_blob(want)
    assert got["pos_embed"].shape == (arch.tokens, arch.dim)
    # a torn cache file is rebuilt, not trusted
    for f in os.listdir(tmp_path / "cache"):
        if f.endswith(".rtdw"):
            (tmp_path / "cache" / f).write_bytes(want[: len(want) // 2])
    assert ck.cached_blob(pt)[1] == want


# ------------------------------------------------------------------------------------------------------------ the C side, before any HIP call
def test_create_refuses_a_bad_config_or_blob_before_any_hip_call():
    L = _capi.lib()
    arch = ref.case_arch("t1_56")
    blob = ck.make_blob(ref.synth_state(arch, 0), arch)[1]
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)

    def create(cfg, b=buf, n=len(blob)):
        h = C.c_void_p(0xDEAD)
        rc = L.rtd_eva_create(C.byref(cfg), b, n, C.byref(h))
        assert h.value is None                                            # a refused create overwrites the handle with NULL
        return rc, L.rtd_eva_last_error(None) or b""

    def cfg(**kw):
        c = classifier.eva_config(arch, 0, "f16x3", 4)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    for kw, word in ((dict(heads=4), b"head dim must be 64"), (dict(precision=_capi.PREC_BF16), b"precision"), (dict(max_batch=65), b"max_batch"),
                     (dict(img=57), b"multiple of patch"), (dict(pool=3), b"pool"), (dict(struct_size=8), b"struct_size")):
        rc, msg = create(cfg(**kw))
        assert rc == _capi.RTD_E_INVALID and word in msg, (kw, msg)
    rc, msg = create(cfg(), None, 0)
    assert rc == _capi.RTD_E_WEIGHTS and b"empty weight blob" in msg
    rc, msg = create(cfg(), (C.c_char * 64).from_buffer_copy(b"XXXX" + bytes(60)), 64)
    assert rc == _capi.RTD_E_WEIGHTS and b"bad magic" in msg
    rc, msg = create(cfg(depth=3))
    assert rc == _capi.RTD_E_WEIGHTS and b"missing tensor blocks.2.norm1.weight" in msg
    rc, msg = create(cfg(classes=100))
    assert rc == _capi.RTD_E_WEIGHTS and b"weight shape mismatch: head.weight" in msg
    bad = bytearray(blob)
    w = unpack_blob(blob)["blocks.0.attn.proj.weight"]
    off = w.__array_interface__["data"][0] - np.frombuffer(blob, np.uint8).__array_interface__["data"][0]
    bad[off:off + 4] = np.float32(70000.0).tobytes()
    rc, msg = create(cfg(), (C.c_char * len(bad)).from_buffer_copy(bytes(bad)))
    assert rc == _capi.RTD_E_WEIGHTS and b"blocks.0.attn.proj.weight" in msg and b"65504" in msg
    assert L.rtd_eva_forward(None, None, 1, None, None) == _capi.RTD_E_INVALID
    L.rtd_eva_close(None)


# ------------------------------------------------------------------------------------------------------------ install()
def test_install_on_a_stand_in_species_classifier():
    arch = ref.case_arch("t1_56")
    sd = ref.synth_state(arch, 0)

    class HostModel:                                                       # what install() needs of an Eva02Classifier, on the CPU
        def __init__(self):
            self.arch, self.device, self.torch_device = arch, 0, "cpu"

        def __call__(self, x):
            return ref.forward(sd, x, arch)

    clf = StandInSpeciesClassifier(num_classes=arch.classes, input_size=336, device="cpu")
    clf.mean, clf.std = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)
    model = classifier.install(clf, HostModel())
    assert clf.model is model and clf.input_size == 56
    assert clf._mean_tensor.shape == clf._std_tensor.shape == (3, 1, 1) and clf._mean_tensor.flatten().tolist() == pytest.approx([0.5, 0.4, 0.3])
    with torch.no_grad():
        x = (torch.rand(2, 3, 56, 56) - clf._mean_tensor) / clf._std_tensor
        assert clf.model(x).shape == (2, arch.classes)
    bare = types.SimpleNamespace(device="cpu")
    classifier.install(bare, HostModel())
    assert bare._mean_tensor.flatten().tolist() == pytest.approx(list(classifier.OPENAI_CLIP_MEAN))
    e = classifier.Eva02Classifier.__new__(classifier.Eva02Classifier)
    assert e.eval() is e and e.to("cuda:0") is e
