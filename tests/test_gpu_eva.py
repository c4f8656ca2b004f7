"""The EVA02 species classifier on the MI355X (csrc/classifier.hip) against the fp64 restatement (tests/eva_ref.py).

One gate for every float comparison, kernel level and end to end: the error of the SAME computation in torch fp32 on the CPU against fp64
(computed here for the kernels, read from tests/golden/eva_yardstick.json for the network), times
  8 for f16x3: 4 for the two significant bits the pair format lacks against fp32, times 2 for the dropped lo * lo term and the spread
               of a maximum over a few thousand elements;
  2 for fp32:  accumulation order only.
Kernel inputs are the stored values (pair-rounded for f16x3), and every ratio is printed.  Shapes are the smallest at which each path can
go wrong: L = 17 (below one key tile), L = 82 (crosses a 64-key tile, not a multiple of 16), L = 577 (the ViT-L/14 @ 336 length: nine full
tiles and one key), c_valid 341 of 352 and 2730 of 2752 (a valid prefix that ends inside an 8-channel chunk; the second register chunk)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eva_ref as ref
from tests.standins import StandInPipeline
from telescope_cam_detection_amd import _capi, classifier
from telescope_cam_detection_amd.eva_checkpoint import rope_table
from telescope_cam_detection_amd.stage2 import BatchedStage2, CropBatcher

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARD = json.load(open(os.path.join(ROOT, "tests", "golden", "eva_yardstick.json")))
ENGINES = ("f16x3", "fp32")
FACTOR = {"f16x3": 8.0, "fp32": 2.0}
DTYPE = {"f16x3": _capi.DT_F16X2, "fp32": _capi.DT_F32}


def ck(rc):
    assert rc == 0, (rc, _capi.lib().rtd_last_error(None))


def quant(x, engine):
    """the values the kernel sees for an fp32 array stored in the engine's format, and their device storage"""
    x = np.ascontiguousarray(x, np.float32)
    if engine == "fp32":
        return x, torch.from_numpy(x).cuda()
    s = _capi.to_split(x)
    return _capi.from_split(s), torch.from_numpy(s.view(np.int16)).cuda()


def unquant(t, engine):
    return t.cpu().numpy() if engine == "fp32" else _capi.from_split(t.cpu().numpy().view(np.uint16))


def empty_like_stored(shape, engine):
    return torch.zeros(shape, dtype=torch.float32, device="cuda") if engine == "fp32" else torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=torch.int16, device="cuda")


def within(what, engine, got, ref64, ref32):
    """the gate: max |got - fp64| <= factor x max |torch fp32 - fp64|"""
    ref64 = np.asarray(ref64, np.float64)
    e_ref = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    e_got = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    assert e_ref > 0, what
    print(f"{what} [{engine}]: max |delta| {e_got:.3e}, torch fp32 {e_ref:.3e}, ratio {e_got / e_ref:.2f} (gate {FACTOR[engine]:.0f})")
    assert np.isfinite(got).all() and e_got <= FACTOR[engine] * e_ref, (what, engine, e_got, e_ref)


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("engine", ENGINES)
def test_patchify(engine):
    n, S, p = 2, 56, 14
    G, K, Kp = S // p, 3 * p * p, 608
    x = torch.randn((n, 3, S, S), generator=torch.Generator().manual_seed(1))
    rows = empty_like_stored((n * G * G, Kp), engine)
    xd = x.cuda()
    ck(_capi.lib().rtd_op_eva_patchify(DTYPE[engine], xd.data_ptr(), rows.data_ptr(), n, S, p))
    want = np.zeros((n * G * G, Kp), np.float32)
    want[:, :K] = F.unfold(x, p, stride=p).transpose(1, 2).reshape(n * G * G, K).numpy()      # unfold's k = (c p + i) p + j: the conv filter's own flattening
    assert np.array_equal(unquant(rows, engine), quant(want, engine)[0])                         # data movement: exact


@pytest.mark.parametrize("engine", ENGINES)
def test_rope(engine):
    n, G, heads = 2, 4, 2
    L, D = G * G + 1, heads * 64
    q, qd = quant(np.random.default_rng(2).standard_normal((n, L, 3 * D)).astype(np.float32), engine)
    sin, cos = rope_table(G)
    sin32, cos32 = sin.float().contiguous(), cos.float().contiguous()
    sind, cosd = sin32.cuda(), cos32.cuda()
    ck(_capi.lib().rtd_op_eva_rope(DTYPE[engine], qd.data_ptr(), sind.data_ptr(), cosd.data_ptr(), n, L, heads))
    got = unquant(qd, engine).reshape(n, L, 3 * D)

    def rotated(dt):
        t = torch.from_numpy(q).to(dt).reshape(n, L, 3, heads, 64)
        out = t.clone()
        out[:, 1:, :2] = ref.rope(t[:, 1:, :2], sin32.to(dt).reshape(L - 1, 1, 1, 64), cos32.to(dt).reshape(L - 1, 1, 1, 64))
        return out.reshape(n, L, 3 * D).numpy()

    r64, r32 = rotated(torch.float64), rotated(torch.float32)
    assert np.array_equal(got[:, 0], q[:, 0]) and np.array_equal(got[:, :, 2 * D:], q[:, :, 2 * D:])      # the cls token and v are untouched
    within("rope L 17", engine, got, r64, r32)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("c,c_valid,swiglu", [(352, 341, 0), (352, 341, 1), (2752, 2730, 0)])
def test_layernorm(engine, c, c_valid, swiglu):
    rows = 5
    rng = np.random.default_rng(3)
    x, xd = quant((rng.standard_normal((rows, (2 if swiglu else 1) * c)) * 1.5 + 0.3).astype(np.float32), engine)
    gain = torch.from_numpy((1 + 0.2 * rng.standard_normal(c)).astype(np.float32))
    bias = torch.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32))
    y = empty_like_stored((rows, c), engine)
    gd, bd = gain.cuda(), bias.cuda()
    ck(_capi.lib().rtd_op_eva_layernorm(DTYPE[engine], xd.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), rows, c, c_valid, swiglu, 1, 1e-6))
    got = unquant(y, engine)

    def normed(dt):
        t = torch.from_numpy(x).to(dt)
        v = F.silu(t[:, :c]) * t[:, c:] if swiglu else t
        return F.layer_norm(v[:, :c_valid], (c_valid,), gain[:c_valid].to(dt), bias[:c_valid].to(dt), 1e-6).numpy()

    assert (got[:, c_valid:] == 0).all()                                  # the pad channels are written as zero
    within(f"layernorm {c_valid} of {c} swiglu {swiglu}", engine, got[:, :c_valid], normed(torch.float64), normed(torch.float32))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("n,L", [(1, 17), (2, 82), (1, 577)])
def test_attention(engine, n, L):
    heads, D = 2, 128
    rng = np.random.default_rng(4)
    qkv = rng.standard_normal((n, L, 3 * D)).astype(np.float32)
    qkv[..., :D] *= 0.6
    qkv[..., D:2 * D] *= 0.6                                               # score std ~ 8 * 0.36: a softmax neither uniform nor one-hot
    x, _ = quant(qkv, engine)
    stored = x.copy()
    if engine == "fp32":
        stored[..., :D] *= 8.0                                             # the fp32 form multiplies its scores by 1 / 8 itself (exact)
    xd = quant(stored, engine)[1]
    o = empty_like_stored((n, L, D), engine)
    ck(_capi.lib().rtd_op_eva_attention(DTYPE[engine], xd.data_ptr(), o.data_ptr(), n, L, heads))
    got = unquant(o, engine)

    def attn(dt):
        t = torch.from_numpy(x).to(dt).reshape(n, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(t[0] @ t[1].transpose(-2, -1), -1)
        return (a @ t[2]).transpose(1, 2).reshape(n, L, D).numpy()

    within(f"attention n {n} L {L}", engine, got, attn(torch.float64), attn(torch.float32))


# ------------------------------------------------------------------------------------------------------------ the handle
_REF, _CLF = {}, {}


def reference(name, n):
    """the fp64 restatement of a yardstick case at batch n, computed once: (arch, state, x [n], logits, stages)"""
    if (name, n) not in _REF:
        arch, sd, x = ref.case_inputs(name, YARD["cases"][name]["weight_seed"])
        st = {}
        with torch.no_grad():
            out = ref.forward(sd, x[:n].double(), arch, st)
        _REF[name, n] = (arch, sd, x[:n].contiguous(), out.numpy(), {k: v.numpy() for k, v in st.items()})
    return _REF[name, n]


def clf_for(name, engine):
    if (name, engine) not in _CLF:
        arch, sd = reference(name, 1)[:2]
        _CLF[name, engine] = classifier.Eva02Classifier(sd, precision=engine, max_batch=3, arch=arch)
    return _CLF[name, engine]


@pytest.fixture(scope="module", autouse=True)
def _close_classifiers():
    yield
    for c in _CLF.values():
        c.close()
    _CLF.clear()


def gate(what, engine, got, want, e32):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what} [{engine}]: max |delta| {err:.3e}, torch fp32 {e32:.3e}, ratio {err / e32:.2f} (gate {FACTOR[engine]:.0f})")
    assert np.isfinite(got).all() and err <= FACTOR[engine] * e32, (what, engine, err, e32)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("n", ref.BATCHES)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_logits_and_top5(name, n, engine):
    arch, _, x, want, _ = reference(name, n)
    clf = clf_for(name, engine)
    got = clf(x.cuda()).cpu().numpy()
    assert got.shape == (n, arch.classes)
    gate(f"{name} n {n} logits", engine, got, want, YARD["cases"][name]["n"][str(n)]["fp32_logits_err"])
    assert np.array_equal(np.argsort(-got, 1)[:, :5], np.argsort(-want, 1)[:, :5])
    assert np.array_equal(np.argsort(-want, 1)[:, :6], np.asarray(YARD["cases"][name]["n"][str(n)]["top6_index"]))
    assert clf.self_check() == 0


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("n", ref.BATCHES)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_stage_by_stage(name, n, engine):
    arch, _, x, _, stages = reference(name, n)
    clf = clf_for(name, engine)
    xd = x.cuda()
    clf(xd)
    yard = YARD["cases"][name]["n"][str(n)]["fp32_stage_err"]
    for st in ref.stage_names(arch):
        got = clf.debug_tensor(st)
        assert got.shape == stages[st].shape, st
        gate(f"{name} n {n} {st}", engine, got, stages[st], yard[st])


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["t1_126", "t2_126"])
def test_cached_batch_size_allocates_nothing_and_a_batch_equals_its_images(name, engine):
    _, _, x, _, _ = reference(name, 3)
    clf = clf_for(name, engine)
    xd = x.cuda()
    first = clf(xd)
    singles = torch.cat([clf(xd[i:i + 1]) for i in range(3)])
    torch.cuda.synchronize()
    arena = clf.arena_bytes()                                              # (the handle's one growing allocation; the device's free memory is shared with others)
    out = torch.empty_like(first)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ck(_capi.lib().rtd_eva_forward(clf._h, C.c_void_p(xd.data_ptr()), 3, C.c_void_p(out.data_ptr()), stream))
    ck(_capi.lib().rtd_eva_forward(clf._h, C.c_void_p(xd.data_ptr()), 1, C.c_void_p(out.data_ptr()), stream))
    ck(_capi.lib().rtd_eva_forward(clf._h, C.c_void_p(xd.data_ptr()), 3, C.c_void_p(out.data_ptr()), stream))
    torch.cuda.synchronize()
    assert clf.arena_bytes() == arena
    assert torch.equal(out, first)                                         # the same plan, the same launches: the same bits
    # N = 3 equals three N = 1 calls: every kernel here works row by row (a conv tile sums a row's K in one order whatever the tile's
    # height), so the images of a batch carry the bits of their own calls
    print(f"{name} batch of 3 against three calls [{engine}]: max |delta| {float((first - singles).abs().max()):.3e}")
    assert torch.equal(first, singles)


@pytest.mark.parametrize("name", ["t1_56", "t2_126"])
def test_create_forward_refused_forward_close_round(name):
    arch, sd, x, want, _ = reference(name, 3)
    L = _capi.lib()
    clf = classifier.Eva02Classifier(sd, precision="f16x3", max_batch=2, arch=arch)
    xd = x.cuda()
    a = clf(xd[:2]).clone()
    out = torch.full((3, arch.classes), 7.0, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.rtd_eva_forward(clf._h, C.c_void_p(xd.data_ptr()), 3, C.c_void_p(out.data_ptr()), stream) == _capi.RTD_E_INVALID
    assert b"max_batch" in L.rtd_eva_last_error(clf._h)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                        # a refused call leaves the output untouched
    with pytest.raises(_capi.RtdError):
        clf.debug_tensor("blocks.9")
    assert torch.equal(clf(xd[:2]), a)
    big = clf(xd)                                                          # above max_batch the Python side chunks: 2 + 1
    gate(f"{name} chunked 2 + 1", "f16x3", big.cpu().numpy(), want, YARD["cases"][name]["n"]["3"]["fp32_logits_err"])
    with pytest.raises(_capi.RtdError):
        clf.wait_stream(0)                                                 # the handle owns no stream: nothing to order
    clf.close()
    clf.close()


# ------------------------------------------------------------------------------------------------------------ glue
def test_batched_stage2_with_installed_classifiers_yields_the_restatement_s_species():
    name = "t1_56"
    arch, sd, _, _, _ = reference(name, 1)
    e32 = YARD["cases"][name]["n"]["3"]["fp32_logits_err"]

    def pipeline(installed):
        p = StandInPipeline(min_crop_size=16)
        for clf in p.species_classifiers.values():
            if installed:
                _CLF[id(clf), "glue"] = classifier.install(clf, sd, arch=arch, max_batch=4)
                assert clf.input_size == arch.img and clf._mean_tensor.shape == (3, 1, 1) and clf._std_tensor.is_cuda
            else:
                clf.model = lambda t: ref.forward(sd, t.double().cpu(), arch).float().to(t.device)      # the fp64 restatement
                clf.input_size = arch.img
        return p

    rng = np.random.default_rng(91)
    frames_np = [rng.integers(0, 256, (80, 100, 3), dtype=np.uint8), rng.integers(0, 256, (60, 64, 3), dtype=np.uint8)]
    boxes = [[(14, 10.5, 12.2, 34.9, 40.0), (15, 50, 10, 90, 45), (14, 0, 0, 10, 10), (2, 20, 20, 60, 60)], [(21, 8, 9, 40, 44), (14, 30, 20, 63, 59.5)]]
    results = []
    for installed in (True, False):
        p = pipeline(installed)
        s2 = BatchedStage2(p, batcher=CropBatcher(input_size=arch.img, min_crop_size=p.min_crop_size, crop_padding_percent=p.crop_padding_percent))
        dets = [[{"class_id": c, "class_name": "x", "confidence": 0.9, "bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}} for c, x1, y1, x2, y2 in per]
                for per in boxes]
        results.append(s2.process_batch([torch.from_numpy(f).cuda() for f in frames_np], dets))
    classified = 0
    for g_per, w_per in zip(*results):
        for g, w in zip(g_per, w_per):
            assert set(g) == set(w)
            for k in ("species", "taxonomic_level", "stage2_category"):
                assert g.get(k) == w.get(k), (k, g, w)
            # softmax moves a probability by at most the largest logit error (|dp| <= 2 p (1 - p) max |dlogit|), held to 8 x the fp32 yardstick;
            # plus torch's own fp32 softmax rounding
            assert abs(g["species_confidence"] - w["species_confidence"]) <= 8 * e32 + 2.0 ** -20, (g, w)
            classified += g.get("stage2_category") is not None
    assert classified >= 4
