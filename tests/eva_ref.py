"""Restatement of the Stage-2 species classifier's network: timm's `Eva` (timm/models/eva.py), the model class behind
timm/eva02_large_patch14_clip_336.merged2b_ft_inat21 which the reference's config names.  Plain torch on a timm-keyed state dict, generic
in the dtype, so the same code is the fp64 definition and the fp32 / fp16 runs it is compared with.

timm is not importable here and no EVA02 checkpoint is at hand: the architecture, the state-dict key table and the RoPE rule
(telescope_cam_detection_amd/eva_checkpoint.rope_table) are written from the public sources and could NOT be checked against them
offline.

Arithmetic (pre-norm blocks, no layer scale, LayerNorm eps 1e-6):
  x = cat(cls_token, patch_embed(img)) + pos_embed                       patch_embed: patch x patch conv, stride patch, bias
  per block:  y = norm1(x);  q, k, v = linear(y) with q and v biases, no k bias;  q, k = rope(q), rope(k) on the patch tokens only;
              x = x + proj(attn_norm?(softmax(q k^T / 8) v));  y = norm2(x);  x = x + fc2(mlp_norm?(silu(fc1_g y) * fc1_x y))
  rope(t) = t * cos + stack(-t[1::2], t[0::2]) * sin                      (interleaved pairs)
  pool token: head(norm(x)[:, 0]);  pool avg: head(fc_norm(mean(x[:, 1:])))
"""
import numpy as np
import torch
import torch.nn.functional as F

from telescope_cam_detection_amd.eva_checkpoint import HEAD_DIM, EvaArch, rope_table

EPS = 1e-6


def tiny_arch(name, img):
    """the test architectures: dim 128, 2 heads, depth 2, hidden int(128 * 8 / 3) = 341, 37 classes"""
    base = dict(img=img, patch=14, dim=128, depth=2, heads=2, hidden=int(128 * 8 / 3), classes=37, ref_feat=16)
    if name == "t1":
        return EvaArch(scale_attn_inner=True, scale_mlp=True, pool="token", **base)
    if name == "t2":
        return EvaArch(scale_attn_inner=False, scale_mlp=False, pool="avg", **base)
    raise KeyError(name)


QKV_FORM = {"t1": "separate", "t2": "fused"}

INIT_RULE = ("one torch.Generator(seed), tensors drawn in the order synth_state writes them; linear / conv filters randn * gain / sqrt(fan_in) "
             "with gain 1.6 for q and k, 1 elsewhere; biases randn * 0.1; LayerNorm gains 1 + 0.2 * randn, biases 0.1 * randn; "
             "cls_token and pos_embed randn * 0.5; pos_embed is drawn last")


def synth_state(arch: EvaArch, seed=0, qkv="separate", fc1="separate"):
    """A seeded timm-keyed state dict (fp32).  qkv: 'separate' (q_proj / k_proj / v_proj) or 'fused' (qkv.weight + q_bias / v_bias);
    fc1: 'separate' (fc1_g / fc1_x) or 'fused' (one fc1 of 2 H rows, gate first)."""
    g = torch.Generator().manual_seed(seed)
    D, H = arch.dim, arch.hidden
    sd = {}

    def randn(*shape, std=1.0):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    def lin(name, out, inp, gain=1.0, bias=True):
        sd[name + ".weight"] = randn(out, inp, std=gain / inp ** 0.5)
        if bias:
            sd[name + ".bias"] = randn(out, std=0.1)

    def ln(name, width):
        sd[name + ".weight"] = 1.0 + randn(width, std=0.2)
        sd[name + ".bias"] = randn(width, std=0.1)

    K = 3 * arch.patch ** 2
    sd["patch_embed.proj.weight"] = randn(D, 3, arch.patch, arch.patch, std=1.0 / K ** 0.5)
    sd["patch_embed.proj.bias"] = randn(D, std=0.1)
    sd["cls_token"] = randn(1, 1, D, std=0.5)
    for i in range(arch.depth):
        b = f"blocks.{i}."
        ln(b + "norm1", D)
        lin(b + "attn.q_proj", D, D, 1.6)
        lin(b + "attn.k_proj", D, D, 1.6, bias=False)
        lin(b + "attn.v_proj", D, D)
        if qkv == "fused":
            sd[b + "attn.qkv.weight"] = torch.cat([sd.pop(b + f"attn.{n}_proj.weight") for n in "qkv"], 0)
            sd[b + "attn.q_bias"], sd[b + "attn.v_bias"] = sd.pop(b + "attn.q_proj.bias"), sd.pop(b + "attn.v_proj.bias")
        if arch.scale_attn_inner:
            ln(b + "attn.norm", D)
        lin(b + "attn.proj", D, D)
        ln(b + "norm2", D)
        lin(b + "mlp.fc1_g", H, D)
        lin(b + "mlp.fc1_x", H, D)
        if fc1 == "fused":
            sd[b + "mlp.fc1.weight"] = torch.cat([sd.pop(b + "mlp.fc1_g.weight"), sd.pop(b + "mlp.fc1_x.weight")], 0)
            sd[b + "mlp.fc1.bias"] = torch.cat([sd.pop(b + "mlp.fc1_g.bias"), sd.pop(b + "mlp.fc1_x.bias")], 0)
        if arch.scale_mlp:
            ln(b + "mlp.norm", H)
        lin(b + "mlp.fc2", D, H)
    ln("fc_norm" if arch.pool == "avg" else "norm", D)
    lin("head", arch.classes, D)
    sd["pos_embed"] = randn(1, arch.tokens, D, std=0.5)
    return sd


def rope(t, sin, cos):
    """t: [B, heads, tokens, 64]; sin, cos: [tokens, 64].  x * cos + stack(-x[1::2], x[0::2]) * sin"""
    rot = torch.stack([-t[..., 1::2], t[..., 0::2]], -1).reshape(t.shape)
    return t * cos + rot * sin


def forward(sd, x, arch: EvaArch, stages=None, probs=None):
    """x: [N, 3, S, S] in the dtype to compute in; sd: a timm-keyed state dict (any float dtype: cast to x's).  Returns the logits
    [N, classes].  `stages` (a dict) receives the stage outputs rtd_debug_eva_tensor knows, as [N, rows, C]; `probs` (a list) the
    attention probabilities of every block, [N, heads, L, L]."""
    dt, N, D, hd = x.dtype, x.shape[0], arch.dim, arch.dim // arch.heads
    dev = x.device

    def w(name):
        return sd[name].to(device=dev, dtype=dt)

    def keep(name, t):
        if stages is not None:
            stages[name] = t.detach().reshape(N, -1, t.shape[-1]).clone()

    def ln(name, t):
        return F.layer_norm(t, (t.shape[-1],), w(name + ".weight"), w(name + ".bias"), EPS)

    sin, cos = (t.to(device=dev, dtype=dt) for t in rope_table(arch.grid, arch.ref_feat, hd))
    pe = F.conv2d(x, w("patch_embed.proj.weight"), w("patch_embed.proj.bias"), stride=arch.patch).flatten(2).transpose(1, 2)
    keep("patch_embed", pe)
    x = torch.cat([w("cls_token").reshape(1, 1, D).expand(N, -1, -1), pe], 1) + w("pos_embed").reshape(1, -1, D)
    keep("tokens", x)
    L = x.shape[1]
    for i in range(arch.depth):
        b = f"blocks.{i}."
        y = ln(b + "norm1", x)
        if b + "attn.qkv.weight" in sd:
            bias = torch.cat([w(b + "attn.q_bias"), torch.zeros(D, dtype=dt, device=dev), w(b + "attn.v_bias")])
            q, k, v = F.linear(y, w(b + "attn.qkv.weight"), bias).chunk(3, -1)
        else:
            q = F.linear(y, w(b + "attn.q_proj.weight"), w(b + "attn.q_proj.bias"))
            k = F.linear(y, w(b + "attn.k_proj.weight"))
            v = F.linear(y, w(b + "attn.v_proj.weight"), w(b + "attn.v_proj.bias"))
        q, k, v = (t.reshape(N, L, arch.heads, hd).transpose(1, 2) for t in (q, k, v))
        q = torch.cat([q[:, :, :1], rope(q[:, :, 1:], sin, cos)], 2)
        k = torch.cat([k[:, :, :1], rope(k[:, :, 1:], sin, cos)], 2)
        a = torch.softmax((q * hd ** -0.5) @ k.transpose(-2, -1), -1)
        if probs is not None:
            probs.append(a.detach())
        o = (a @ v).transpose(1, 2).reshape(N, L, D)
        if arch.scale_attn_inner:
            o = ln(b + "attn.norm", o)
        x = x + F.linear(o, w(b + "attn.proj.weight"), w(b + "attn.proj.bias"))
        keep(f"blocks.{i}.attn", x)
        y = ln(b + "norm2", x)
        if b + "mlp.fc1.weight" in sd:
            g_, x_ = F.linear(y, w(b + "mlp.fc1.weight"), w(b + "mlp.fc1.bias")).chunk(2, -1)
        else:
            g_ = F.linear(y, w(b + "mlp.fc1_g.weight"), w(b + "mlp.fc1_g.bias"))
            x_ = F.linear(y, w(b + "mlp.fc1_x.weight"), w(b + "mlp.fc1_x.bias"))
        h = F.silu(g_) * x_
        if arch.scale_mlp:
            h = ln(b + "mlp.norm", h)
        x = x + F.linear(h, w(b + "mlp.fc2.weight"), w(b + "mlp.fc2.bias"))
        keep(f"blocks.{i}", x)
    if arch.pool == "avg":
        p = ln("fc_norm", x[:, 1:].mean(1))
    else:
        p = ln("norm", x)[:, 0]
    keep("pool", p)
    out = F.linear(p, w("head.weight"), w("head.bias"))
    keep("logits", out)
    return out


class EvaModule(torch.nn.Module):
    """the restatement as a module (tools/eva_bench.py times its forward, plain and under autocast): the state dict as buffers"""

    def __init__(self, sd, arch: EvaArch):
        super().__init__()
        self.arch = arch
        self._names = {}
        for k, v in sd.items():
            self._names[k] = k.replace(".", "__")
            self.register_buffer(self._names[k], v.clone())

    def forward(self, x):
        return forward({k: getattr(self, n) for k, n in self._names.items()}, x, self.arch)


def stage_names(arch: EvaArch):
    names = ["patch_embed", "tokens"]
    for i in range(arch.depth):
        names += [f"blocks.{i}.attn", f"blocks.{i}"]
    return names + ["pool", "logits"]


# ---- the yardstick cases (tools/make_eva_yardstick.py records them in tests/golden/eva_yardstick.json)
CASES = {
    "t1_56": dict(arch="t1", img=56, input_seed=11),      # L = 17: below one key tile
    "t1_126": dict(arch="t1", img=126, input_seed=12),    # L = 82: crosses a 64-key tile, not a multiple of 16
    "t2_126": dict(arch="t2", img=126, input_seed=13),
}
BATCHES = (1, 3)


def case_arch(name):
    c = CASES[name]
    return tiny_arch(c["arch"], c["img"])


def case_inputs(name, weight_seed):
    """(arch, state dict, x [3, 3, S, S] fp32): normalised-crop-like inputs, randn; a batch of n is x[:n]"""
    c = CASES[name]
    arch = case_arch(name)
    sd = synth_state(arch, weight_seed, qkv=QKV_FORM[c["arch"]])
    x = torch.randn((max(BATCHES), 3, arch.img, arch.img), generator=torch.Generator().manual_seed(c["input_seed"]), dtype=torch.float32)
    return arch, sd, x


def measure_case(name, weight_seed):
    """per batch size: the fp32 run's max |delta| against fp64 for the logits and every stage, the fp64 top-6 logits, their smallest gap,
    and the mean over (block, image, head, row) of the largest attention probability"""
    arch, sd, x = case_inputs(name, weight_seed)
    rec = {}
    with torch.no_grad():
        for n in BATCHES:
            st64, st32, pr = {}, {}, []
            ref = forward(sd, x[:n].double(), arch, st64, pr)
            got = forward(sd, x[:n], arch, st32)
            top = ref.topk(6, -1)
            rec[str(n)] = {
                "fp32_logits_err": float((got.double() - ref).abs().max()),
                "fp32_stage_err": {k: float((st32[k].double() - st64[k]).abs().max()) for k in stage_names(arch)},
                "stage_max_abs": {k: float(st64[k].abs().max()) for k in stage_names(arch)},
                "top6_index": top.indices.tolist(),
                "top6_logit": top.values.tolist(),
                "top6_min_gap": float((top.values[:, :-1] - top.values[:, 1:]).min()),
                "attn_max_mean": float(np.mean([float(a.max(-1).values.mean()) for a in pr])),
            }
    return rec
