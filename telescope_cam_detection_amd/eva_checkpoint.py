"""timm `Eva` checkpoints -> the weight blob rtd_eva_create reads (csrc/classifier_host.h lists its tensors).

The checkpoint decides the architecture (`guess_arch`), as checkpoint.guess_arch does for the detector:
  `blocks.0.attn.norm.*`  -> LayerNorm between attention and proj (scale_attn_inner)
  `blocks.0.mlp.norm.*`   -> LayerNorm between SwiGLU and fc2 (scale_mlp)
  `fc_norm.*`             -> avg pool + fc_norm, else the cls token behind `norm`
  `attn.qkv.weight` with `attn.q_bias` / `attn.v_bias`, or `attn.q_proj` / `k_proj` / `v_proj`: one [3 D, D] filter with a zero k bias
  `mlp.fc1_g` / `mlp.fc1_x`, or one fused `mlp.fc1.weight` [2 H, D] (timm's GluMlp: gate first)
Folding on the host (`fold_state`): head_dim ** -0.5 = 1 / 8 into the q filter and bias (exact, a power of two); hidden, 3 * patch^2 and
the classes zero-padded to whole 32-channel groups; the RoPE sin / cos tables computed HERE, in `rope_table` - the one place that knows
the frequency rule - and shipped as data.

timm is not importable where this was written and no EVA02 checkpoint was at hand: the key table and the module arithmetic
(tests/eva_ref.py) are restated from the public sources and could not be checked against them offline.
"""
from __future__ import annotations

import json
import os
import struct
from dataclasses import asdict, dataclass
from typing import Dict, Mapping, Tuple

import numpy as np
import torch

from . import _capi
from .weights import BLOB_MAGIC, BLOB_VERSION, _cache_dir, pack_blob, unpack_blob

HEAD_DIM = 64
POOLS = {"token": 0, "avg": 1}


def _refuse(msg: str):
    raise _capi.RtdError(_capi.RTD_E_WEIGHTS, msg)


def pad32(v: int) -> int:
    return (int(v) + 31) // 32 * 32


@dataclass(frozen=True)
class EvaArch:
    img: int = 336
    patch: int = 14
    dim: int = 1024
    depth: int = 24
    heads: int = 16
    hidden: int = 2730
    classes: int = 10000
    ref_feat: int = 16
    scale_attn_inner: bool = True
    scale_mlp: bool = True
    pool: str = "token"

    @property
    def grid(self) -> int:
        return self.img // self.patch

    @property
    def tokens(self) -> int:
        return self.grid * self.grid + 1

    @property
    def name(self) -> str:
        return "eva_" + "_".join(str(int(v)) if not isinstance(v, str) else v for v in asdict(self).values())


VIT_L_14_336 = EvaArch()      # timm/eva02_large_patch14_clip_336.merged2b_ft_inat21 (the reference's config/config.yaml:279-281)


def rope_table(grid: int, ref_feat: int = 16, head_dim: int = HEAD_DIM, temperature: float = 10000.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sin, cos), each [grid * grid, head_dim] float64: timm's RotaryEmbeddingCat(head_dim, in_pixels=False, feat_shape=(grid, grid),
    ref_feat_shape=(ref_feat, ref_feat)).  head_dim / 4 bands temperature ** -(i / bands) per axis, positions arange(grid) * ref_feat /
    grid, the y axis in the first half of the channels and the x axis in the second, every value twice (the interleaved pairs)."""
    nb = head_dim // 4
    bands = 1.0 / (temperature ** (torch.arange(nb, dtype=torch.float64) / nb))
    t = torch.arange(grid, dtype=torch.float64) / grid * ref_feat
    gy, gx = torch.meshgrid(t, t, indexing="ij")
    pos = torch.stack([gy, gx], -1).unsqueeze(-1) * bands           # [G, G, 2, nb]
    sin = pos.sin().reshape(grid * grid, 2 * nb).repeat_interleave(2, -1)
    cos = pos.cos().reshape(grid * grid, 2 * nb).repeat_interleave(2, -1)
    return sin, cos


# ---------------------------------------------------------------------------------------------------------------- reading
_ST_DTYPES = {"F64": np.float64, "F32": np.float32, "F16": np.float16, "I64": np.int64, "I32": np.int32, "U8": np.uint8, "BOOL": np.bool_}


def read_safetensors(path: str) -> Dict[str, torch.Tensor]:
    """the safetensors container (8-byte header length, a JSON table, raw little-endian data), read without the safetensors package"""
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        table = json.loads(f.read(n).decode("utf-8"))
        data = f.read()
    out = {}
    for name, e in table.items():
        if name == "__metadata__":
            continue
        a, b = e["data_offsets"]
        raw = data[a:b]
        if e["dtype"] == "BF16":
            t = torch.frombuffer(bytearray(raw), dtype=torch.bfloat16)
        elif e["dtype"] in _ST_DTYPES:
            t = torch.from_numpy(np.frombuffer(raw, dtype=_ST_DTYPES[e["dtype"]]).copy())
        else:
            _refuse(f"{name}: unsupported safetensors dtype {e['dtype']}")
        out[name] = t.reshape(e["shape"])
    return out


def state_dict_of(path_or_dict) -> Mapping[str, torch.Tensor]:
    """timm's `model.safetensors`, or a torch.save state dict, optionally under `model_state_dict` (src/species_classifier.py:266-267)
    or `state_dict`"""
    sd = path_or_dict
    if not isinstance(sd, Mapping):
        p = os.fspath(path_or_dict)
        sd = read_safetensors(p) if p.endswith(".safetensors") else torch.load(p, map_location="cpu")
    if not isinstance(sd, Mapping):
        _refuse("checkpoint is not a dict")
    for key in ("model_state_dict", "state_dict"):
        if isinstance(sd.get(key), Mapping):
            return sd[key]
    return sd


# ---------------------------------------------------------------------------------------------------------------- arch + folding
def _depth_of(sd) -> int:
    n = 0
    while f"blocks.{n}.norm1.weight" in sd:
        n += 1
    return n


def _refuse_post_norm(sd, model_args=None) -> None:
    """timm's post-norm blocks (use_post_norm) keep the names norm1 / norm2, so the keys alone cannot tell them apart: the flag of the
    checkpoint's model args (timm's config.json `model_args`, when the caller has it) decides, and any `post_norm` key does too"""
    if (model_args or {}).get("use_post_norm") or any("post_norm" in k for k in sd):
        _refuse("use_post_norm checkpoints are not built")


def guess_arch(sd: Mapping[str, torch.Tensor], ref_feat: int = 16, heads: int = None, model_args: Mapping = None) -> EvaArch:
    """The architecture a timm Eva state dict describes; RtdError(RTD_E_WEIGHTS) with the reason for what this build does not run.
    The head count is not in a state dict: `heads` (or model_args["num_heads"]) names it, the default is dim / 64."""
    _refuse_post_norm(sd, model_args)
    for k in ("patch_embed.proj.weight", "pos_embed", "cls_token", "head.weight", "blocks.0.norm1.weight"):
        if k not in sd:
            _refuse(f"missing tensor {k}: not a timm Eva state dict")
    pw = sd["patch_embed.proj.weight"]
    dim, patch = int(pw.shape[0]), int(pw.shape[2])
    depth = _depth_of(sd)
    fused = "blocks.0.attn.qkv.weight" in sd
    if not fused and "blocks.0.attn.q_proj.weight" not in sd:
        _refuse("missing tensor blocks.0.attn.qkv.weight (or attn.q_proj / k_proj / v_proj)")
    heads = int(heads or (model_args or {}).get("num_heads") or max(dim // HEAD_DIM, 1))
    L = int(sd["pos_embed"].shape[-2])
    grid = int(round((L - 1) ** 0.5))
    if grid * grid + 1 != L:
        _refuse(f"pos_embed has {L} rows: not a square grid plus one cls token")
    if "blocks.0.mlp.fc1_g.weight" in sd:
        hidden = int(sd["blocks.0.mlp.fc1_g.weight"].shape[0])
    elif "blocks.0.mlp.fc1.weight" in sd:
        rows = int(sd["blocks.0.mlp.fc1.weight"].shape[0])
        fc2_in = int(sd["blocks.0.mlp.fc2.weight"].shape[1])
        if rows != 2 * fc2_in:
            _refuse(f"blocks.0.mlp.fc1.weight has {rows} rows for an fc2 of {fc2_in} inputs: not a fused gate | value filter this converter can split "
                    "(a plain GELU Mlp is not built)")
        hidden = fc2_in
    else:
        _refuse("missing tensor blocks.0.mlp.fc1_g.weight (or a fused mlp.fc1.weight)")
    return EvaArch(img=grid * patch, patch=patch, dim=dim, depth=depth, heads=heads, hidden=hidden, classes=int(sd["head.weight"].shape[0]),
                   ref_feat=int(ref_feat), scale_attn_inner="blocks.0.attn.norm.weight" in sd, scale_mlp="blocks.0.mlp.norm.weight" in sd,
                   pool="avg" if "fc_norm.weight" in sd else "token")


def check_arch(sd: Mapping[str, torch.Tensor], arch: EvaArch) -> None:
    """what `arch` (the checkpoint's own, or the caller's) must satisfy to run here"""
    _refuse_post_norm(sd)
    if arch.heads < 1 or arch.dim % arch.heads or arch.dim // arch.heads != HEAD_DIM:
        _refuse(f"head dim {arch.dim // max(arch.heads, 1)}: only head dim 64 is built (dim {arch.dim}, {arch.heads} heads)")
    if arch.pool not in POOLS:
        _refuse(f"unknown pool {arch.pool!r} (token | avg)")
    L = int(sd["pos_embed"].shape[-2])
    if L != arch.tokens:
        _refuse(f"pos_embed holds a grid of {L - 1} patches, img / patch = {arch.grid} wants {arch.grid ** 2} (no resampling is built)")


def fold_state(sd: Mapping[str, torch.Tensor], arch: EvaArch) -> Dict[str, torch.Tensor]:
    """the blob's tensors (fp32): see the module text.  Arithmetic in fp64, rounded once."""
    check_arch(sd, arch)
    D, H, Hp, G = arch.dim, arch.hidden, pad32(arch.hidden), arch.grid
    K, Kp, Cp = 3 * arch.patch ** 2, pad32(3 * arch.patch ** 2), pad32(arch.classes)

    def get(name, shape=None):
        if name not in sd:
            _refuse(f"missing tensor {name}")
        t = torch.as_tensor(sd[name]).detach().to(torch.float64).cpu()
        if shape is not None and tuple(t.shape) != tuple(shape):
            _refuse(f"shape mismatch: {name} is {tuple(t.shape)}, not {tuple(shape)}")
        return t

    def rows_padded(t, rows):          # zero rows below
        out = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=torch.float64)
        out[: t.shape[0]] = t
        return out

    def cols_padded(t, cols):
        out = torch.zeros((t.shape[0], cols), dtype=torch.float64)
        out[:, : t.shape[1]] = t
        return out

    out = {}
    out["patch_embed.weight"] = cols_padded(get("patch_embed.proj.weight", (D, 3, arch.patch, arch.patch)).reshape(D, K), Kp)
    out["patch_embed.bias"] = get("patch_embed.proj.bias", (D,))
    out["cls_token"] = get("cls_token").reshape(-1)
    out["pos_embed"] = get("pos_embed").reshape(-1, D)
    if out["cls_token"].numel() != D or out["pos_embed"].shape[0] != arch.tokens:
        _refuse("shape mismatch: cls_token / pos_embed")
    sin, cos = rope_table(G, arch.ref_feat)
    out["rope_sin"], out["rope_cos"] = sin, cos
    scale = HEAD_DIM ** -0.5
    for i in range(arch.depth):
        b = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            out[b + n + ".weight"], out[b + n + ".bias"] = get(b + n + ".weight", (D,)), get(b + n + ".bias", (D,))
        if b + "attn.qkv.weight" in sd:
            w = get(b + "attn.qkv.weight", (3 * D, D)).clone()
            qb = get(b + "attn.q_bias", (D,)) if b + "attn.q_bias" in sd else torch.zeros(D, dtype=torch.float64)
            vb = get(b + "attn.v_bias", (D,)) if b + "attn.v_bias" in sd else torch.zeros(D, dtype=torch.float64)
        else:
            w = torch.cat([get(b + f"attn.{n}_proj.weight", (D, D)) for n in "qkv"], 0)
            qb = get(b + "attn.q_proj.bias", (D,)) if b + "attn.q_proj.bias" in sd else torch.zeros(D, dtype=torch.float64)
            vb = get(b + "attn.v_proj.bias", (D,)) if b + "attn.v_proj.bias" in sd else torch.zeros(D, dtype=torch.float64)
        w[:D] *= scale
        out[b + "attn.qkv.weight"] = w
        out[b + "attn.qkv.bias"] = torch.cat([qb * scale, torch.zeros(D, dtype=torch.float64), vb])
        if arch.scale_attn_inner:
            out[b + "attn.norm.weight"], out[b + "attn.norm.bias"] = get(b + "attn.norm.weight", (D,)), get(b + "attn.norm.bias", (D,))
        out[b + "attn.proj.weight"], out[b + "attn.proj.bias"] = get(b + "attn.proj.weight", (D, D)), get(b + "attn.proj.bias", (D,))
        if b + "mlp.fc1_g.weight" in sd:
            wg, bg = get(b + "mlp.fc1_g.weight", (H, D)), get(b + "mlp.fc1_g.bias", (H,))
            wx, bx = get(b + "mlp.fc1_x.weight", (H, D)), get(b + "mlp.fc1_x.bias", (H,))
        else:
            w1 = get(b + "mlp.fc1.weight")
            if tuple(w1.shape) != (2 * H, D):
                _refuse(f"{b}mlp.fc1.weight is {tuple(w1.shape)}: not a fused gate | value filter [2 * {H}, {D}] this converter can split")
            b1 = get(b + "mlp.fc1.bias", (2 * H,))
            wg, wx, bg, bx = w1[:H], w1[H:], b1[:H], b1[H:]
        out[b + "mlp.fc1.weight"] = torch.cat([rows_padded(wg, Hp), rows_padded(wx, Hp)], 0)
        out[b + "mlp.fc1.bias"] = torch.cat([rows_padded(bg, Hp), rows_padded(bx, Hp)], 0)
        if arch.scale_mlp:
            out[b + "mlp.norm.weight"] = rows_padded(get(b + "mlp.norm.weight", (H,)), Hp)
            out[b + "mlp.norm.bias"] = rows_padded(get(b + "mlp.norm.bias", (H,)), Hp)
        out[b + "mlp.fc2.weight"] = cols_padded(get(b + "mlp.fc2.weight", (D, H)), Hp)
        out[b + "mlp.fc2.bias"] = get(b + "mlp.fc2.bias", (D,))
    fn = "fc_norm" if arch.pool == "avg" else "norm"
    out["final_norm.weight"], out["final_norm.bias"] = get(fn + ".weight", (D,)), get(fn + ".bias", (D,))
    out["head.weight"] = rows_padded(get("head.weight", (arch.classes, D)), Cp)
    out["head.bias"] = rows_padded(get("head.bias", (arch.classes,)), Cp)
    return {k: v.to(torch.float32).contiguous() for k, v in out.items()}


def make_blob(path_or_dict, arch: EvaArch = None) -> Tuple[EvaArch, bytes]:
    sd = state_dict_of(path_or_dict)
    arch = arch or guess_arch(sd)
    return arch, pack_blob(fold_state(sd, arch))


# ---------------------------------------------------------------------------------------------------------------- blob cache
def _cache_path(source: str):
    """the packed-blob cache of weights.py, keyed by the file (path, size, mtime) and the text of this module (the folding rules)"""
    import hashlib
    d = _cache_dir()
    if not d or not os.path.exists(source):
        return None
    st = os.stat(source)
    with open(os.path.abspath(__file__), "rb") as f:
        rules = hashlib.sha256(f.read()).hexdigest()[:16]
    key = hashlib.sha256(f"eva|{os.path.abspath(source)}|{st.st_size}|{st.st_mtime_ns}|{rules}|v{BLOB_VERSION}".encode()).hexdigest()[:32]
    return os.path.join(d, key + ".rtdw")


def cached_blob(path: str) -> Tuple[EvaArch, bytes]:
    """(arch, blob) of a checkpoint file: from the cache when present and intact, else folded and stored for the next process.  The arch
    travels beside the blob as JSON.  Any cache trouble falls back to building: the cache is an optimisation."""
    import tempfile
    cp = _cache_path(os.fspath(path))
    if cp and os.path.exists(cp) and os.path.exists(cp + ".json"):
        try:
            with open(cp, "rb") as f:
                blob = f.read()
            with open(cp + ".json") as f:
                arch = EvaArch(**json.load(f))
            if blob[:4] == BLOB_MAGIC and len(blob) >= 12:
                unpack_blob(blob)
                return arch, blob
        except Exception:
            pass
    arch, blob = make_blob(path)
    if cp:
        try:
            os.makedirs(os.path.dirname(cp), exist_ok=True)
            for target, payload, mode in ((cp + ".json", json.dumps(asdict(arch)).encode(), "wb"), (cp, blob, "wb")):
                fd, tmp = tempfile.mkstemp(dir=os.path.dirname(cp), suffix=".tmp")
                with os.fdopen(fd, mode) as f:
                    f.write(payload)
                os.replace(tmp, target)
        except OSError:
            pass
    return arch, blob
