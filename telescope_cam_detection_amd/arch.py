"""RT-DETRv2 architecture descriptors (R18 / R34 / R50 / R101).

The reference never spells the network out: `src/rtdetr_detector.py:132` hands a YAML
path to the un-vendored lyuwenyu/RT-DETR `YAMLConfig`.  The hyper-parameters below are
the ones SURVEY.md §8(c) cross-checked against upstream's published parameter / FLOP
counts (20 M / 42 M / 76 M params; 60 / 136 GFLOPs @640²).

An `Arch` is pure data.  It is serialised into `rtd_config` (include/rtdetr_mi355.h) for
the HIP engine and drives the weight recipe / packer (weights.py) and the CPU oracle
(oracle/rtdetr_oracle.py), so all three agree on one description of the graph.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field, replace
from typing import List, Tuple


@dataclass(frozen=True)
class Arch:
    name: str
    # PResNet-vd backbone (HF:rt_detr/modeling_rt_detr_resnet.py:71-310)
    layer_type: str                      # "basic" | "bottleneck"
    depths: Tuple[int, int, int, int]
    hidden_sizes: Tuple[int, int, int, int]
    embedding_size: int = 64
    # hybrid encoder (HF:rt_detr_v2/modeling_rt_detr_v2.py:1098-1209)
    enc_dim: int = 256
    enc_ffn: int = 1024
    enc_heads: int = 8
    expansion: float = 1.0               # CSPRep hidden = int(enc_dim * expansion)
    # decoder (HF:...v2.py:555-661, 1339-1623)
    d_model: int = 256
    dec_ffn: int = 1024
    dec_heads: int = 8
    dec_layers: int = 6
    num_queries: int = 300
    num_classes: int = 80
    n_levels: int = 3
    n_points: int = 4
    offset_scale: float = 0.5
    feat_strides: Tuple[int, int, int] = (8, 16, 32)
    # cross-attention sampler (upstream `cross_attn_method`, HF `decoder_method`, :44-115): "default" = zero-padded bilinear grid_sample,
    # "discrete" = one clamped nearest tap per point (the "dsp" checkpoints).  Same weight shapes either way.
    dec_method: str = "default"

    @property
    def backbone_out_channels(self) -> Tuple[int, int, int]:
        return tuple(self.hidden_sizes[1:])  # stages 2..4 (out_indices [2,3,4])

    @property
    def csp_hidden(self) -> int:
        return int(self.enc_dim * self.expansion)

    def level_shapes(self, height: int, width: int) -> List[Tuple[int, int]]:
        """(h, w) of the stride-8/16/32 maps for an input of height x width.

        Follows the conv arithmetic of the stem (3x3 s2 p1, maxpool 3x3 s2 p1) and the
        stride-2 stages (3x3 s2 p1 on the main path, AvgPool2d(2,2,ceil) on the shortcut).
        """
        def down(n):  # k=3, s=2, p=1
            return (n + 2 - 3) // 2 + 1
        h, w = down(down(height)), down(down(width))  # stride 4
        out = []
        for _ in range(3):
            h, w = down(h), down(w)
            out.append((h, w))
        return out


ARCHS = {
    "r18": Arch("r18", "basic", (2, 2, 2, 2), (64, 128, 256, 512), expansion=0.5, dec_layers=3),
    "r34": Arch("r34", "basic", (3, 4, 6, 3), (64, 128, 256, 512), expansion=0.5, dec_layers=4),
    "r50": Arch("r50", "bottleneck", (3, 4, 6, 3), (256, 512, 1024, 2048)),
    "r101": Arch("r101", "bottleneck", (3, 4, 23, 3), (256, 512, 1024, 2048), enc_dim=384, enc_ffn=2048),
    # tiny graph-shaped model for fast CPU/GPU unit tests (not a reference variant)
    "tiny": Arch("tiny", "bottleneck", (1, 1, 1, 1), (64, 128, 256, 512), embedding_size=32,
                 enc_dim=64, enc_ffn=128, enc_heads=2, d_model=64, dec_ffn=128, dec_heads=2,
                 dec_layers=2, num_queries=50, expansion=1.0),
    "tinyb": Arch("tinyb", "basic", (1, 1, 1, 1), (32, 64, 128, 256), embedding_size=32,
                  enc_dim=64, enc_ffn=128, enc_heads=2, d_model=64, dec_ffn=128, dec_heads=2,
                  dec_layers=2, num_queries=50, expansion=0.5),
    # a one-block-per-stage R18 trunk with small heads: every trunk width is a whole 32-channel group, which the f16x3 engine's hi/lo
    # layout needs (basic blocks need embedding_size == hidden_sizes[0], HF:rt_detr_resnet.py:150-163)
    "tinyc": Arch("tinyc", "basic", (1, 1, 1, 1), (64, 128, 256, 512), embedding_size=64,
                  enc_dim=64, enc_ffn=128, enc_heads=2, d_model=64, dec_ffn=128, dec_heads=2,
                  dec_layers=2, num_queries=50, expansion=0.5),
}
# the discrete-sampling ("dsp") twins, e.g. upstream's rtdetrv2_r18vd_dsp_3x_coco.yml: the same graph and weight shapes, another sampler.
# They come AFTER the plain entries: a checkpoint's shapes cannot tell the two apart and checkpoint.guess_arch takes the first fit.
DSP_SUFFIX = "_dsp"
ARCHS.update({n + DSP_SUFFIX: replace(ARCHS[n], name=n + DSP_SUFFIX, dec_method="discrete") for n in ("r18", "r34", "r50", "r101", "tinyc")})
# Upstream's speed-tuned members, AFTER every entry above (guess_arch's first fit stays what it was for every checkpoint that fitted before;
# these differ from their base in tensor shapes, so the file tells them apart):
# * rtdetrv2_r50vd_m_7x_coco.yml: the R50 trunk with the half-width CSP blocks (expansion 0.5).  The file trains 6 decoder layers and sets
#   `eval_idx: 2`: inference runs layers 0..2 and reads the heads of index 2, which is a 3-layer decoder; the converters pick only the
#   keys they map, so the stored layers 3..5 are ignored.  (Restated from upstream's public config, unverifiable offline: DESIGN.md §8.)
# * rtdetrv2_r18vd_sp1 / sp2 / sp3_120e_coco.yml: R18 with `num_points: [k, k, k]`, k sampling points per level instead of 4.  Upstream
#   publishes no sp twins of other backbones and no sp + dsp files, so there are no such entries.
ARCHS["r50_m"] = replace(ARCHS["r50"], name="r50_m", expansion=0.5, dec_layers=3)
ARCHS["r50_m" + DSP_SUFFIX] = replace(ARCHS["r50_m"], name="r50_m" + DSP_SUFFIX, dec_method="discrete")
SP_POINTS = (1, 2, 3)
ARCHS.update({f"r18_sp{k}": replace(ARCHS["r18"], name=f"r18_sp{k}", n_points=k) for k in SP_POINTS})


def same_weights(a: Arch, b: Arch) -> bool:
    """the two variants read the same checkpoint: they differ in nothing but the name and the sampler"""
    return replace(a, name="", dec_method="default") == replace(b, name="", dec_method="default")


_DISCRETE_LINE = re.compile(r"^\s*cross_attn_method\s*:\s*[\"']?discrete[\"']?\s*(#.*)?$", re.MULTILINE)


def _config_is_discrete(config_path: str) -> bool:
    """upstream's dsp configs set `cross_attn_method: discrete` on the decoder and carry the tag `dsp` in their file name.  The YAML
    decides when it can be read (a plain text scan: no include is followed); otherwise the name does, `dsp` being one of its
    `_`-delimited tokens (rtdetrv2_r18vd_dsp_3x_coco.yml) - never a part of another word."""
    try:
        if os.path.isfile(config_path):
            with open(config_path, "r", errors="replace") as fh:
                if _DISCRETE_LINE.search(fh.read()):
                    return True
    except OSError:
        pass
    stem = os.path.basename(str(config_path)).lower().split(".")[0]
    return "dsp" in stem.split("_")


class UnsupportedVariant(ValueError):
    """a config that names a network this build has no description of (arch_from_config_path): a refusal, where a plain ValueError
    only says that the path names no variant at all and the checkpoint's shapes may decide"""


_NUM_POINTS_LINE = re.compile(r"^\s*num_points\s*:\s*\[([^\]\n]*)\]\s*(#.*)?$", re.MULTILINE)
_SP_TOKEN = re.compile(r"^sp(\d+)$")


def _config_points(config_path: str, tokens) -> "int | None":
    """the sampling points per level a config asks for, None when it says nothing.  Upstream's sp configs set `num_points: [k, k, k]` on the
    decoder and carry the token `sp<k>` in their file name (rtdetrv2_r18vd_sp2_120e_coco.yml).  As for the sampler, the YAML decides when it
    can be read (a plain text scan), otherwise the name does.  A list that is not uniform raises: per-level counts are not built, and
    serving such a checkpoint with one count for every level must not be silent."""
    try:
        if os.path.isfile(config_path):
            with open(config_path, "r", errors="replace") as fh:
                m = _NUM_POINTS_LINE.search(fh.read())
            if m:
                try:
                    pts = [int(v) for v in m.group(1).split(",") if v.strip()]
                except ValueError:
                    pts = []
                if not pts or len(set(pts)) != 1:
                    raise UnsupportedVariant(f"{config_path!r}: num_points: [{m.group(1).strip()}] - one point count for every level is all this build "
                                     f"serves (per-level counts are not built)")
                return pts[0]
    except OSError:
        pass
    sp = [int(_SP_TOKEN.match(t).group(1)) for t in tokens if _SP_TOKEN.match(t)]
    return sp[0] if sp else None


def arch_from_config_path(config_path: str) -> Arch:
    """Map the reference's `config_path` argument (src/rtdetr_detector.py:31) to a variant.

    The reference passes e.g. "RT-DETR/rtdetrv2_pytorch/configs/rtdetrv2/rtdetrv2_r18vd_120e_coco.yml";
    upstream's file names carry the backbone tag; beside it this build needs the decoder's sampler (`_config_is_discrete`), its point
    count (`_config_points`: the sp1 / sp2 / sp3 files of R18) and the mid-size marker `m` of rtdetrv2_r50vd_m_7x_coco.yml, each one of
    the `_`-delimited tokens of the file stem.  A marker on a backbone upstream publishes no such model for raises: the name asks for a
    network this build has no description of.
    """
    s = str(config_path).lower()
    tokens = os.path.basename(s).split(".")[0].split("_")
    for tag in ("r101", "r50", "r34", "r18", "tinyc", "tinyb", "tiny"):
        if tag in s:
            name = tag
            if "m" in tokens:
                if tag != "r50":
                    raise UnsupportedVariant(f"config_path={config_path!r}: the mid-size variant `m` exists for r50 only")
                name = "r50_m"
            points = _config_points(str(config_path), tokens)
            if points is not None and points != ARCHS[name].n_points:
                if name != "r18" or points not in SP_POINTS:
                    raise UnsupportedVariant(f"config_path={config_path!r}: {points} sampling point(s) per level - the sp variants are "
                                     f"r18 with {', '.join(map(str, SP_POINTS))} points")
                name = f"r18_sp{points}"
            if _config_is_discrete(str(config_path)):
                if points is not None and points != ARCHS[tag].n_points:
                    raise UnsupportedVariant(f"config_path={config_path!r}: no variant has both {points} sampling points and the discrete sampler")
                if name + DSP_SUFFIX in ARCHS:
                    name += DSP_SUFFIX
            return ARCHS[name]
    raise ValueError(f"cannot infer RT-DETR variant from config_path={config_path!r}")
