"""The YOLOX network on the GPU: upstream's `YOLOX(YOLOPAFPN(CSPDarknet), YOLOXHead)` on this library's conv kernels
(csrc/yolox_net.hip, rtd_yolox_net_* in include/rtdetr_mi355.h), from an upstream checkpoint (`yolox_s.pth`, `yolox_l.pth`).

`YoloxNetwork` owns one rtd_yolox_net handle and is the callable `YOLOXDetector` wants as its model: a [B, 3, H, W] float batch (BGR,
0..255, the reference's `preprocess` output) -> the head's undecoded rows [B, A, 5 + C] on torch's current stream, which the
post-processing back end reads with `decode=True`.  `run_frames` takes the camera frames themselves - uint8 HWC, each at its own size -
and does the reference's resize inside the kernel that writes the Focus map (rtd_yolox_net_run_frames).  The architecture, the
state-dict keys and BatchNorm's eps of 1e-3 (upstream's
`Exp.get_model` sets it; a checkpoint does not carry it) are restated from upstream's public source in tests/yolox_net_ref.py.

Served: yolox-s and yolox-l (every channel count a multiple of 32).  yolox-m, -x, -tiny (widths 48, 80, 24) and the depthwise nano are
refused with the reason.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

from . import _capi

BN_EPS = 1e-3
FOCUS_C = 32
STRIDES = (8, 16, 32)
# model name -> (depth factor, width factor), upstream's exps/default/*.py
FACTORS = {"yolox-s": (0.33, 0.50), "yolox-m": (0.67, 0.75), "yolox-l": (1.0, 1.0), "yolox-x": (1.33, 1.25), "yolox-tiny": (0.33, 0.375),
           "yolox-nano": (0.33, 0.25)}


class Variant(NamedTuple):
    name: str
    base: int            # int(64 * width)
    depth: int           # max(round(3 * depth), 1): the bottlenecks of dark2's CSP layer
    num_classes: int


def _err(msg: str):
    return _capi.RtdError(_capi.RTD_E_INVALID, msg)


def csp_table(prefix: str, cin: int, cout: int, n: int) -> List[Tuple[str, int, int, int, int]]:
    h = cout // 2
    t = [(prefix + ".conv1", cin, h, 1, 1), (prefix + ".conv2", cin, h, 1, 1)]
    for i in range(n):
        t += [(f"{prefix}.m.{i}.conv1", h, h, 1, 1), (f"{prefix}.m.{i}.conv2", h, h, 3, 1)]
    return t + [(prefix + ".conv3", 2 * h, cout, 1, 1)]


def conv_table(base: int, depth: int) -> List[Tuple[str, int, int, int, int]]:
    """(state-dict prefix, Cin, Cout, k, stride) of every BaseConv of the network in execution order (yolox_net_host.h conv_table
    without the head's pred convs, and with the stem's real 12 input channels)"""
    bb, fp = "backbone.backbone.", "backbone."
    t = [(bb + "stem.conv", 12, base, 3, 1)]
    units = (depth, 3 * depth, 3 * depth, depth)
    for s in range(4):
        d, cin, cout = f"{bb}dark{s + 2}", base << s, base << (s + 1)
        t.append((d + ".0", cin, cout, 3, 2))
        if s == 3:
            t += [(d + ".1.conv1", cout, cout // 2, 1, 1), (d + ".1.conv2", 2 * cout, cout, 1, 1)] + csp_table(d + ".2", cout, cout, units[s])
        else:
            t += csp_table(d + ".1", cout, cout, units[s])
    c3, c4, c5 = 4 * base, 8 * base, 16 * base
    t.append((fp + "lateral_conv0", c5, c4, 1, 1))
    t += csp_table(fp + "C3_p4", 2 * c4, c4, depth)
    t.append((fp + "reduce_conv1", c4, c3, 1, 1))
    t += csp_table(fp + "C3_p3", 2 * c3, c3, depth)
    t.append((fp + "bu_conv2", c3, c3, 3, 2))
    t += csp_table(fp + "C3_n3", 2 * c3, c4, depth)
    t.append((fp + "bu_conv1", c4, c4, 3, 2))
    t += csp_table(fp + "C3_n4", 2 * c4, c5, depth)
    hc = 4 * base
    for l, c in enumerate((c3, c4, c5)):
        t.append((f"head.stems.{l}", c, hc, 1, 1))
        t += [(f"head.cls_convs.{l}.{j}", hc, hc, 3, 1) for j in range(2)] + [(f"head.reg_convs.{l}.{j}", hc, hc, 3, 1) for j in range(2)]
    return t


def _count(state, fmt: str) -> int:
    n = 0
    while fmt.format(n) in state:
        n += 1
    return n


def variant_of(model_name: str, state: Dict[str, object]) -> Variant:
    """depth, width and C of `model_name` ("yolox-s", "yolox_s", "yolox-l", ...), which the state dict's shapes must agree with.  Raises
    RtdError (RTD_E_INVALID) with the reason for a mismatch and for a variant that is not served."""
    name = str(model_name).lower().replace("_", "-")
    if name not in FACTORS:
        raise _err(f"unknown YOLOX model {model_name!r} (one of {', '.join(sorted(FACTORS))})")
    depth_f, width_f = FACTORS[name]
    base, depth = int(64 * width_f), max(round(3 * depth_f), 1)
    if name == "yolox-nano":
        raise _err("yolox-nano is not served: its convolutions are depthwise (and its base width is 16 channels, no multiple of 32)")
    if base % 32:
        raise _err(f"{name} is not served: its base width is {base} channels, and every channel count must be a multiple of 32 (served: yolox-s, yolox-l)")
    for key in ("backbone.backbone.stem.conv.conv.weight", "head.cls_preds.0.weight"):
        if key not in state:
            raise _err(f"the state dict has no {key}: not a YOLOX checkpoint")
    got_base = int(state["backbone.backbone.stem.conv.conv.weight"].shape[0])
    if got_base != base:
        raise _err(f"{name} has a base width of {base} channels, the checkpoint's stem has {got_base}")
    got_depth = _count(state, "backbone.backbone.dark2.1.m.{}.conv1.conv.weight")
    if got_depth != depth or _count(state, "backbone.backbone.dark3.1.m.{}.conv1.conv.weight") != 3 * depth:
        raise _err(f"{name} has {depth} bottlenecks in dark2 and {3 * depth} in dark3, the checkpoint {got_depth} and "
                   f"{_count(state, 'backbone.backbone.dark3.1.m.{}.conv1.conv.weight')}")
    return Variant(name, base, depth, int(state["head.cls_preds.0.weight"].shape[0]))


def state_dict_of(path_or_dict) -> Dict[str, object]:
    """upstream's checkpoints keep the model under "model"; a plain state dict is taken as it is.  Files are read with weights-only
    loading onto the CPU."""
    import torch

    sd = path_or_dict
    if not isinstance(sd, dict):
        sd = torch.load(os.fspath(path_or_dict), map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise _capi.RtdError(_capi.RTD_E_WEIGHTS, "checkpoint is not a dict")
    if isinstance(sd.get("model"), dict):
        return sd["model"]
    return sd


def fold_tensors(state: Dict[str, object], variant: Variant) -> Dict[str, "object"]:
    """The tensors of the blob, as fp64 (fold_state rounds them to fp32 once): per conv `name`.weight [cout][k][k][cin] - BatchNorm folded
    into filter and bias with eps 1e-3, tap-major and channel-minor as launch_conv reads a filter row - and `name`.bias [cout].  The
    Focus filter is zero-padded to 32 input channels; reg_preds.<l> and obj_preds.<l> are stacked into head.regobj_preds.<l>."""
    import torch

    def get(key, shape):
        t = state.get(key)
        if t is None:
            raise _capi.RtdError(_capi.RTD_E_WEIGHTS, f"missing tensor {key}")
        t = torch.as_tensor(t).detach().cpu()
        if tuple(t.shape) != tuple(shape):
            raise _capi.RtdError(_capi.RTD_E_WEIGHTS, f"shape mismatch: {key} is {tuple(t.shape)}, not {tuple(shape)}")
        return t.double()

    out = {}
    for name, cin, cout, k, _ in conv_table(variant.base, variant.depth):
        w = get(name + ".conv.weight", (cout, cin, k, k))
        g, b, m, v = (get(f"{name}.bn.{s}", (cout,)) for s in ("weight", "bias", "running_mean", "running_var"))
        scale = g / torch.sqrt(v + BN_EPS)
        w = (w * scale[:, None, None, None]).permute(0, 2, 3, 1)
        if cin == 12:
            w = torch.cat([w, torch.zeros((cout, k, k, FOCUS_C - cin), dtype=torch.float64)], 3)
        out[name + ".weight"], out[name + ".bias"] = w.contiguous(), (b - m * scale).contiguous()
    hc, C_ = 4 * variant.base, variant.num_classes
    for l in range(3):
        out[f"head.cls_preds.{l}.weight"] = get(f"head.cls_preds.{l}.weight", (C_, hc, 1, 1)).permute(0, 2, 3, 1).contiguous()
        out[f"head.cls_preds.{l}.bias"] = get(f"head.cls_preds.{l}.bias", (C_,))
        w = torch.cat([get(f"head.reg_preds.{l}.weight", (4, hc, 1, 1)), get(f"head.obj_preds.{l}.weight", (1, hc, 1, 1))], 0)
        out[f"head.regobj_preds.{l}.weight"] = w.permute(0, 2, 3, 1).contiguous()
        out[f"head.regobj_preds.{l}.bias"] = torch.cat([get(f"head.reg_preds.{l}.bias", (4,)), get(f"head.obj_preds.{l}.bias", (1,))], 0)
    return out


def fold_state(state: Dict[str, object], variant: Variant) -> bytes:
    """the weight blob rtd_yolox_net_create reads (fold_tensors, rounded to fp32, packed)"""
    import torch

    from .weights import pack_blob

    return pack_blob({k: t.to(torch.float32).contiguous() for k, t in fold_tensors(state, variant).items()})


def anchors(in_h: int, in_w: int) -> int:
    return sum((int(in_h) // s) * (int(in_w) // s) for s in STRIDES)


def is_u8_frame(f) -> bool:
    """a uint8 [h][w][3] numpy array or torch tensor: what run_frames (and YOLOXDetector's fused front end) takes"""
    shape = getattr(f, "shape", None)
    return shape is not None and len(shape) == 3 and int(shape[2]) == 3 and str(getattr(f, "dtype", "")) in ("uint8", "torch.uint8")


def frame_arrays(ptrs, hw):
    """the two host arrays of rtd_yolox_net_run_frames / rtd_op_yolox_focus_u8: device addresses and (h, w) pairs (None stays a null array)"""
    frames = None if ptrs is None else (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(int(p) or None) for p in ptrs])
    sizes = None if hw is None else (C.c_int32 * max(2 * len(hw), 1))(*[int(v) for s in hw for v in s])
    return frames, sizes


class YoloxNetwork(_capi.Handle):
    """One rtd_yolox_net handle.  state_or_path: a checkpoint path or a state dict.  Calls are asynchronous on torch's current stream; the
    handle's arena belongs to the call in flight, so use one network from one stream at a time."""

    _prefix, _what = "rtd_yolox_net", "the YOLOX network"
    decode = True        # the rows are the head's undecoded output: post-process them with decode = 1

    def __init__(self, state_or_path, model_name: str = "yolox-s", device=0, input_size=(640, 640), max_batch: int = 8, precision="f16x3"):
        state = state_dict_of(state_or_path)
        self.variant = variant_of(model_name, state)
        self.num_classes = self.variant.num_classes
        self.input_size = (int(input_size[0]), int(input_size[1]))
        if isinstance(device, str):                            # "cuda", "cuda:1"
            if not device.lower().startswith("cuda"):
                raise _err(f"device {device!r}: the YOLOX network runs on the GPU only")
            device = int(device.split(":")[1]) if ":" in device else 0
        self.device, self.max_batch = _capi.device_index(device), int(max_batch)
        cfg = _capi.RtdYoloxNetConfig()
        cfg.struct_size = C.sizeof(_capi.RtdYoloxNetConfig)
        cfg.device, cfg.precision, cfg.num_classes = self.device, _capi.precision_code(precision), self.num_classes
        cfg.base_channels, cfg.depth, cfg.max_batch = self.variant.base, self.variant.depth, self.max_batch
        self.precision = cfg.precision
        blob = fold_state(state, self.variant)
        self._open(C.byref(cfg), (C.c_char * len(blob)).from_buffer_copy(blob), len(blob))

    def run_raw(self, n: int, in_ptr, in_h: int, in_w: int, pred_ptr, stream: int) -> int:
        """rtd_yolox_net_run as it is: the return code"""
        return self._L.rtd_yolox_net_run(self._h, int(n), C.c_void_p(in_ptr), int(in_h), int(in_w), C.c_void_p(pred_ptr), C.c_void_p(int(stream) or None))

    def __call__(self, batch):
        """batch: a device float [B, 3, H, W] tensor (H, W multiples of 32) -> a fresh contiguous fp32 [B, A, 5 + C] device tensor, enqueued
        on torch's current stream.  Batches above max_batch run as several calls."""
        import torch

        assert batch.is_cuda and batch.dim() == 4 and batch.shape[1] == 3, "batch: a device [B, 3, H, W] tensor"
        x = batch.to(torch.float32).contiguous()
        B, _, H, W = (int(v) for v in x.shape)
        pred = torch.empty((B, anchors(H, W), 5 + self.num_classes), dtype=torch.float32, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        for i0 in range(0, B, self.max_batch):
            k = min(self.max_batch, B - i0)
            self._check(self.run_raw(k, x[i0].data_ptr(), H, W, pred[i0].data_ptr(), stream))
        return pred

    def run_frames_raw(self, n: int, ptrs, hw, in_h: int, in_w: int, pred_ptr, stream: int) -> int:
        """rtd_yolox_net_run_frames as it is: the return code.  ptrs: the frames' device addresses, hw: their (h, w); None: a null array"""
        frames, sizes = frame_arrays(ptrs, hw)
        return self._L.rtd_yolox_net_run_frames(self._h, int(n), frames, sizes, int(in_h), int(in_w), C.c_void_p(pred_ptr), C.c_void_p(int(stream) or None))

    def run_frames(self, frames, input_size=None):
        """frames: uint8 [h][w][3] BGR numpy arrays or tensors, each at its own size -> a fresh contiguous fp32 [B, A, 5 + C] device tensor
        for `input_size` (default: the network's), enqueued on torch's current stream: the reference's `preprocess` (bilinear,
        align_corners=False) and the Focus map in one kernel, from the bytes.  A numpy frame is uploaded as uint8, one copy; a tensor on the
        network's device is read in place.  Lists above max_batch run as several calls."""
        import torch

        H, W = (int(v) for v in (input_size if input_size is not None else self.input_size))
        dev = torch.device("cuda", self.device)
        held = []
        for f in frames:
            if not is_u8_frame(f):
                raise TypeError(f"run_frames takes uint8 [h][w][3] arrays or tensors, not {type(f).__name__} {getattr(f, 'dtype', '')} {tuple(getattr(f, 'shape', ()))}")
            t = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))
            held.append(t.to(dev).contiguous())
        B = len(held)
        pred = torch.empty((B, anchors(H, W), 5 + self.num_classes), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for i0 in range(0, B, self.max_batch):
            part = held[i0:i0 + self.max_batch]
            self._check(self.run_frames_raw(len(part), [t.data_ptr() for t in part], [(int(t.shape[0]), int(t.shape[1])) for t in part], H, W,
                                            pred[i0].data_ptr(), stream))
        return pred

    def arena_bytes(self) -> int:
        return int(self._L.rtd_yolox_net_arena_bytes(self._h))

    def debug_tensor(self, name: str) -> np.ndarray:
        """rtd_debug_yolox_tensor: a float stage output [n, h, w, c] of the last call"""
        shape = (C.c_int64 * 4)()
        self._check(self._L.rtd_debug_yolox_tensor(self._h, name.encode(), None, 0, shape))
        out = np.zeros(tuple(shape), np.float32)
        self._check(self._L.rtd_debug_yolox_tensor(self._h, name.encode(), out.ctypes.data, out.size, shape))
        return out
