"""YOLOX post-processing on the GPU, and the reference's `YOLOXDetector` (src/yolox_detector.py) around it.

The reference calls upstream's `yolox.utils.postprocess`, which calls `torchvision.ops.batched_nms`; torchvision does not exist on this
stack.  Here the whole post-processing - class maximum, confidence threshold, ranking, per-class NMS, and optionally the head's grid
decode - is four HIP launches per batch on the caller's stream (csrc/yolox_post.hip, rtd_yolox_post_* in include/rtdetr_mi355.h),
restated in tests/yolox_ref.py.

* `DeviceBackend(device, num_classes, max_batch, max_anchors, max_candidates=2048)`: one rtd_yolox_post handle.  `run(pred, conf, nms,
  decode=False, in_hw=None, class_keep=None)` -> `(rows, counts)` as device tensors: rows [n][max_candidates][7] (x1, y1, x2, y2, obj,
  class_conf, class_id; only the first counts[i][0] of image i are written), counts [n][2] (kept, passed).
* `YOLOXDetector`: the reference's constructor keywords, attributes and methods, plus `model=None, backend=None, decode=False`.  The
  NETWORK is a pluggable callable from a [B, 3, H, W] float batch to [B, A, 5 + C] (with `decode=True`: the head's undecoded output);
  without an injected model it is chosen by `network`: "auto" builds upstream's PyTorch model through `yolox.exp.get_exp` as the
  reference does where that package is importable, and otherwise this library's network (yolox_network.YoloxNetwork, csrc/yolox_net.hip)
  from the checkpoint at `model_path`; "mi355" always takes this library's network.  With it load_model() sets `decode = True` and
  `num_classes` from the checkpoint.  A checkpoint that does not exist, cannot be read or is refused makes load_model() log one error
  and return False before any device call.
  `frontend`: "auto" (default) hands uint8 [h][w][3] frames - numpy or device tensors, at their native sizes - to this library's network as
  they are (YoloxNetwork.run_frames: the resize happens inside the kernel that writes the Focus map); float, CHW and 4-d frames, an
  injected `model=` and upstream's torch model go through `preprocess()` as in the reference.  "torch" always takes `preprocess()`;
  "mi355" always takes the fused path, refuses an injected model at construction and raises for a frame the kernel cannot read.
* `install()`: sets this class on the module `src.yolox_detector` (the reference imports it function-locally).
"""
from __future__ import annotations

import ctypes as C
import logging
import sys
import time
from typing import Any, Dict, Iterable, List, Optional, Union

import numpy as np

from . import _capi
from .coco_constants import COCO_CLASSES, MAMMAL_CLASS_IDS, WILDLIFE_CLASSES

logger = logging.getLogger(__name__)

ROW = 7


def anchors(in_h: int, in_w: int) -> int:
    """rtd_yolox_anchors: the anchors of an in_h x in_w input (strides 8, 16, 32); raises RtdError for a size that is no multiple of 32"""
    L = _capi.lib()
    out = C.c_int32(0)
    rc = L.rtd_yolox_anchors(int(in_h), int(in_w), C.byref(out))
    if rc != _capi.RTD_OK:
        raise _capi.RtdError(rc, (L.rtd_yolox_post_last_error(None) or b"").decode(errors="replace"))
    return int(out.value)


def keep_words(num_classes: int, class_keep: Optional[Iterable[int]]):
    """class ids -> the ceil(C / 32) words of rtd_yolox_post_params.class_keep (None: every class)"""
    if class_keep is None:
        return None
    words = [0] * ((int(num_classes) + 31) // 32)
    for c in class_keep:
        if 0 <= int(c) < num_classes:
            words[int(c) >> 5] |= 1 << (int(c) & 31)
    return (C.c_uint32 * len(words))(*words)


class DeviceBackend(_capi.Handle):
    """One rtd_yolox_post handle.  A test may hand YOLOXDetector another object with the same run() (tests/yolox_ref.py RefBackend)."""

    _prefix, _what = "rtd_yolox_post", "the YOLOX post-processing"

    def __init__(self, device, num_classes: int, max_batch: int, max_anchors: int, max_candidates: int = 2048):
        if isinstance(device, str):                            # "cuda", "cuda:1"
            device = int(device.split(":")[1]) if ":" in device else 0
        self.device = _capi.device_index(device)
        self.num_classes, self.max_batch, self.max_anchors, self.max_candidates = int(num_classes), int(max_batch), int(max_anchors), int(max_candidates)
        cfg = _capi.RtdYoloxPostConfig()
        cfg.struct_size = C.sizeof(_capi.RtdYoloxPostConfig)
        cfg.device, cfg.num_classes, cfg.max_batch = self.device, self.num_classes, self.max_batch
        cfg.max_anchors, cfg.max_candidates = self.max_anchors, self.max_candidates
        self._open(C.byref(cfg))

    def params(self, conf: float, nms: float, decode: bool = False, in_hw=None, class_keep=None) -> _capi.RtdYoloxPostParams:
        p = _capi.RtdYoloxPostParams()
        p.struct_size = C.sizeof(_capi.RtdYoloxPostParams)
        p.conf_threshold, p.nms_threshold, p.decode = float(conf), float(nms), int(bool(decode))
        if in_hw is not None:
            p.in_h, p.in_w = int(in_hw[0]), int(in_hw[1])
        words = keep_words(self.num_classes, class_keep)
        if words is not None:
            p.class_keep = C.cast(words, C.POINTER(C.c_uint32))
            p._keep_alive = words
        return p

    def run_raw(self, n: int, pred_ptr, n_anchors: int, params, rows_ptr, counts_ptr, stream: int) -> int:
        """rtd_yolox_post_run as it is: the return code"""
        return self._L.rtd_yolox_post_run(self._h, int(n), C.c_void_p(pred_ptr), int(n_anchors), C.byref(params) if params is not None else None,
                                          C.c_void_p(rows_ptr), C.c_void_p(counts_ptr), C.c_void_p(int(stream) or None))

    def run(self, pred, conf: float, nms: float, decode: bool = False, in_hw=None, class_keep=None, out=None):
        """pred: a device fp32 tensor [n][A][5 + C] (contiguous, at any 4-byte address).  Enqueued on torch's current stream: `rows` and
        `counts` are ready when that stream reaches them.  `out`: (rows, counts) tensors to write into instead of fresh ones."""
        import torch

        assert pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 3 and pred.is_contiguous(), "pred: a contiguous device fp32 [n][A][5 + C]"
        n, A, F = (int(v) for v in pred.shape)
        if F != 5 + self.num_classes:
            raise ValueError(f"pred has {F} floats per row; {self.num_classes} classes need {5 + self.num_classes}")
        if out is None:
            rows = torch.empty((max(n, 1), self.max_candidates, ROW), dtype=torch.float32, device=pred.device)
            counts = torch.empty((max(n, 1), 2), dtype=torch.int32, device=pred.device)
        else:
            rows, counts = out
        stream = torch.cuda.current_stream(pred.device).cuda_stream
        self._check(self.run_raw(n, pred.data_ptr(), A, self.params(conf, nms, decode, in_hw, class_keep), rows.data_ptr(), counts.data_ptr(), stream))
        return rows, counts


def _to_numpy(t) -> np.ndarray:
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


class YOLOXDetector:
    """Fast YOLOX detector for Stage 1 detection: the reference's class with the post-processing on the GPU.

    `model`: the network, a callable [B, 3, H, W] float (BGR, 0..255) -> [B, A, 5 + C]; `decode=True` says it returns the head's undecoded
    output.  `backend`: an object with DeviceBackend's run() (built by load_model when None).  `max_batch` / `max_candidates` size it."""

    def __init__(self, model_name: str = "yolox-s", model_path: str = "models/yolox/yolox_s.pth", device: str = "cuda:0",
                 conf_threshold: float = 0.25, nms_threshold: float = 0.45, input_size: tuple = (640, 640), wildlife_only: bool = True,
                 use_tensorrt: bool = False, model=None, backend=None, decode: bool = False, num_classes: int = 80, max_batch: int = 8,
                 max_candidates: int = 2048, network: str = "auto", frontend: str = "auto"):
        if network not in ("auto", "mi355"):
            raise ValueError(f"network must be 'auto' or 'mi355', not {network!r}")
        if frontend not in ("auto", "torch", "mi355"):
            raise ValueError(f"frontend must be 'auto', 'torch' or 'mi355', not {frontend!r}")
        if frontend == "mi355" and model is not None:
            raise ValueError("frontend='mi355' needs this library's network (rtd_yolox_net_run_frames): it cannot be combined with an injected model=")
        self.model_name = model_name
        self.model_path = model_path
        self.device = device
        self.conf_threshold = conf_threshold
        self.nms_threshold = nms_threshold
        self.input_size = input_size
        self.wildlife_only = wildlife_only
        self.use_tensorrt = use_tensorrt

        self.model = None
        self.exp = None
        self.is_tensorrt = False

        self.decode = bool(decode)
        self.num_classes = int(num_classes)
        self.max_batch = int(max_batch)
        self.max_candidates = int(max_candidates)
        self.network = network
        self.frontend = frontend
        self._injected_model = model
        self._backend = backend
        self._warned_cap = False

    # ------------------------------------------------------------------ load
    def load_model(self, max_retries: int = 3) -> bool:
        """True / False, never raises (the reference's contract).  An injected model needs no loading; without one upstream's PyTorch
        model is built as the reference builds it, where the `yolox` package is importable.  TensorRT models are not loaded here."""
        if str(self.device).lower().startswith("cpu") and self._backend is None:      # (an injected back end is the tests' seam)
            logger.error("YOLOX (MI355X): device %r - the post-processing runs on the GPU only", self.device)
            return False
        try:
            if self._injected_model is not None:
                model = self._injected_model
            elif self._wants_own_network():
                model = self._load_own_network()
            else:
                model = self._load_pytorch_model()
            if model is None:
                return False
            if self._backend is None:
                self._backend = DeviceBackend(self.device, self.num_classes, self.max_batch, anchors(*self.input_size), self.max_candidates)
        except Exception as e:
            logger.error("YOLOX (MI355X): cannot load %s: %s", self.model_name, e, exc_info=True)
            return False
        self.model = model
        logger.info("YOLOX (MI355X): %s ready on %s - input %dx%d, %d classes, confidence threshold %.2f, NMS threshold %.2f", self.model_name,
                    self.device, self.input_size[0], self.input_size[1], self.num_classes, self.conf_threshold, self.nms_threshold)
        return True

    def _wants_own_network(self) -> bool:
        if self.network == "mi355" or self.frontend == "mi355":
            return True
        if self.use_tensorrt:
            return False
        try:
            import yolox  # noqa: F401
        except ImportError:
            return True
        return False

    def _load_own_network(self):
        """this library's network from the checkpoint at model_path; the file and its tensor table are checked on the host first"""
        import os

        from . import yolox_network as yn
        if not self.model_path or not os.path.isfile(self.model_path) or not os.access(self.model_path, os.R_OK):
            logger.error("YOLOX (MI355X): no network - the checkpoint %r does not exist or cannot be read (and no model=... was given)", self.model_path)
            return None
        try:
            state = yn.state_dict_of(self.model_path)
            variant = yn.variant_of(self.model_name, state)
            yn.fold_tensors(state, variant)                      # every tensor present and of its shape
        except Exception as e:
            logger.error("YOLOX (MI355X): the checkpoint %r is refused: %s", self.model_path, e)
            return None
        net = yn.YoloxNetwork(state, self.model_name, device=self.device, input_size=self.input_size, max_batch=self.max_batch)
        self.decode = True
        self.num_classes = net.num_classes
        return net

    def _load_pytorch_model(self):
        """upstream's model as src/yolox_detector.py:_load_pytorch_model builds it (not exercised where `yolox` is absent)"""
        if self.use_tensorrt:
            logger.error("YOLOX (MI355X): TensorRT models cannot be loaded on this stack; pass model=... or a PyTorch checkpoint")
            return None
        try:
            from yolox.exp import get_exp
        except ImportError:
            logger.error("YOLOX (MI355X): no network - the `yolox` package is not importable and no model=... was given")
            return None
        import torch
        self.exp = get_exp(None, self.model_name)
        self.exp.test_size = self.input_size
        self.num_classes = int(self.exp.num_classes)
        model = self.exp.get_model()
        ckpt = torch.load(self.model_path, map_location="cpu")
        model.load_state_dict(ckpt["model"])
        model.to(self.device)
        model.eval()
        if self.decode:
            model.head.decode_in_inference = False
        return model

    # ------------------------------------------------------------------ the reference's pre-processing (src/yolox_detector.py:186-220)
    def preprocess(self, img):
        import torch
        if isinstance(img, torch.Tensor):
            img_tensor = img.permute(2, 0, 1).unsqueeze(0).float()
            target_device = torch.device(self.device)
            if img_tensor.device != target_device:
                img_tensor = img_tensor.to(target_device)
        else:
            img_tensor = torch.from_numpy(img).permute(2, 0, 1).unsqueeze(0).float()
            img_tensor = img_tensor.to(self.device)
        if img_tensor.shape[2:] != self.input_size:
            img_tensor = torch.nn.functional.interpolate(img_tensor, size=self.input_size, mode="bilinear", align_corners=False)
        return img_tensor

    # ------------------------------------------------------------------ the reference's formatting (:222-282)
    def _format_model_output_to_detections(self, output: np.ndarray, orig_h: int, orig_w: int) -> List[Dict[str, Any]]:
        detections = []
        ratio_h = orig_h / self.input_size[0]
        ratio_w = orig_w / self.input_size[1]
        for detection in output:
            x1, y1, x2, y2, obj_conf, class_conf, class_id = detection
            x1 = float(x1 * ratio_w)
            y1 = float(y1 * ratio_h)
            x2 = float(x2 * ratio_w)
            y2 = float(y2 * ratio_h)
            class_id = int(class_id)
            confidence = float(obj_conf * class_conf)
            if self.wildlife_only and not self.is_wildlife_relevant(class_id):      # (already dropped before the NMS: class_keep)
                continue
            class_name = COCO_CLASSES[class_id] if class_id < len(COCO_CLASSES) else f"class_{class_id}"
            box_area = int((x2 - x1) * (y2 - y1))
            detections.append({"class_id": class_id, "class_name": class_name, "confidence": confidence,
                               "bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2, "area": box_area}})
        return detections

    # ------------------------------------------------------------------ detection
    def _postprocess(self, outputs) -> List[np.ndarray]:
        """one back-end call for the batch, one download of the counts and the rows: per image its kept rows [k][7]"""
        n = int(outputs.shape[0])
        keep = sorted(WILDLIFE_CLASSES) if self.wildlife_only else None
        rows, counts = self._backend.run(outputs, float(self.conf_threshold), float(self.nms_threshold), decode=self.decode,
                                         in_hw=tuple(self.input_size), class_keep=keep)
        counts = _to_numpy(counts)
        rows = _to_numpy(rows)
        cap = int(rows.shape[1])
        if not self._warned_cap and any(int(counts[i][1]) > cap for i in range(n)):
            self._warned_cap = True
            logger.warning("YOLOX (MI355X): %d rows passed the confidence threshold in one image; only the best %d enter the NMS "
                           "(max_candidates) - the reference has no such cap", int(max(counts[i][1] for i in range(n))), cap)
        return [rows[i, :int(counts[i][0])] for i in range(n)]

    def _run_model(self, batch):
        import torch
        with torch.no_grad():
            out = self.model(batch)
        return out.float().contiguous() if hasattr(out, "contiguous") else out

    # ------------------------------------------------------------------ the fused front end (YoloxNetwork.run_frames)
    def _takes_fused_path(self, frames) -> bool:
        """True: these frames go to the network as their uint8 bytes (one kernel resizes them and writes the Focus map); False: through
        preprocess().  "auto" asks for this library's own network (not an injected model) and uint8 [h][w][3] frames throughout; "mi355"
        raises for anything else instead of falling back."""
        if self.frontend == "torch":
            return False
        from .yolox_network import YoloxNetwork, is_u8_frame
        own = self._injected_model is None and isinstance(self.model, YoloxNetwork)
        fits = all(is_u8_frame(f) for f in frames)
        if self.frontend == "mi355" and not (own and fits):
            raise ValueError("frontend='mi355' takes uint8 [h][w][3] frames and this library's network; use frontend='auto' for float or CHW frames")
        return own and fits

    def _run_frames(self, frames):
        import torch
        with torch.no_grad():
            return self.model.run_frames(frames, self.input_size)

    def detect(self, frame) -> List[Dict[str, Any]]:
        if self.model is None:
            logger.error("Model not loaded")
            return []
        orig_h, orig_w = frame.shape[:2]
        if self._takes_fused_path([frame]):
            output = self._postprocess(self._run_frames([frame]))[0]
        else:
            output = self._postprocess(self._run_model(self.preprocess(frame)))[0]
        return self._format_model_output_to_detections(output, orig_h, orig_w)

    def detect_batch(self, frames: List) -> List[List[Dict[str, Any]]]:
        import torch
        if self.model is None:
            logger.error("Model not loaded")
            return [[] for _ in frames]
        if not frames:
            return []
        orig_sizes = []
        for frame in frames:
            if isinstance(frame, torch.Tensor):
                if frame.ndim == 3:
                    if frame.shape[0] in (1, 3):
                        h, w = frame.shape[1], frame.shape[2]
                    else:
                        h, w = frame.shape[0], frame.shape[1]
                elif frame.ndim == 4:
                    if frame.shape[1] in (1, 3):
                        h, w = frame.shape[2], frame.shape[3]
                    else:
                        h, w = frame.shape[1], frame.shape[2]
                else:
                    raise ValueError(f"Unexpected tensor dimensions: {frame.shape}")
            else:
                h, w = frame.shape[0], frame.shape[1]
            orig_sizes.append((h, w))
        fused = self._takes_fused_path(frames)
        batch_tensor = None if fused else torch.cat([self.preprocess(frame) for frame in frames], dim=0)
        all_detections: List[List[Dict[str, Any]]] = []
        step = max(1, int(getattr(self._backend, "max_batch", len(frames))))
        for i0 in range(0, len(frames), step):                 # larger lists run as several device batches
            outputs = self._postprocess(self._run_frames(frames[i0:i0 + step]) if fused else self._run_model(batch_tensor[i0:i0 + step]))
            for k, output in enumerate(outputs):
                orig_h, orig_w = orig_sizes[i0 + k]
                all_detections.append(self._format_model_output_to_detections(output, orig_h, orig_w))
        del batch_tensor
        return all_detections

    def is_wildlife_relevant(self, class_id: int) -> bool:
        return class_id in WILDLIFE_CLASSES

    def get_class_category(self, class_id: int) -> str:
        if class_id == 0:
            return "person"
        elif class_id == 14:
            return "bird"
        elif class_id in MAMMAL_CLASS_IDS:
            return "mammal"
        else:
            return "other"

    def close(self) -> None:
        if self._backend is not None and hasattr(self._backend, "close"):
            self._backend.close()
        if self._injected_model is None and hasattr(self.model, "close"):
            self.model.close()
            self.model = None


def install() -> None:
    """Let the reference build this detector without editing it: `main.py` and the engine import `YOLOXDetector` from `src.yolox_detector`
    function-locally, so the class is set on that module in sys.modules (import it first; where upstream's YOLOX tree is absent the
    reference's module cannot be imported at all - place a module of that name there instead)."""
    mod = sys.modules.get("src.yolox_detector")
    if mod is None:
        raise RuntimeError("src.yolox_detector is not imported: import it (or place a module of that name in sys.modules) before install()")
    mod.YOLOXDetector = YOLOXDetector
