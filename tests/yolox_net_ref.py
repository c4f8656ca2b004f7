"""Restatement of upstream's YOLOX network - YOLOX(YOLOPAFPN(CSPDarknet(depth, width)), YOLOXHead(C, width)) in eval mode with
decode_in_inference = False - in plain torch, generic in the dtype, so the same code is the fp64 yardstick and the fp32 / fp16 runs it is
compared with.  The state-dict keys are upstream's, so one seeded state dict feeds this file and yolox_network.fold_state.

`yolox` is not importable here and no upstream checkpoint is at hand: the architecture and the key table below are written from the public
source and could NOT be checked against it offline.  Where `yolox` is importable, tests/test_yolox_net_host.py compares.

Arithmetic:
  BaseConv(in, out, k, s) = Conv2d(k, s, pad (k - 1) // 2, no bias) -> BatchNorm2d(eps 1e-3: Exp.get_model sets it, a checkpoint does
  not carry it) -> SiLU; keys .conv.weight, .bn.{weight, bias, running_mean, running_var}.
  Focus: cat(x[::2, ::2], x[1::2, ::2], x[::2, 1::2], x[1::2, 1::2]) (top-left, bottom-left, top-right, bottom-right) -> BaseConv(12, base, 3, 1).
  Bottleneck(c, c, shortcut, expansion 1): y = conv2(conv1(x)) (1x1, 3x3), + x after the SiLU with shortcut.
  CSPLayer(in, out, n, shortcut): h = out // 2; conv3(cat(m(conv1(x)), conv2(x))), m = n Bottlenecks on h channels.
  SPPBottleneck(c, c): conv1 1x1 c -> c / 2; cat(x, pool5, pool9, pool13) with MaxPool2d(k, 1, k // 2); conv2 1x1 2c -> c.
  CSPDarknet: stem; dark2 = [BaseConv(3, 2), CSP(n = d)]; dark3, dark4 = [BaseConv(3, 2), CSP(n = 3d)]; dark5 = [BaseConv(3, 2), SPP,
  CSP(n = d, shortcut=False)], base = int(64 width), d = max(round(3 depth), 1).
  PAFPN and head: see forward() below.  Output [B][A][5 + C]: cat(reg, sigmoid(obj), sigmoid(cls)) per level, levels of stride 8, 16, 32
  flattened row-major over (y, x) and concatenated in that order.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
STRIDES = (8, 16, 32)
VARIANTS = {"yolox-s": (0.33, 0.50), "yolox-l": (1.0, 1.0), "yolox-m": (0.67, 0.75), "yolox-x": (1.33, 1.25), "yolox-tiny": (0.33, 0.375),
            "yolox-nano": (0.33, 0.25)}
STAGES = ("stem", "dark2", "dark3", "dark4", "dark5", "spp", "fpn_out0", "fpn_out1", "pan_out2", "pan_out1", "pan_out0") + tuple(
    f"{n}_{l}" for l in range(3) for n in ("stem", "cls_feat", "reg_feat"))


def dims(model_name):
    depth, width = VARIANTS[model_name]
    return int(64 * width), max(round(3 * depth), 1)


def csp_names(prefix, cin, cout, n):
    h = cout // 2
    t = [(prefix + ".conv1", cin, h, 1), (prefix + ".conv2", cin, h, 1)]
    for i in range(n):
        t += [(f"{prefix}.m.{i}.conv1", h, h, 1), (f"{prefix}.m.{i}.conv2", h, h, 3)]
    return t + [(prefix + ".conv3", 2 * h, cout, 1)]


def base_conv_names(base, d):
    """(prefix, Cin, Cout, k) of every BaseConv in module order"""
    bb, fp = "backbone.backbone.", "backbone."
    t = [(bb + "stem.conv", 12, base, 3)]
    for s, n in enumerate((d, 3 * d, 3 * d, d)):
        p, cin, cout = f"{bb}dark{s + 2}", base << s, base << (s + 1)
        t.append((p + ".0", cin, cout, 3))
        if s == 3:
            t += [(p + ".1.conv1", cout, cout // 2, 1), (p + ".1.conv2", 2 * cout, cout, 1)] + csp_names(p + ".2", cout, cout, n)
        else:
            t += csp_names(p + ".1", cout, cout, n)
    c3, c4, c5 = 4 * base, 8 * base, 16 * base
    t += [(fp + "lateral_conv0", c5, c4, 1)] + csp_names(fp + "C3_p4", 2 * c4, c4, d) + [(fp + "reduce_conv1", c4, c3, 1)]
    t += csp_names(fp + "C3_p3", 2 * c3, c3, d) + [(fp + "bu_conv2", c3, c3, 3)] + csp_names(fp + "C3_n3", 2 * c3, c4, d)
    t += [(fp + "bu_conv1", c4, c4, 3)] + csp_names(fp + "C3_n4", 2 * c4, c5, d)
    hc = 4 * base
    for l, c in enumerate((c3, c4, c5)):
        t.append((f"head.stems.{l}", c, hc, 1))
        t += [(f"head.cls_convs.{l}.{j}", hc, hc, 3) for j in range(2)] + [(f"head.reg_convs.{l}.{j}", hc, hc, 3) for j in range(2)]
    return t


def synth_state(model_name="yolox-s", num_classes=80, seed=0, obj_bias=-3.5, obj_std=2.0, cls_std=3.0, reg_std=0.4, cls_bias=0.0, calib=None):
    """Seeded weights: one torch.Generator, walking the modules in order.  Filters normal with std sqrt(2 / fan_in); BatchNorm gain
    1 +- 0.1 and bias +- 0.1; its running statistics are then SET, as training sets them, to each conv's per-channel mean and variance
    over a calibration batch (`calib`, by default a seeded 6 x 160 x 160 one; one fp32 pass, the variance floored at a twentieth of the layer's mean), so that
    every BaseConv's output is O(1) through the network's ~60 layers whatever the residual sums add.  The pred convs are scaled in the
    same pass to the given standard deviation of their outputs: box terms +- 0.4 around a bias of +- 0.3, objectness logits 2 around
    obj_bias (about a tenth of the rows pass a threshold of 0.25), class logits 3 around cls_bias +- 0.5 (the best of 80 classes is then
    close to 1, so a row's score is its objectness)."""
    base, d = dims(model_name)
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def u(n, lo, hi):
        return torch.rand((n,), generator=g, dtype=torch.float32) * (hi - lo) + lo

    for name, cin, cout, k in base_conv_names(base, d):
        sd[name + ".conv.weight"] = torch.randn((cout, cin, k, k), generator=g, dtype=torch.float32) * (2.0 / (cin * k * k)) ** 0.5
        sd[name + ".bn.weight"], sd[name + ".bn.bias"] = u(cout, 0.9, 1.1), u(cout, -0.1, 0.1)
        sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"] = torch.zeros(cout), torch.ones(cout)
        sd[name + ".bn.num_batches_tracked"] = torch.tensor(1000)
    hc = 4 * base
    for l in range(3):
        for kind, n, lo, hi in (("cls", num_classes, cls_bias - 0.5, cls_bias + 0.5), ("reg", 4, -0.3, 0.3), ("obj", 1, obj_bias, obj_bias)):
            sd[f"head.{kind}_preds.{l}.weight"] = torch.randn((n, hc, 1, 1), generator=g, dtype=torch.float32) / hc ** 0.5
            sd[f"head.{kind}_preds.{l}.bias"] = u(n, lo, hi)
    forward(sd, torch.from_numpy(seeded_input(seed + 7919, 6, 160, 160)) if calib is None else calib, calibrate={"cls": cls_std, "reg": reg_std, "obj": obj_std})
    return sd


def focus_split(x):
    """[B, 3, H, W] -> [B, 12, H/2, W/2]: channel 3 k + c from quadrant k"""
    return torch.cat((x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]), 1)


def pool5(x):
    return F.max_pool2d(x, 5, 1, 2)


def base_conv_of(sd, name, t, stride=1, calibrate=None):
    """BaseConv `name` of the state dict on t, in t's dtype: conv (pad (k - 1) // 2, no bias) -> BatchNorm (eps 1e-3) -> SiLU"""
    dt = t.dtype
    w = sd[name + ".conv.weight"].to(dt)
    t = F.conv2d(t, w, None, stride=stride, padding=(w.shape[-1] - 1) // 2)
    if calibrate:                # synth_state: this conv's batch statistics become its BatchNorm's running statistics
        var = t.var((0, 2, 3), unbiased=False)
        sd[name + ".bn.running_mean"] = t.mean((0, 2, 3)).float()
        sd[name + ".bn.running_var"] = torch.maximum(var, var.mean() / 20).float()
    g, b, m, v = (sd[f"{name}.bn.{s}"].to(dt)[None, :, None, None] for s in ("weight", "bias", "running_mean", "running_var"))
    t = (t - m) / torch.sqrt(v + BN_EPS) * g + b
    return t * torch.sigmoid(t)


def forward(sd, x, stages=None, calibrate=None):
    """x: [B, 3, H, W] in the dtype to compute in (BGR 0..255, the reference's preprocess output); sd: upstream's state dict (any float
    dtype: cast to x's).  Returns the head's undecoded rows [B, A, 5 + C].  `stages` (a dict) receives the named stage outputs
    rtd_debug_yolox_tensor knows, as [B, h, w, c] tensors.  calibrate: see synth_state."""
    dt = x.dtype

    def keep(name, t):
        if stages is not None:
            stages[name] = t.permute(0, 2, 3, 1).contiguous()

    def base_conv(name, t, stride=1):
        return base_conv_of(sd, name, t, stride, calibrate)

    def bottleneck(name, t, shortcut):
        y = base_conv(name + ".conv2", base_conv(name + ".conv1", t))
        return y + t if shortcut else y

    def csp(name, t, shortcut):
        a, b = base_conv(name + ".conv1", t), base_conv(name + ".conv2", t)
        i = 0
        while f"{name}.m.{i}.conv1.conv.weight" in sd:
            a = bottleneck(f"{name}.m.{i}", a, shortcut)
            i += 1
        return base_conv(name + ".conv3", torch.cat((a, b), 1))

    def up2(t):
        return F.interpolate(t, scale_factor=2, mode="nearest")

    bb = "backbone.backbone."
    t = base_conv(bb + "stem.conv", focus_split(x))
    keep("stem", t)
    feats = {}
    for s in (2, 3, 4):
        t = csp(f"{bb}dark{s}.1", base_conv(f"{bb}dark{s}.0", t, 2), True)
        keep(f"dark{s}", t)
        feats[s] = t
    t = base_conv(bb + "dark5.0", t, 2)
    t = base_conv(bb + "dark5.1.conv1", t)
    p5 = pool5(t)
    p9 = pool5(p5)
    t = base_conv(bb + "dark5.1.conv2", torch.cat((t, p5, p9, pool5(p9)), 1))      # pool9 = pool5 o pool5: the padding never wins
    keep("spp", t)
    dark5 = csp(bb + "dark5.2", t, False)
    keep("dark5", dark5)

    fpn_out0 = base_conv("backbone.lateral_conv0", dark5)
    f0 = csp("backbone.C3_p4", torch.cat((up2(fpn_out0), feats[4]), 1), False)
    fpn_out1 = base_conv("backbone.reduce_conv1", f0)
    pan_out2 = csp("backbone.C3_p3", torch.cat((up2(fpn_out1), feats[3]), 1), False)
    pan_out1 = csp("backbone.C3_n3", torch.cat((base_conv("backbone.bu_conv2", pan_out2, 2), fpn_out1), 1), False)
    pan_out0 = csp("backbone.C3_n4", torch.cat((base_conv("backbone.bu_conv1", pan_out1, 2), fpn_out0), 1), False)
    for n, v in (("fpn_out0", fpn_out0), ("fpn_out1", fpn_out1), ("pan_out2", pan_out2), ("pan_out1", pan_out1), ("pan_out0", pan_out0)):
        keep(n, v)

    rows = []
    for l, f in enumerate((pan_out2, pan_out1, pan_out0)):
        st = base_conv(f"head.stems.{l}", f)
        cf = base_conv(f"head.cls_convs.{l}.1", base_conv(f"head.cls_convs.{l}.0", st))
        rf = base_conv(f"head.reg_convs.{l}.1", base_conv(f"head.reg_convs.{l}.0", st))
        keep(f"stem_{l}", st), keep(f"cls_feat_{l}", cf), keep(f"reg_feat_{l}", rf)

        def pred(kind, t):
            if calibrate:        # synth_state: the pred conv is scaled to the output deviation asked for
                w = sd[f"head.{kind}_preds.{l}.weight"]
                sd[f"head.{kind}_preds.{l}.weight"] = w * (calibrate[kind] / float(F.conv2d(t, w.to(dt)).std()))
            return F.conv2d(t, sd[f"head.{kind}_preds.{l}.weight"].to(dt), sd[f"head.{kind}_preds.{l}.bias"].to(dt))

        out = torch.cat((pred("reg", rf), torch.sigmoid(pred("obj", rf)), torch.sigmoid(pred("cls", cf))), 1)
        rows.append(out.flatten(2).permute(0, 2, 1))
    return torch.cat(rows, 1).contiguous()


def forward_fp16(sd, x, stages=None):
    """the restatement with fp16 storage and arithmetic (on the CPU: the yardstick of the GPU tests' gate)"""
    st = {} if stages is not None else None
    out = forward({k: v.half() if v.is_floating_point() else v for k, v in sd.items()}, x.half(), st)
    if stages is not None:
        stages.update({k: v.float() for k, v in st.items()})
    return out.float()


def seeded_input(seed, n, h, w, integer=False):
    """[n, 3, h, w] float32 in 0..255: smooth blobs over noise, non-integer unless asked (the reference's bilinear resize gives such)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, 3, h, w), np.float32)
    for i in range(n):
        img = rng.uniform(0, 90, (3, h, w)).astype(np.float32)
        for _ in range(6):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, max(h, w) / 3)
            img += rng.uniform(20, 160, (3, 1, 1)).astype(np.float32) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))[None]
        out[i] = np.clip(img, 0, 255)
    return np.round(out) if integer else out


class RefModel:
    """the restatement as YOLOXDetector's `model`: [B, 3, H, W] -> [B, A, 5 + C] in `dtype`, returned as fp32 on the input's device"""

    def __init__(self, sd, dtype=torch.float64):
        self.sd, self.dtype = sd, dtype

    def __call__(self, x):
        return forward(self.sd, x.detach().cpu().to(self.dtype)).to(torch.float32).to(x.device)


# ---- the seeded cases of the GPU tests (tools/make_yolox_net_yardstick.py records their errors in tests/golden/yolox_net_yardstick.json) ----
# name: (model, classes, state seed, input seed, n, h, w).  64 x 96 is the smallest input whose three levels (8 x 12, 4 x 6, 2 x 3) all
# differ and are no multiple of any tile; 160 x 160 gives odd maps (5 x 5 at stride 32) larger than SPP's window at stride 8 and 16.
NET_CASES = {
    "s_64x96_n2": ("yolox-s", 80, 1, 5, 2, 64, 96),
    "s_160x160_n1": ("yolox-s", 80, 1, 6, 1, 160, 160),
    "l_64x96_n1": ("yolox-l", 80, 2, 7, 1, 64, 96),
}
# the end-to-end case: a seeded yolox-s checkpoint, input 160 x 160, two scene frames of different sizes (seed, h, w), thresholds as the
# detector's defaults.  The head is seeded narrow (see synth_state), so that 100 x the fp32 restatement's error fits between the scores.
E2E = {"model": "yolox-s", "classes": 80, "state_seed": 3, "input_size": (160, 160), "frames": ((68, 120, 200), (307, 240, 176)), "conf": 0.25, "nms": 0.45,
       "head": {"obj_bias": -6.2, "obj_std": 3.0, "cls_std": 0.5, "reg_std": 0.05}}
_states = {}


def case_state(name):
    """the seeded state dict of a case (built once per process)"""
    if name not in _states:
        if name == "e2e":
            from telescope_cam_detection_amd.synth import scene_frame
            calib = e2e_batch([scene_frame(1000 + i, 120 + 24 * i, 200 - 8 * i) for i in range(8)])      # frames like the case's own
            _states[name] = synth_state(E2E["model"], E2E["classes"], E2E["state_seed"], calib=calib, **E2E["head"])
        else:
            model, C, seed = NET_CASES[name][:3]
            _states[name] = synth_state(model, C, seed)
    return _states[name]


def case_input(name):
    _, _, _, seed, n, h, w = NET_CASES[name]
    return torch.from_numpy(seeded_input(seed, n, h, w))


def e2e_frames():
    from telescope_cam_detection_amd.synth import scene_frame
    return [scene_frame(seed, h, w) for seed, h, w in E2E["frames"]]


def e2e_batch(frames, device="cpu"):
    """the reference's preprocess of the frames: float, bilinear to the input size where the frame has another"""
    out = []
    for f in frames:
        t = torch.from_numpy(f).to(device).permute(2, 0, 1).unsqueeze(0).float()
        if tuple(t.shape[2:]) != tuple(E2E["input_size"]):
            t = F.interpolate(t, size=E2E["input_size"], mode="bilinear", align_corners=False)
        out.append(t)
    return torch.cat(out, 0)


def e2e_conditions(batch, err32):
    """The input conditions of the end-to-end case on the restatement, per image: rows that pass, the smallest |score - conf| and
    |IoU - nms|, and whether the fp32 restatement keeps fp64's rows in fp64's order.  m = 100 x err32."""
    from tests import yolox_ref
    sd = case_state("e2e")
    o64, o32 = forward(sd, batch.double()).numpy(), forward(sd, batch.float()).numpy()
    out = []
    for i in range(len(o64)):
        r64, passed, kept64 = yolox_ref.postprocess(o64[i], E2E["conf"], E2E["nms"], np.float64, E2E["input_size"])
        r32, _, kept32 = yolox_ref.postprocess(o32[i], E2E["conf"], E2E["nms"], np.float32, E2E["input_size"])
        d_iou, d_score = yolox_ref.margins(o64[i], E2E["conf"], E2E["nms"], E2E["input_size"])
        out.append({"passed": int(passed), "kept": int(len(kept64)), "d_score": float(d_score), "d_iou": float(min(d_iou, 1.0)),
                    "same_rows": bool(list(kept64) == list(kept32) and list(r64[:, 6]) == list(r32[:, 6])), "m": 100.0 * err32})
    return out
