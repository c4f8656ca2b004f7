"""Restatement of the reference's Real-ESRGAN x4 path (src/image_enhancement.py, method "realesrgan"): basicsr's
RRDBNet(3, 3, num_feat 64, num_block B, num_grow_ch 32, scale 4) inside realesrgan's `RealESRGANer.enhance(img, outscale=4)` for a
3-channel uint8 BGR crop with pre_pad = 0.  Plain torch, generic in the dtype, so the same code is the fp64 yardstick and the fp32 /
fp16 runs it is compared with.

basicsr and realesrgan are not importable here and no upstream checkpoint is at hand: the architecture, the state-dict key table and the
`RealESRGANer` flow below are written from the public sources and could NOT be checked against them offline.  Where `realesrgan` is
importable, tests/test_esrgan_host.py compares.

Arithmetic:
  conv_first 3 -> 64; B x RRDB; feat + conv_body(body(feat)); lrelu(conv_up1(nearest2x(.))); lrelu(conv_up2(nearest2x(.)));
  conv_last(lrelu(conv_hr(.))).  An RRDB is three dense blocks and returns rdb3(rdb2(rdb1(x))) * 0.2 + x; a dense block is
  conv1..conv4 (64 + 32 k -> 32 channels, LeakyReLU(0.2), each reading the concatenation of the block input and all earlier outputs),
  conv5 192 -> 64 without activation, and x5 * 0.2 + x.  All convs 3 x 3, stride 1, zero pad 1, with bias.
  enhance(): float32(v) / 255 in fp32, BGR -> RGB; the network on the whole crop (tile = 0) or tile_process; clamp(0, 1), RGB -> BGR,
  round(x * 255) as numpy rounds (half to even), uint8.
"""
import numpy as np
import torch
import torch.nn.functional as F

NUM_FEAT, NUM_GROW_CH = 64, 32


def conv_names(num_block):
    """(state-dict prefix, Cin, Cout) in module order (= named_parameters() order of the upstream modules)"""
    t = [("conv_first", 3, NUM_FEAT)]
    for i in range(num_block):
        for j in (1, 2, 3):
            for k in (1, 2, 3, 4, 5):
                t.append((f"body.{i}.rdb{j}.conv{k}", NUM_FEAT + NUM_GROW_CH * (k - 1), NUM_FEAT if k == 5 else NUM_GROW_CH))
    t += [("conv_body", NUM_FEAT, NUM_FEAT), ("conv_up1", NUM_FEAT, NUM_FEAT), ("conv_up2", NUM_FEAT, NUM_FEAT), ("conv_hr", NUM_FEAT, NUM_FEAT),
          ("conv_last", NUM_FEAT, 3)]
    return t


def synth_state(num_block, seed=0):
    """Seeded weights: one torch.Generator, walking the parameters in module order (weight, then bias, per conv).  Filters He-normal,
    x 0.1 under `body.`, x 0.3 elsewhere; biases (U[0, 1) - 0.5) * 0.1; conv_last.bias + 0.5.  With these the fp64 outputs stay
    strictly inside (0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout in conv_names(num_block):
        std = (2.0 / (cin * 9)) ** 0.5
        w = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float32) * std * (0.1 if name.startswith("body.") else 0.3)
        b = (torch.rand((cout,), generator=g, dtype=torch.float32) - 0.5) * 0.1
        if name == "conv_last":
            b = b + 0.5
        sd[name + ".weight"], sd[name + ".bias"] = w, b
    return sd


def num_blocks_of(sd):
    n = 0
    while f"body.{n}.rdb1.conv1.weight" in sd:
        n += 1
    return n


def _lrelu(x):
    return F.leaky_relu(x, 0.2)


def rrdbnet(sd, x, stages=None):
    """x: [1, 3, h, w] in the dtype to compute in; sd: the state dict (any float dtype: cast to x's).  `stages` (a dict) receives the
    named stage outputs rtd_debug_esrgan_tensor knows, as [h, w, c] tensors."""
    dt = x.dtype

    def conv(name, t):
        return F.conv2d(t, sd[name + ".weight"].to(dt), sd[name + ".bias"].to(dt), stride=1, padding=1)

    def keep(name, t):
        if stages is not None:
            stages[name] = t[0].permute(1, 2, 0).contiguous()

    def rdb(pfx, t):
        x1 = _lrelu(conv(pfx + ".conv1", t))
        x2 = _lrelu(conv(pfx + ".conv2", torch.cat((t, x1), 1)))
        x3 = _lrelu(conv(pfx + ".conv3", torch.cat((t, x1, x2), 1)))
        x4 = _lrelu(conv(pfx + ".conv4", torch.cat((t, x1, x2, x3), 1)))
        x5 = conv(pfx + ".conv5", torch.cat((t, x1, x2, x3, x4), 1))
        return x5 * 0.2 + t

    feat = conv("conv_first", x)
    keep("first", feat)
    body = feat
    for i in range(num_blocks_of(sd)):
        t = body
        for j in (1, 2, 3):
            t = rdb(f"body.{i}.rdb{j}", t)
            keep(f"body.{i}.rdb{j}", t)
        body = t * 0.2 + body
        keep(f"body.{i}", body)
    feat = feat + conv("conv_body", body)
    keep("trunk", feat)
    feat = _lrelu(conv("conv_up1", F.interpolate(feat, scale_factor=2, mode="nearest")))
    keep("up1", feat)
    feat = _lrelu(conv("conv_up2", F.interpolate(feat, scale_factor=2, mode="nearest")))
    keep("up2", feat)
    hr = _lrelu(conv("conv_hr", feat))
    keep("hr", hr)
    out = conv("conv_last", hr)
    keep("last", out)
    return out


def ingest(crop_bgr, dtype):
    """step 1: float32(v) / 255 in fp32, BGR -> RGB, [1, 3, h, w] in `dtype`"""
    img = crop_bgr.astype(np.float32) / np.float32(255.0)
    rgb = np.ascontiguousarray(img[:, :, ::-1].transpose(2, 0, 1))
    return torch.from_numpy(rgb)[None].to(dtype)


def tile_list(h, w, tile, pad):
    """RealESRGANer.tile_process: ((core y0, y1, x0, x1), (input y0, y1, x0, x1)) per tile, row-major"""
    if tile <= 0:
        return [((0, h, 0, w), (0, h, 0, w))]
    out = []
    for ty in range((h + tile - 1) // tile):
        for tx in range((w + tile - 1) // tile):
            x0, y0 = tx * tile, ty * tile
            x1, y1 = min(x0 + tile, w), min(y0 + tile, h)
            out.append(((y0, y1, x0, x1), (max(y0 - pad, 0), min(y1 + pad, h), max(x0 - pad, 0), min(x1 + pad, w))))
    return out


def upscale_float(sd, crop_bgr, dtype=torch.float64, tile=0, tile_pad=10, stages=None):
    """the float output of the network, [3, 4h, 4w] (RGB) in `dtype`, before the clamp; `stages`: those of the LAST tile"""
    x = ingest(crop_bgr, dtype)
    h, w = crop_bgr.shape[:2]
    out = torch.zeros((3, 4 * h, 4 * w), dtype=dtype)
    with torch.no_grad():
        for (cy0, cy1, cx0, cx1), (iy0, iy1, ix0, ix1) in tile_list(h, w, tile, tile_pad):
            st = {} if stages is not None else None
            xin = x[:, :, iy0:iy1, ix0:ix1]
            y = rrdbnet(sd, xin, st)[0]
            if stages is not None:
                stages.clear()
                stages.update(st)
                stages["ingest"] = xin[0].permute(1, 2, 0).contiguous()
            oy, ox = 4 * (cy0 - iy0), 4 * (cx0 - ix0)
            out[:, 4 * cy0:4 * cy1, 4 * cx0:4 * cx1] = y[:, oy:oy + 4 * (cy1 - cy0), ox:ox + 4 * (cx1 - cx0)]
    return out


def to_bytes(out_float):
    """step 3: clamp(0, 1), RGB -> BGR, round(x * 255) half to even, uint8 [4h, 4w, 3]"""
    o = out_float.clamp(0, 1).permute(1, 2, 0).numpy()[:, :, ::-1]
    return np.ascontiguousarray((o * 255.0).round().astype(np.uint8))


def enhance(sd, crop_bgr, dtype=torch.float64, tile=0, tile_pad=10):
    return to_bytes(upscale_float(sd, crop_bgr, dtype, tile, tile_pad))


def random_crop(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the yardstick cases (tools/make_esrgan_yardstick.py records them in tests/golden/esrgan_yardstick.json)
CASES = {
    "b2_19x27": dict(num_block=2, h=19, w=27, seed=1),
    "b23_32x32": dict(num_block=23, h=32, w=32, seed=2),
    "b1_19x27": dict(num_block=1, h=19, w=27, seed=3),
    "b1_40x33_t16p4": dict(num_block=1, h=40, w=33, seed=4, tile=16, tile_pad=4),
    "b1_24x20": dict(num_block=1, h=24, w=20, seed=5),
}
STAGE_CASE = "b1_19x27"


def stage_names(num_block):
    names = ["first"]
    for i in range(num_block):
        names += [f"body.{i}.rdb{j}" for j in (1, 2, 3)] + [f"body.{i}"]
    return names + ["trunk", "up1", "up2", "hr", "last"]


def case_inputs(name):
    c = CASES[name]
    return synth_state(c["num_block"], 0), random_crop(c["h"], c["w"], c["seed"]), c.get("tile", 0), c.get("tile_pad", 10)


def measure_case(name, dtypes=(torch.float32, torch.float16)):
    """max |delta| of the float output and the share of differing bytes of every dtype's run against fp64; for STAGE_CASE also the max
    |delta| per named stage"""
    sd, crop, tile, pad = case_inputs(name)
    st64 = {} if name == STAGE_CASE else None
    ref = upscale_float(sd, crop, torch.float64, tile, pad, st64)
    ref_bytes = to_bytes(ref)
    rec = {"range": [float(ref.min()), float(ref.max())]}
    for dt in dtypes:
        key = {torch.float32: "fp32", torch.float16: "fp16"}[dt]
        st = {} if name == STAGE_CASE else None
        got = upscale_float(sd, crop, dt, tile, pad, st).double()
        b = to_bytes(got)
        diff = np.abs(b.astype(np.int16) - ref_bytes.astype(np.int16))
        rec[key] = {"max_abs": float((got - ref).abs().max()), "byte_share": float((diff != 0).mean()), "worst_byte": int(diff.max())}
        if st is not None:
            rec[key]["stages"] = {k: float((st[k].double() - st64[k]).abs().max()) for k in stage_names(CASES[name]["num_block"])}
    return rec
