#!/usr/bin/env python3
"""Write the JPEG fixtures from Pillow (libjpeg): tests/golden/jpeg_small.npz and tests/golden/jpeg_large.json.

    python tools/make_jpeg_golden.py

Needs Pillow; runs on the CPU.  The judge is `Image.fromarray(rgb_or_gray).save(buf, "JPEG", quality=q)` with every other option at its
default (baseline, 4:2:0, standard Huffman tables: what cv2.imencode produces with IMWRITE_JPEG_QUALITY alone).

jpeg_small.npz   in_<name>: the input (HxWxC uint8, BGR for C = 3); jpg_<name>_q<q>: Pillow's file as a uint8 array
jpeg_large.json  per (kind, seed, h, w, q): length and sha256 of Pillow's file; the inputs are regenerated from synth.make_frame
"""
from __future__ import annotations

import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from telescope_cam_detection_amd.synth import make_frame, noise_frame, scene_frame   # noqa: E402

QUALITIES = [1, 25, 50, 75, 90, 95, 100]
LARGE = [(kind, seed, h, w) for (h, w, seed) in ((1080, 1920, 11), (720, 1280, 12), (487, 641, 13)) for kind in ("scene", "noise")]
LARGE_Q = [50, 90]


def pillow_jpeg(frame: np.ndarray, quality: int) -> bytes:
    from PIL import Image
    a = np.asarray(frame)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    im = Image.fromarray(np.ascontiguousarray(a[:, :, ::-1]) if a.ndim == 3 else np.ascontiguousarray(a))
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=int(quality))
    return buf.getvalue()


def small_inputs() -> dict:
    y, x = np.mgrid[0:64, 0:64]
    hf = np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16)          # the (7, 7) DCT basis: one coefficient at
    zero_runs = np.clip(np.rint(128 + 60 * hf), 0, 255).astype(np.uint8)[:, :, None]           # zig-zag 63, three ZRL codes per block
    y, x = np.mgrid[0:48, 0:64]
    many_ff = ((((x // 3) + (y // 3)) % 2) * 255).astype(np.uint8)[:, :, None]                 # ~6 % of its q = 100 scan bytes are 0xFF
    return {
        "c3_1x1_noise": noise_frame(1, 1, 1),
        "c3_7x5_noise": noise_frame(2, 7, 5),
        "c3_8x8_noise": noise_frame(3, 8, 8),
        "c1_8x8_noise": noise_frame(4, 8, 8)[:, :, :1].copy(),
        "c3_16x16_scene": scene_frame(5, 16, 16),
        "c3_17x23_noise": noise_frame(6, 17, 23),
        "c1_33x16_noise": noise_frame(7, 33, 16)[:, :, :1].copy(),
        "c1_17x23_scene": scene_frame(8, 17, 23)[:, :, 1:2].copy(),
        "c3_64x48_scene": scene_frame(9, 64, 48),
        "c3_250x130_scene": scene_frame(10, 250, 130),
        "c3_40x56_zeros": np.zeros((40, 56, 3), np.uint8),
        "c1_24x40_255": np.full((24, 40, 1), 255, np.uint8),
        "c3_24x40_255": np.full((24, 40, 3), 255, np.uint8),
        "c1_64x64_zero_runs": zero_runs,
        "c1_48x64_many_ff": many_ff,
    }


def main() -> None:
    import PIL
    from PIL import features
    out_dir = os.path.join(ROOT, "tests", "golden")
    arrays = {}
    for name, a in small_inputs().items():
        arrays["in_" + name] = a
        for q in QUALITIES:
            arrays[f"jpg_{name}_q{q}"] = np.frombuffer(pillow_jpeg(a, q), np.uint8)
    path = os.path.join(out_dir, "jpeg_small.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
    entries = []
    for kind, seed, h, w in LARGE:
        a = make_frame(kind, seed, h, w)
        for q in LARGE_Q:
            b = pillow_jpeg(a, q)
            entries.append({"kind": kind, "seed": seed, "h": h, "w": w, "quality": q, "length": len(b), "sha256": hashlib.sha256(b).hexdigest()})
    doc = {"pillow": PIL.__version__, "libjpeg": features.version("jpg"), "libjpeg_turbo": bool(features.check_feature("libjpeg_turbo")),
           "entries": entries}
    path = os.path.join(out_dir, "jpeg_large.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{path}: {len(entries)} entries")


if __name__ == "__main__":
    main()
