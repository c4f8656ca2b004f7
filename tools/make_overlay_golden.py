#!/usr/bin/env python3
"""Record the cv2 calls the reference makes when it draws detections: tests/golden/overlay_calls.json.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_overlay_golden.py --reference /path/to/reference

Runs on the CPU and needs the reference checkout (it is imported, never copied).  A recording stand-in `cv2` module of our own
(tests/overlay_ref.py RecordingCv2: rectangle, getTextSize by a declared fake metric rule, putText, the constants) is put into
sys.modules, and whatever of the web stack is not installed (fastapi, uvicorn) is replaced by empty stand-ins; then the reference's
`src.visualization_utils.draw_detections` and `src.web_server.WebServer._draw_detections(None, frame, result)` are driven over the
scenarios below.  The JSON holds the scenarios, the metric rule and the recorded call lists - recorded results only.

The scenarios cover float and inverted corners, boxes at the top edge (both label_y branches, negative bar coordinates), every palette
class and an unknown one, species with and without a level and the level "species", an empty list, a missing total_latency_ms,
draw_labels=False, and one 1080p web scene of ten detections (the GPU test's whole-frame comparison).
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.overlay_ref import METRIC, RecordingCv2   # noqa: E402

PALETTE = ["person", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant", "bear", "zebra", "giraffe"]


def det(name, conf, x1, y1, x2, y2, **extra):
    d = {"class_name": name, "confidence": conf, "bbox": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}}
    d.update(extra)
    return d


def scenarios() -> list:
    palette = [det(n, 0.5 + 0.04 * i, 20 + 90 * i, 60 + 7 * i, 100 + 90 * i, 200 + 5 * i) for i, n in enumerate(PALETTE)]
    palette += [det("Cat", 0.77, 30, 300, 130, 420), det("telescope", 0.31, 400, 300, 520, 400)]       # case-folded, unknown
    edge = [det("cat", 0.9, 10, 5, 110, 90), det("dog", 0.81, 200, 0, 300, 80), det("bird", 0.66, 0, 33, 50, 70),
            det("person", 0.99, -20, -15, 60, 40), det("car", 0.42, 500.7, 31.2, 620.9, 140.5)]
    floats = [det("bird", 0.914, 100.9, 120.99, 220.1, 260.5), det("person", 0.505, 300, 400, 250, 310),   # inverted corners
              det("cat", 0.125, -30.7, 250.5, 80.2, 330.9)]
    species = [det("bird", 0.8, 50, 100, 200, 220, species="Northern Cardinal", species_confidence=0.93, taxonomic_level="species"),
               det("bird", 0.7, 250, 100, 400, 220, species="Corvus", species_confidence=0.612, taxonomic_level="genus"),
               det("cat", 0.6, 450, 100, 600, 220, species="Bobcat", species_confidence=0.5),
               det("dog", 0.55, 50, 300, 200, 420, species="Canidae", species_confidence=0.4, taxonomic_level=""),
               det("dog", 0.45, 250, 300, 400, 420, species="Coyote", species_confidence=None, taxonomic_level="species"),
               det("bear", 0.35, 450, 10, 600, 90, species="Ursus americanus", species_confidence=0.87, taxonomic_level="family")]
    wide = [det(["person", "cat", "dog", "bird", "car", "deer", "person", "bird", "truck", "cat"][i], 0.35 + 0.06 * i,
                60.5 + 180 * i, 40 + 95 * i, 240.25 + 175 * i, 180 + 90 * i) for i in range(10)]
    out = []
    for name, dets, hw in (("palette", palette, (480, 1100)), ("top_edge", edge, (200, 640)), ("floats_inverted", floats, (480, 640)),
                           ("species", species, (480, 640)), ("empty", [], (48, 64))):
        out.append({"name": "snap_" + name, "kind": "snapshot", "hw": hw, "detections": dets, "thickness": 3, "font_scale": 0.7, "draw_labels": True})
        out.append({"name": "web_" + name, "kind": "web", "hw": hw, "result": {"detections": dets, "total_latency_ms": 12.6}})
    out.append({"name": "snap_no_labels", "kind": "snapshot", "hw": (200, 640), "detections": edge, "thickness": 1, "font_scale": 0.7, "draw_labels": False})
    out.append({"name": "snap_thin_small_font", "kind": "snapshot", "hw": (480, 640), "detections": species, "thickness": 2, "font_scale": 0.5, "draw_labels": True})
    out.append({"name": "web_no_latency", "kind": "web", "hw": (200, 640), "result": {"detections": edge[:2]}})
    out.append({"name": "web_no_detections_key", "kind": "web", "hw": (48, 64), "result": {"total_latency_ms": 3.49}})
    out.append({"name": "web_1080p", "kind": "web", "hw": (1080, 1920), "result": {"detections": wide, "total_latency_ms": 41.5}})
    return out


def stand_in(name: str) -> types.ModuleType:
    """an empty module whose every attribute is a class that accepts anything (enough for imports and annotations)"""
    class Anything:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return self

        def __getattr__(self, _):
            return Anything()

    m = types.ModuleType(name)
    m.__getattr__ = lambda _attr: Anything          # type: ignore[attr-defined]
    return m


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (the directory that holds src/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "overlay_calls.json"))
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    rec = RecordingCv2()
    sys.modules["cv2"] = rec                          # type: ignore[assignment]
    for name in ("fastapi", "fastapi.responses", "fastapi.staticfiles", "fastapi.security", "uvicorn"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = stand_in(name)
    sys.path.insert(0, os.path.abspath(a.reference))
    vis = importlib.import_module("src.visualization_utils")
    web = importlib.import_module("src.web_server")
    doc = {"metric": dict(METRIC),
           "metric_rule": "w = int(len(text) * char_w * scale + 0.5), h = int(cap_h * scale + 0.5), baseline = int(base * scale + 0.5) + thickness // 2",
           "events": "['rect', [x1, y1], [x2, y2], bgr, thickness] / ['text', text, [x, y], scale, bgr, thickness, line type is LINE_AA]",
           "scenarios": []}
    for s in scenarios():
        rec.calls = []
        frame = np.zeros((s["hw"][0], s["hw"][1], 3), np.uint8)
        if s["kind"] == "snapshot":
            vis.draw_detections(frame, s["detections"], thickness=s["thickness"], font_scale=s["font_scale"], draw_labels=s["draw_labels"])
        else:
            web.WebServer._draw_detections(None, frame, s["result"])
        doc["scenarios"].append(dict(s, calls=rec.calls))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"{a.out}: {len(doc['scenarios'])} scenarios, {sum(len(s['calls']) for s in doc['scenarios'])} calls, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
