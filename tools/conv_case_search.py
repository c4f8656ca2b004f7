#!/usr/bin/env python3
"""Finds, for every conv kernel instantiation launch_conv can name, the cheapest launch that reaches it - and writes tests/conv_cases.py.

The library says which instantiations exist (rtd_debug_conv_instantiations) and what a described launch would run under the debug
options as they stand (rtd_debug_conv_choice: the launchers' own checks and choice functions, host arithmetic only).  This tool walks
the candidate grid stated below, asks for every candidate and keeps, per instantiation key, the candidate with the fewest
multiply-accumulates; ties go to a ragged last pixel tile, then to a partial last channel tile, then to the earlier candidate.
Besides one row per instantiation (one-pass, S = 1) it keeps, per (stages, bn) group of the flexible and the fixed pair tiles, the
cheapest launch with S = 2 and with S = 4 slices of the two-pass split-K.  Each row then gets its residual mode, output type and
activation by rotation within its family (kept only if the choice does not move), so that every family sees all of them.

Needs no GPU.   python tools/conv_case_search.py [--check]     (--check: compare with the committed table, write nothing)
"""
import argparse
import itertools
import os
import pprint
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from telescope_cam_detection_amd import _capi  # noqa: E402

MAX_MACS = 8e9
BIG = 1 << 30
DT = {"bf16": 0, "f32": 1, "f16x2": 4}

# ---- option sets: only rtd_debug_option names that exist (no forcing switch) ----------------------------------------------------------
_PAIR_TILES_ONLY = {"split_sx": 0, "conv_reg": 0}                           # no streaming / direct 3x3 kernel takes the shape
_FIXED = dict(_PAIR_TILES_ONLY, split_flex=0, split_wsq=0)
OPTION_SETS = {
    "default": {},
    "mode1": {"conv_mode": 1}, "mode3": {"conv_mode": 3}, "mode4": {"conv_mode": 4}, "mode10": {"conv_mode": 10},
    "sx4": {"split_sx": 4},
    "flex": dict(_PAIR_TILES_ONLY, split_flex_small_max=BIG, split_flex_min_nk=1),
    "quad": dict(_PAIR_TILES_ONLY, split_flex=0, split_wsq=2, split_wsq_min_nk=1, split_k2=0),
    "fixed_s2_bn128": dict(_FIXED, split_ws2_min_blocks=1, split_ws64_max_blocks=0),
    "fixed_s2_bn64": dict(_FIXED, split_ws2_min_blocks=1, split_ws64_max_blocks=BIG),
    "fixed_s4_bn128": dict(_FIXED, split_ws2_min_blocks=BIG, split_ws64_max_blocks=0),
    "fixed_s4_bn64": dict(_FIXED, split_ws2_min_blocks=BIG, split_ws64_max_blocks=BIG),
}
PLAIN_SETS = ("default", "mode1", "mode3", "mode4", "mode10")
FIXED_SETS = ("fixed_s2_bn128", "fixed_s2_bn64", "fixed_s4_bn128", "fixed_s4_bn64")

FORM_DEFAULTS = dict(k=1, stride=1, pad=0, C2=0, x_up2=0, Cnext=0, avg=0, pool=0, res_mode=0, out_f32=0)


def form(**kw):
    return dict(FORM_DEFAULTS, **kw)


def candidates():
    """(option set, launch) in a fixed order: the stated grid."""
    # bf16 / fp32 operands: register-staged tiles (small-channel loader: Cin % 32 != 0) and the LDS-DMA tiles
    hw_plain = [(7, 9), (16, 16), (33, 29), (64, 64), (65, 63), (112, 112), (113, 111)]
    for dt, opt, k, cin, cout, B, (H, W) in itertools.product(("bf16", "f32"), PLAIN_SETS, (1, 3), (8, 16, 32, 64, 128), (32, 64, 96, 128, 192, 512),
                                                              (1, 2, 4), hw_plain):
        yield opt, form(dtype=dt, B=B, H=H, W=W, Cin=cin, Cout=cout, k=k, pad=k // 2)
    # pair operands, tile kernels (flexible height, quad): option sets x k x Cin x Cout x B x H x W
    hs = (8, 10, 13, 16, 20, 25, 29, 33, 37, 40, 45, 50, 57, 64, 73, 76, 80)
    ws = (8, 11, 16, 20, 26, 31, 36, 40, 45, 52, 61, 70, 75, 81, 90)
    couts = (64, 96, 128, 192, 256, 512, 672, 704)
    for opt, k, cin, cout, B, H, W in itertools.product(("flex", "quad"), (1, 3), (32, 64, 128, 256, 512), couts, (1, 2, 3, 8), hs, ws):
        yield opt, form(dtype="f16x2", B=B, H=H, W=W, Cin=cin, Cout=cout, k=k, pad=k // 2)
    # ... fixed 128-pixel tiles: every (stages, bn) is a matter of the two thresholds, so small maps do
    for opt, k, cin, cout, B, H, W in itertools.product(FIXED_SETS, (1, 3), (32, 512), couts, (1, 2), (8, 13, 20, 33), (8, 11, 26, 52)):
        yield opt, form(dtype="f16x2", B=B, H=H, W=W, Cin=cin, Cout=cout, k=k, pad=k // 2)
    # ... two-pass split-K on the 2-stage flexible tile: more than one round of blocks (> 256) on <= 16 (S = 2) or <= 8 (S = 4) tiles per
    # image with >= 128 K-steps needs a batch of 13+ images; Cout = 72 (fp32 rows out) keeps the S = 2 launch below MAX_MACS
    for (k, cin), cout, B, H, W, f32 in itertools.product(((1, 4096), (3, 512)), (72, 96, 128), (13, 14, 16), (28, 30, 32), (34, 40, 60, 62, 64), (0, 1)):
        yield "flex", form(dtype="f16x2", B=B, H=H, W=W, Cin=cin, Cout=cout, k=k, pad=k // 2, out_f32=f32)
    # streaming 1x1 kernel: plain, dual (x2), with a fused follower (next), with the fused average (avg); fp32 rows out
    hw_sx = [(80, 80), (81, 80), (80, 96), (82, 80), (40, 40), (41, 40), (40, 48)]
    for opt, cin, c2, cout, res, f32, cnext, avg, (H, W) in itertools.product(("default", "sx4"), (64, 128, 256), (0, 64), (256, 512, 1024), (0, 1), (0, 1), (0, 64, 128),
                                                                              (0, 1), hw_sx):
        yield opt, form(dtype="f16x2", B=1, H=H, W=W, Cin=cin, C2=c2, Cout=cout, res_mode=res, out_f32=f32, Cnext=cnext, avg=avg)
    # direct 3x3 kernels (8 x 32 and 8 x 16 pixel tiles; floors of 32 and 128 tiles per image) and the fused max-pool
    for cin, cout, pool, B, H, W in itertools.product((32, 64), (32, 64), (0, 1), (1, 3), (57, 58, 64, 121, 122, 128), (97, 98, 113, 114, 128, 241)):
        yield "default", form(dtype="f16x2", B=B, H=H, W=W, Cin=cin, Cout=cout, k=3, pad=1, pool=pool)


def set_options(opts):
    _capi.debug_option("reset", 0)
    for name, value in opts.items():
        _capi.debug_option(name, value)


def predict(f):
    return _capi.conv_choice(DT[f["dtype"]], f["B"], f["H"], f["W"], f["Cin"], f["Cout"], f["k"], f["stride"], f["pad"], f["res_mode"], f["out_f32"],
                             f["C2"], f["x_up2"], f["Cnext"], f["avg"], f["pool"])


def out_hw(f):
    return (f["H"] + 2 * f["pad"] - f["k"]) // f["stride"] + 1, (f["W"] + 2 * f["pad"] - f["k"]) // f["stride"] + 1


def macs(f):
    oh, ow = out_hw(f)
    return f["B"] * oh * ow * f["Cout"] * (f["k"] * f["k"] * f["Cin"] + f["C2"] + f["Cnext"])


FAMILY = ("tile", "ws", "sx", "reg3x3", "reg3x3_64", "wsf", "wsq", "wsx")

# The cheapest launch of a tile kernel would have ONE K-step, which never turns the staging ring over.  A row must walk K far enough
# to wrap every stage more than twice and leave an odd tail behind the 2-unrolled loops: 9 K-steps for the LDS-DMA tiles (up to 4
# stages; 9 = one 3x3 conv over one 32-channel group), 3 for the register-staged kernel (two buffers).
MIN_K_STEPS = {"tile": 3, "ws": 9, "wsf": 9, "wsq": 9, "wsx": 9}


def k_steps(f, fam):
    """K-steps of the family's loop: the LDS-DMA tiles stage 128-byte filter rows (32 pair channels with hi and lo, 64 bf16 or 32 fp32
    values); the register-staged kernel walks the filter row, padded to 64 values, 32 at a time."""
    K = f["k"] * f["k"] * f["Cin"] + f["C2"]
    if fam == "tile":
        return (K + 63) // 64 * 2
    per = {"f16x2": 32, "bf16": 64, "f32": 32}[f["dtype"]]
    return (K + per - 1) // per


# ... and a row must put more than one block along the pixels (block index arithmetic, a tile straddling two images): at least 3 tiles
MIN_PIXEL_TILES = 3


def tile_extent(c):
    """(pixels, channels) of one tile of the chosen tile kernel."""
    fam = FAMILY[c["family"]]
    if fam == "wsq":
        a, b = (int(t) for t in c["key"].split(".")[1].split("x"))
        return 16 * (a + b), 128
    return {"tile": c["bm"], "ws": 128, "sx": 32, "wsf": 16 * c["mt"], "wsx": 128}[fam], (256 if fam == "sx" else c["bn"])


def raggedness(f, c):
    """(ragged last pixel tile, partial last channel tile) of launch f under choice c."""
    oh, ow = out_hw(f)
    M, N, fam = f["B"] * oh * ow, f["Cout"], FAMILY[c["family"]]
    if fam in ("reg3x3", "reg3x3_64"):
        return int(oh % 8 != 0 and ow % (32 if fam == "reg3x3" else 16) != 0), 0
    pix, ch = tile_extent(c)
    return int(M % pix != 0), int(N % ch != 0)


def group_of(c):
    return f"{FAMILY[c['family']]}.s{c['stages']}.bn{c['bn']}"


def search(only_keys=None):
    """{row name: (option set, launch, choice)}: row name = key for the one-pass rows, '<group>@S<n>' for the split-K rows."""
    best = {}
    by_opt = {}
    for opt, f in candidates():
        by_opt.setdefault(opt, []).append(f)
    for opt, forms in by_opt.items():
        set_options(OPTION_SETS[opt])
        for f in forms:
            m = macs(f)
            if m > MAX_MACS:
                continue
            c = predict(f)
            if c is None:
                continue
            if only_keys is not None and c["key"] not in only_keys:
                continue
            fam = FAMILY[c["family"]]
            if fam in MIN_K_STEPS:
                oh, ow = out_hw(f)
                if k_steps(f, fam) // c["S"] < MIN_K_STEPS[fam] or f["B"] * oh * ow <= (MIN_PIXEL_TILES - 1) * tile_extent(c)[0]:
                    continue
            names = [c["key"]] if c["S"] == 1 else []
            if c["S"] > 1 and FAMILY[c["family"]] in ("wsf", "wsx"):
                names.append(f"{group_of(c)}@S{c['S']}")
            for name in names:
                rm, rn = raggedness(f, c)
                score = (m, -rm, -rn)
                if name not in best or score < best[name][0]:
                    best[name] = (score, opt, f, c)
    _capi.debug_option("reset", 0)
    return {n: v[1:] for n, v in best.items()}


# what a family's epilogue offers (rtd_op_conv's arguments): residual modes, fp32 rows out beside the operand type
def finish_rows(found):
    """Rotate residual mode, output type and activation through each family's rows; keep a setting only if the choice stays."""
    rows, turn = [], {}
    for name in sorted(found):
        opt, f, c = found[name]
        fam = FAMILY[c["family"]]
        set_options(OPTION_SETS[opt])
        t = turn.get(fam, 0)
        turn[fam] = t + 1
        f = dict(f)
        if fam not in ("sx", "reg3x3", "reg3x3_64") and not f["pool"]:
            outs = (0,) if f["dtype"] == "f32" else (0, 1)
            wanted = [(r, o) for r in (0, 1, 2) for o in outs]
            for i in range(len(wanted)):
                r, o = wanted[(t + i) % len(wanted)]
                g = dict(f, res_mode=r, out_f32=o)
                c2 = predict(g)
                if c2 is not None and c2["key"] == c["key"] and c2["S"] == c["S"]:
                    f = g
                    break
        elif fam == "sx" and f["res_mode"]:
            f["res_mode"] = 1 + t % 2
        f["act"] = "relu" if f["pool"] else ("relu", "silu", "none", "gelu")[t % 4]
        c = predict(f)
        rows.append(dict(name=name, key=c["key"], S=c["S"], grid=c["grid"], opts=OPTION_SETS[opt], **f))
    _capi.debug_option("reset", 0)
    return rows


# instantiations the grid above does not reach: key -> why (at most 2, none of the pair tile families; tests/test_conv_choice_host.py)
UNREACHED = {}

HEADER = '''"""One small launch per conv kernel instantiation (and per split-K slice count of the pair tile groups): GENERATED by
tools/conv_case_search.py from the library's own choice functions - edit the tool's grid, not this file.
name: the instantiation key (rtd_debug_conv_instantiations) or '<family>.s<stages>.bn<bn>@S<slices>'; key / S / grid: what
rtd_debug_conv_choice answers for the launch under `opts` (rtd_debug_option settings on top of "reset")."""

'''


def render(rows):
    body = "CASES = [\n" + "".join("    " + pprint.pformat(r, width=1000, sort_dicts=False) + ",\n" for r in rows) + "]\n"
    un = "UNREACHED = " + pprint.pformat(UNREACHED, width=140) + "\n"
    return HEADER + "# key -> why no launch reaches it (the search finds none)\n" + un + "\n" + body


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with tests/conv_cases.py instead of writing it")
    args = ap.parse_args()
    found = search()
    missing = sorted(set(_capi.conv_instantiations()) - set(found))
    print(f"{len(found)} rows; instantiations not reached: {missing}")
    text = render(finish_rows(found))
    path = os.path.join(ROOT, "tests", "conv_cases.py")
    if args.check:
        same = os.path.exists(path) and open(path).read() == text
        print("table reproduced" if same else "table DIFFERS from the committed one")
        return 0 if same and set(missing) == set(UNREACHED) else 1
    with open(path, "w") as fh:
        fh.write(text)
    return 0 if set(missing) == set(UNREACHED) else 1


if __name__ == "__main__":
    sys.exit(main())
