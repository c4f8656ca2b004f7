#!/usr/bin/env python3
"""Finds, for every conv kernel instantiation launch_conv can name, the cheapest launch that reaches it - and writes tests/conv_cases.py.

The library says which instantiations exist (rtd_debug_conv_instantiations) and what a described launch would run under the debug
options as they stand (rtd_debug_conv_choice: the launchers' own checks and choice functions, host arithmetic only).  This tool walks
the candidate grid stated below, asks for every candidate and keeps, per instantiation key, the candidate with the fewest
multiply-accumulates; ties go to a ragged last pixel tile, then to a partial last channel tile, then to the earlier candidate.
Besides one row per instantiation (one-pass, S = 1) it keeps, per (stages, bn) group of the flexible and the fixed pair tiles, the
cheapest launch with S = 2 and with S = 4 slices of the two-pass split-K.  Each row then gets its residual mode, output type and
activation by rotation within its family (kept only if the choice does not move), so that every family sees all of them.
A second table, tests/conv_view_cases.py, puts every kernel family on channel-slice views (VIEW_MATRIX below: forms x families, the
cheapest launch per cell as rtd_debug_conv_choice_views answers for the views' strides).

Needs no GPU.   python tools/conv_case_search.py [--check]     (--check: compare with the committed tables, write nothing)
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
    return f["B"] * oh * ow * f["Cout"] * (f["k"] * f["k"] * f["Cin"] + f["C2"] + f.get("Cnext", 0))


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


# ======== the second table: the families on channel-slice views (tests/conv_view_cases.py) ===============================================
# The networks run launch_conv on slices of concat buffers (Tensor::slice_c): pixel strides ldx / ldy / ldres / ldx2 wider than the channel
# counts, batch strides h * w * ld.  VIEW_CASES holds, per cell of the matrix below, the cheapest launch (same MAX_MACS, MIN_K_STEPS,
# MIN_PIXEL_TILES and tie rules as above) that rtd_debug_conv_choice_views puts on that cell's family.  Every row has B >= 2: a batch
# stride that differs from h * w * c is part of what a view is.
#   V   x and y are slices                                     R   V + a residual from a third buffer, ldx, ldy, ldres pairwise different
#   S2  3x3 / stride 2 / pad 1 (one row with odd H and W: the last window reaches the bottom / right padding; one with even: it does not)
#   K   two-pass split-K (S = 2 and S = 4) with a residual and SiLU          D   second input x2 read from a slice          U   D + x_up2
VIEW_MATRIX = {
    "V": ("tile.bf16.smallc0", "tile.bf16.smallc1", "tile.f32.smallc0", "tile.f32.smallc1", "ws.bf16", "ws.f32", "wsf", "wsq", "wsx", "sx", "reg3x3", "reg3x3_64"),
    "R": ("tile.bf16", "tile.f32", "ws.bf16", "ws.f32", "wsf", "wsq", "wsx", "sx"),
    "S2": ("tile.bf16", "tile.f32", "ws.bf16", "ws.f32", "wsf", "wsq", "wsx"),
    "K": ("wsf", "wsx"),
    "D": ("ws.bf16", "ws.f32", "pair", "sx"),          # pair: one of the pair tile families (wsf / wsq / wsx), the cheapest
    "U": ("ws", "pair"),                               # ws: bf16 or fp32 operands, the cheaper
}
PAIR_TILES = ("wsf", "wsq", "wsx")
RES_PRE, RES_POST = 1, 2


def view_cells():
    """Every cell name of the matrix: '<form>:<family cell>' plus ':odd' / ':even' (S2) or '@S2' / '@S4' (K)."""
    out = []
    for frm, cells in VIEW_MATRIX.items():
        for cell in cells:
            tails = {"S2": (":odd", ":even"), "K": ("@S2", "@S4")}.get(frm, ("",))
            out += [f"{frm}:{cell}{t}" for t in tails]
    return out


def view_geometry(f):
    """The buffers [c0 | C | c1] a row's tensors are slices of, as (c0, c1) per tensor: multiples of 32 channels (the small-channel rows'
    input: of 8), different per tensor, and widened until the pixel strides of x, y, res (and x2) are pairwise different."""
    g = dict(x=(8, 16) if f["Cin"] % 32 else (32, 32), y=(64, 32))
    if f["res_mode"]:
        g["res"] = (32, 96)
    if f["C2"]:
        g["x2"] = (96, 64)
    width = dict(x=f["Cin"], y=f["Cout"], res=f["Cout"], x2=f["C2"])
    seen = set()
    for t in ("y", "res", "x2", "x"):
        if t not in g:
            continue
        c0, c1 = g[t]
        while width[t] + c0 + c1 in seen:
            c1 += 32
        g[t] = (c0, c1)
        seen.add(width[t] + c0 + c1)
    return g


def view_ld(f, t):
    width = dict(x=f["Cin"], y=f["Cout"], res=f["Cout"], x2=f["C2"])[t]
    return width + sum(f["views"][t]) if t in f["views"] else 0


def predict_view(f):
    return _capi.conv_choice_views(DT[f["dtype"]], f["B"], f["H"], f["W"], f["Cin"], f["Cout"], view_ld(f, "x"), view_ld(f, "y"), f["k"], f["stride"], f["pad"],
                                   f["res_mode"], view_ld(f, "res"), f["out_f32"], f["C2"], view_ld(f, "x2"), f["x_up2"])


def vform(frm, **kw):
    f = dict(FORM_DEFAULTS, form=frm, **kw)
    del f["Cnext"], f["avg"], f["pool"]                  # the fused consumers take dense tensors (not part of this table)
    f["views"] = view_geometry(f)
    return f


def view_candidates():
    """(option set, launch) in a fixed order: the stated grid of the view table."""
    plain_hw = [(7, 9), (16, 16), (33, 29), (64, 64), (65, 63), (112, 112), (113, 111), (128, 128)]
    pair_hw = [(8, 11), (13, 11), (10, 26), (20, 26), (33, 8), (20, 52), (29, 31), (33, 29), (40, 40), (57, 36)]
    for frm in ("V", "R"):
        res = RES_PRE if frm == "R" else 0
        for dt, opt, k, cin, cout, B, (H, W) in itertools.product(("bf16", "f32"), ("default", "mode1"), (1, 3), (8, 32, 64, 128), (32, 64, 128, 512), (2, 4), plain_hw):
            yield opt, vform(frm, dtype=dt, B=B, H=H, W=W, Cin=cin, Cout=cout, k=k, pad=k // 2, res_mode=res)
        for opt, k, cin, cout, B, (H, W) in itertools.product(("flex", "quad") + FIXED_SETS, (1, 3), (32, 64, 512), (64, 96, 192), (2, 3), pair_hw):
            yield opt, vform(frm, dtype="f16x2", B=B, H=H, W=W, Cin=cin, Cout=cout, k=k, pad=k // 2, res_mode=res)
        for cin, cout, (H, W) in itertools.product((64, 128), (256, 512), ((80, 80), (81, 80))):
            yield "default", vform(frm, dtype="f16x2", B=2, H=H, W=W, Cin=cin, Cout=cout, res_mode=res)
    for cin, cout, H, W in itertools.product((32, 64), (32, 64), (57, 58, 121, 122), (97, 98, 113, 114)):
        yield "default", vform("V", dtype="f16x2", B=2, H=H, W=W, Cin=cin, Cout=cout, k=3, pad=1)
    # stride 2: H = 2 OH - 1 (odd) or 2 OH (even) for the same output extents
    for odd, dt, opt, cin, cout, B, (OH, OW) in itertools.product((1, 0), ("bf16", "f32"), ("default", "mode1"), (8, 32, 64), (32, 64, 128, 512), (2, 4), plain_hw):
        yield opt, vform("S2", dtype=dt, B=B, H=2 * OH - odd, W=2 * OW - odd, Cin=cin, Cout=cout, k=3, stride=2, pad=1)
    for odd, opt, cin, cout, B, (OH, OW) in itertools.product((1, 0), ("flex", "quad") + FIXED_SETS, (32, 64), (64, 96, 192), (2, 3), pair_hw):
        yield opt, vform("S2", dtype="f16x2", B=B, H=2 * OH - odd, W=2 * OW - odd, Cin=cin, Cout=cout, k=3, stride=2, pad=1)
    # two-pass split-K: >= 128 K-steps on <= 16 (S = 2) or <= 8 (S = 4) tiles per image; 3x3 only, as the networks' split-K launches on
    # views are (a Bottleneck's 3x3 with its shortcut as residual), so that the slices walk taps with a halo
    for opt, cin, cout, B, (H, W) in itertools.product(("flex",) + FIXED_SETS, (512, 576), (64, 96, 128), (2, 3), pair_hw):
        yield opt, vform("K", dtype="f16x2", B=B, H=H, W=W, Cin=cin, Cout=cout, k=3, pad=1, res_mode=RES_POST)
    # second input from a slice; x_up2: 1x1 with x at half the output extents
    for up, dt, opt, (k, cin, c2), cout, B, (H, W) in itertools.product((0, 1), ("bf16", "f32"), ("default",), ((3, 64, 64), (1, 256, 64), (1, 512, 64)), (64, 128, 512), (2, 4),
                                                                        [(16, 16), (64, 64), (66, 62), (112, 112), (114, 110), (128, 128)]):
        if not up or k == 1:
            yield opt, vform("U" if up else "D", dtype=dt, B=B, H=H, W=W, Cin=cin, C2=c2, Cout=cout, k=k, pad=k // 2, x_up2=up)
    for up, opt, (k, cin, c2), cout, B, (H, W) in itertools.product((0, 1), ("flex", "quad") + FIXED_SETS, ((3, 32, 32), (1, 256, 64)), (64, 96, 192), (2, 3),
                                                                    [(8, 12), (14, 10), (10, 26), (20, 26), (34, 8), (20, 52), (30, 32)]):
        if not up or k == 1:
            yield opt, vform("U" if up else "D", dtype="f16x2", B=B, H=H, W=W, Cin=cin, C2=c2, Cout=cout, k=k, pad=k // 2, x_up2=up)
    for H, W in ((80, 80), (81, 80)):
        yield "default", vform("D", dtype="f16x2", B=2, H=H, W=W, Cin=64, C2=64, Cout=256)


def cells_of(f, c):
    """The matrix cells a launch f with choice c may fill."""
    fam, frm = FAMILY[c["family"]], f["form"]
    named = {fam, f"{fam}.{f['dtype']}", f"{fam}.{f['dtype']}.smallc{c['smallc']}"} | ({"pair"} if fam in PAIR_TILES else set())
    if frm == "K":
        return [f"K:{n}@S{c['S']}" for n in named if n in VIEW_MATRIX["K"] and c["S"] in (2, 4)]
    if c["S"] != 1:
        return []
    tail = {"S2": ":odd" if f["H"] % 2 else ":even"}.get(frm, "")
    return [f"{frm}:{n}{tail}" for n in named if n in VIEW_MATRIX[frm]]


def search_views(only_cells=None):
    """{cell: (option set, launch, choice)}."""
    best, by_opt = {}, {}
    for opt, f in view_candidates():
        by_opt.setdefault(opt, []).append(f)
    for opt, forms in by_opt.items():
        set_options(OPTION_SETS[opt])
        for f in forms:
            m = macs(f)
            if m > MAX_MACS:
                continue
            c = predict_view(f)
            if c is None:
                continue
            fam = FAMILY[c["family"]]
            if fam in MIN_K_STEPS:
                oh, ow = out_hw(f)
                if k_steps(f, fam) // c["S"] < MIN_K_STEPS[fam] or f["B"] * oh * ow <= (MIN_PIXEL_TILES - 1) * tile_extent(c)[0]:
                    continue
            for cell in cells_of(f, c):
                if only_cells is not None and cell not in only_cells:
                    continue
                rm, rn = raggedness(f, c)
                score = (m, -rm, -rn)
                if cell not in best or score < best[cell][0]:
                    best[cell] = (score, opt, f, c)
    _capi.debug_option("reset", 0)
    return {n: v[1:] for n, v in best.items()}


def finish_view_rows(found):
    """Residual mode by rotation over the R rows (RES_PRE / RES_POST) and by (family + slices) over the K rows, so that each K family and
    each slice count sees both; output type and activation by rotation within a family (K rows: SiLU), kept only if the choice stays."""
    rows, turn, r_turn = [], {}, 0
    for cell in view_cells():
        if cell not in found:
            continue
        opt, f, c = found[cell]
        fam = FAMILY[c["family"]]
        set_options(OPTION_SETS[opt])
        t = turn.get(fam, 0)
        turn[fam] = t + 1
        f = dict(f)
        if f["form"] == "R":
            f["res_mode"] = (RES_PRE, RES_POST)[r_turn % 2]
            r_turn += 1
        elif f["form"] == "K":
            f["res_mode"] = (RES_POST, RES_PRE)[(VIEW_MATRIX["K"].index(cell[2:].split("@")[0]) + c["S"] // 4) % 2]
        if f["dtype"] != "f32":
            g = dict(f, out_f32=t % 2)
            c2 = predict_view(g)
            if c2 is not None and (c2["key"], c2["S"]) == (c["key"], c["S"]):
                f = g
        f["act"] = "silu" if f["form"] == "K" else ("relu", "silu", "none", "gelu")[t % 4]
        c = predict_view(f)
        rows.append(dict(name=cell, key=c["key"], S=c["S"], grid=c["grid"], opts=OPTION_SETS[opt], **f))
    _capi.debug_option("reset", 0)
    return rows


# cells of VIEW_MATRIX no launch reaches: cell -> the rule in the launch code that refuses it (tests/test_conv_choice_host.py)
UNREACHED_VIEWS = {}

VIEW_HEADER = '''"""The conv kernel families on channel-slice views, one small launch per cell of tools/conv_case_search.py's VIEW_MATRIX: GENERATED by
that tool from the library's own choice functions - edit the tool's grid, not this file.
name: '<form>:<family cell>[:odd|:even|@S<slices>]'; views: per tensor (c0, c1), the channels before and behind its slice in the buffer
[c0 | C | c1] (pixel stride c0 + C + c1); key / S / grid: what rtd_debug_conv_choice_views answers for the launch under `opts`."""

'''


def render_views(rows):
    body = "VIEW_CASES = [\n" + "".join("    " + pprint.pformat(r, width=1000, sort_dicts=False) + ",\n" for r in rows) + "]\n"
    un = "UNREACHED_VIEWS = " + pprint.pformat(UNREACHED_VIEWS, width=140) + "\n"
    return VIEW_HEADER + "# cell -> the launch-code rule that refuses it (the search finds no launch)\n" + un + "\n" + body


def write_or_check(path, text, check):
    if check:
        same = os.path.exists(path) and open(path).read() == text
        print(f"{os.path.relpath(path, ROOT)}: " + ("table reproduced" if same else "table DIFFERS from the committed one"))
        return same
    with open(path, "w") as fh:
        fh.write(text)
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with tests/conv_cases.py and tests/conv_view_cases.py instead of writing them")
    args = ap.parse_args()
    found = search()
    missing = sorted(set(_capi.conv_instantiations()) - set(found))
    print(f"{len(found)} rows; instantiations not reached: {missing}")
    ok = write_or_check(os.path.join(ROOT, "tests", "conv_cases.py"), render(finish_rows(found)), args.check)
    views = search_views()
    no_view = sorted(set(view_cells()) - set(views))
    print(f"{len(views)} view rows; cells not reached: {no_view}")
    ok = write_or_check(os.path.join(ROOT, "tests", "conv_view_cases.py"), render_views(finish_view_rows(views)), args.check) and ok
    return 0 if ok and set(missing) == set(UNREACHED) and set(no_view) == set(UNREACHED_VIEWS) else 1


if __name__ == "__main__":
    sys.exit(main())
