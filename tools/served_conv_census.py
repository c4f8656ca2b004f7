#!/usr/bin/env python3
"""Lists every conv launch the served networks make, asks the library which kernel each one runs, and writes tests/conv_served_cases.py:
one small launch per launch signature that no row of tests/conv_cases.py or tests/conv_view_cases.py already has.

The kernel choice depends on M = B * OH * OW (the grid is held near the CU count), so the kernels that run at the served sizes are not
the ones the small network tests run, and they run in combinations (stride, residual mode, fp32 rows out, activation) the kernel tables
do not launch.  A launch SIGNATURE is (dtype, kernel key, split-K slices S, k, stride, residual mode, fp32 rows out, activation).
The launch lists below restate three plan builders in Python (yolox_net.hip's Net::build, classifier.hip's and esrgan.hip's build_plan);
tests/test_gpu_conv_served.py holds them against the real plans through rtd_debug_*_plan_convs.

For a signature without a row the tool shrinks the first served launch that has it - B, H and W only; Cin, Cout, k, stride, activation,
residual mode and the views' pixel strides stay - to the cheapest launch that still lands on the same key and S.  Among the launches
found it prefers one whose M leaves the served launch's remainder in the kernel's pixel tile; failing that the most ragged one
(conv_case_search.raggedness).  conv_case_search.MAX_MACS caps a row.

Needs no GPU.   python tools/served_conv_census.py [--check]     (--check: compare with the committed table, write nothing)
Regenerate whenever choose_pair, choose_plain or one of the three plan builders changes: tests/test_conv_served_host.py fails until then.
"""
import argparse
import os
import pprint
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from telescope_cam_detection_amd import _capi  # noqa: E402
from telescope_cam_detection_amd.esrgan import conv_table as esrgan_conv_table  # noqa: E402
from telescope_cam_detection_amd.eva_checkpoint import EvaArch, pad32  # noqa: E402
from telescope_cam_detection_amd.yolox_network import FOCUS_C, conv_table as yolox_conv_table  # noqa: E402
from tools import conv_case_search as ccs  # noqa: E402

# ---- the served configurations ----------------------------------------------------------------------------------------------------------
ENGINES = ("f16x2", "f32")                                   # RTD_PREC_F16X3 (pair storage) and RTD_PREC_FP32
YOLOX_VARIANTS = {"yolox-s": (32, 1), "yolox-l": (64, 3)}    # name -> (base channels, depth): the two variants yolox_net_host.h serves
YOLOX_CLASSES = 80                                           # COCO
YOLOX_INPUT = (640, 640)                                     # YoloxNetwork's default input_size
YOLOX_BATCHES = tuple(range(1, 9))                           # ... and 1..max_batch (default 8)
EVA_ARCH = EvaArch()                                         # ViT-L/14-336 as tools/eva_bench.py describes it: dim 1024, hidden 2730, 577 tokens, 10 000 classes
EVA_BATCHES = tuple(range(1, 17))                            # 1..max_batch of classifier.py (default 16)
ESRGAN_BLOCKS = 23                                           # RRDBNet x4plus (CropUpscaler's default)
ESRGAN_CROPS = ((64, 64), (96, 128), (128, 128), (200, 150), (256, 256), (512, 512))   # (h, w): one pass each at the default tile 512

RES_NONE, RES_PRE, RES_POST = 0, 1, 2
MAX_UNREACHED = 6


# ---- the three plans, restated ------------------------------------------------------------------------------------------------------------
class T:
    """A channel-slice view as Tensor::slice_c makes it: c channels at offset c0 of a buffer of ld channels per pixel."""

    def __init__(self, c, ld=None, c0=0, f32=False):
        self.c, self.ld, self.c0, self.f32 = c, (c if ld is None else ld), c0, f32

    def slice_c(self, c0, c):
        return T(c, self.ld, self.c0 + c0, self.f32)

    def views(self):
        return (self.c0, self.ld - self.c0 - self.c)


def launch(name, dtype, B, H, W, x, y, k, stride, act, res=None, res_mode=RES_NONE):
    """One conv launch as the plans describe it.  H, W: the input's extents.  out_f32: fp32 rows out of pair operands."""
    f = dict(name=name, dtype=dtype, B=B, H=H, W=W, Cin=x.c, Cout=y.c, k=k, stride=stride, pad=(k - 1) // 2, act=act,
             res_mode=res_mode if res is not None else RES_NONE, out_f32=int(y.f32 and dtype != "f32"),
             ldx=x.ld, ldy=y.ld, ldres=res.ld if res is not None else 0)
    views = dict(x=x.views(), y=y.views())
    if res is not None:
        views["res"] = res.views()
    if any(v != (0, 0) for v in views.values()):
        f["views"] = views
    return f


def yolox_launches(variant, n, dtype, input_size=YOLOX_INPUT, num_classes=YOLOX_CLASSES):
    """yolox_net.hip, Net::build: the convs in execution order, named as yolox_net_host.h's conv_table names them."""
    base, d = YOLOX_VARIANTS[variant]
    names = [t[0] for t in yolox_conv_table(base, d)]
    for l in range(3):                                       # the table of the package stops before the pred convs
        at = names.index(f"head.reg_convs.{l}.1") + 1
        names[at:at] = [f"head.cls_preds.{l}", f"head.regobj_preds.{l}"]
    out, H, W = [], input_size[0], input_size[1]
    hh, ww = [H >> i for i in range(6)], [W >> i for i in range(6)]
    c3, c4, c5, hc = 4 * base, 8 * base, 16 * base, 4 * base

    def conv(tail, x, y, xh, xw, k=1, stride=1, act="silu", res=None):
        name = names[len(out)]
        assert name.endswith(tail), (name, tail)
        out.append(launch(name, dtype, n, xh, xw, x, y, k, stride, act, res, RES_POST))

    def csp(tail, x, y, h_, w_, nb, shortcut):
        h = y.c // 2
        cat, A, B_, Tm = T(2 * h), T(h), T(h), T(h)
        conv(tail + ".conv1", x, A, h_, w_)
        conv(tail + ".conv2", x, cat.slice_c(h, h), h_, w_)
        cur = A
        for i in range(nb):
            dst = cat.slice_c(0, h) if i == nb - 1 else (B_ if cur is A else A)
            conv(f"{tail}.m.{i}.conv1", cur, Tm, h_, w_)
            conv(f"{tail}.m.{i}.conv2", Tm, dst, h_, w_, k=3, res=cur if shortcut else None)
            cur = dst
        conv(tail + ".conv3", cat, y, h_, w_)

    focus, stem = T(FOCUS_C), T(base)
    conv("stem.conv", focus, stem, hh[1], ww[1], k=3)
    p3cat, p4cat, n3cat, n4cat = T(2 * c3), T(2 * c4), T(2 * c3), T(2 * c4)
    dark2, dark3, dark4, dark5 = T(2 * base), p3cat.slice_c(c3, c3), p4cat.slice_c(c4, c4), T(c5)
    x = stem
    for s, o in enumerate((dark2, dark3, dark4)):
        down = T(base << (s + 1))
        conv(f"dark{s + 2}.0", x, down, hh[s + 1], ww[s + 1], k=3, stride=2)
        csp(f"dark{s + 2}.1", down, o, hh[s + 2], ww[s + 2], d if s == 0 else 3 * d, True)
        x = o
    down, sppcat, spp = T(c5), T(2 * c5), T(c5)
    conv("dark5.0", x, down, hh[4], ww[4], k=3, stride=2)
    conv("dark5.1.conv1", down, sppcat.slice_c(0, c5 // 2), hh[5], ww[5])
    conv("dark5.1.conv2", sppcat, spp, hh[5], ww[5])
    csp("dark5.2", spp, dark5, hh[5], ww[5], d, False)
    fpn_out0, fpn_out1 = n4cat.slice_c(c4, c4), n3cat.slice_c(c3, c3)
    f0, pan_out2, pan_out1, pan_out0 = T(c4), T(c3), T(c4), T(c5)
    conv("lateral_conv0", dark5, fpn_out0, hh[5], ww[5])
    csp("C3_p4", p4cat, f0, hh[4], ww[4], d, False)
    conv("reduce_conv1", f0, fpn_out1, hh[4], ww[4])
    csp("C3_p3", p3cat, pan_out2, hh[3], ww[3], d, False)
    conv("bu_conv2", pan_out2, n3cat.slice_c(0, c3), hh[3], ww[3], k=3, stride=2)
    csp("C3_n3", n3cat, pan_out1, hh[4], ww[4], d, False)
    conv("bu_conv1", pan_out1, n4cat.slice_c(0, c4), hh[4], ww[4], k=3, stride=2)
    csp("C3_n4", n4cat, pan_out0, hh[5], ww[5], d, False)
    for l, lv in enumerate((pan_out2, pan_out1, pan_out0)):
        lh, lw = hh[l + 3], ww[l + 3]
        st, cf, rf, t = T(hc), T(hc), T(hc), T(hc)
        conv(f"stems.{l}", lv, st, lh, lw)
        conv(f"cls_convs.{l}.0", st, t, lh, lw, k=3)
        conv(f"cls_convs.{l}.1", t, cf, lh, lw, k=3)
        conv(f"reg_convs.{l}.0", st, t, lh, lw, k=3)
        conv(f"reg_convs.{l}.1", t, rf, lh, lw, k=3)
        conv(f"cls_preds.{l}", cf, T(pad32(num_classes), f32=True), lh, lw, act="none")
        conv(f"regobj_preds.{l}", rf, T(32, f32=True), lh, lw, act="none")
    assert len(out) == len(names)
    return out


def eva_launches(n, dtype, arch=EVA_ARCH):
    """classifier.hip, build_plan: every linear layer is a 1x1 conv over one image of n * rows pixels."""
    D, G = arch.dim, arch.img // arch.patch
    L, Kp, Hp, Cp = G * G + 1, pad32(3 * arch.patch ** 2), pad32(arch.hidden), pad32(arch.classes)
    out = []

    def conv(name, rows, cin, cout, res=False, f32=False):
        out.append(launch(name, dtype, 1, 1, rows, T(cin), T(cout, f32=f32), 1, 1, "none", T(cout) if res else None, RES_PRE))

    conv("patch_embed", n * G * G, Kp, D)
    for i in range(arch.depth):
        b = f"blocks.{i}"
        conv(b + ".attn.qkv", n * L, D, 3 * D)
        conv(b + ".attn.proj", n * L, D, D, res=True)
        conv(b + ".mlp.fc1", n * L, D, 2 * Hp)
        conv(b + ".mlp.fc2", n * L, Hp, D, res=True)
    conv("head", n, D, Cp, f32=True)
    return out


def esrgan_launches(h, w, dtype, num_block=ESRGAN_BLOCKS):
    """esrgan.hip, build_plan: RRDBNet on one h x w tile; a dense block's convs read and write slices of one 192-channel buffer."""
    names = [t[0] for t in esrgan_conv_table(num_block)]
    out = []

    def conv(x, y, hh, ww, act, res=None):
        out.append(launch(names[len(out)], dtype, 1, hh, ww, x, y, 3, 1, act, res, RES_PRE))

    feat, d = T(64), (T(192), T(192), T(192))
    conv(T(32), feat, h, w, "none")
    for _ in range(num_block):
        order = (0, 1, 2, 1)
        for j in range(3):
            cur, nxt = d[order[j]], d[order[j + 1]]
            for k in range(1, 5):
                conv(cur.slice_c(0, 64 + 32 * (k - 1)), cur.slice_c(64 + 32 * (k - 1), 32), h, w, "lrelu")
            conv(cur, nxt.slice_c(0, 64), h, w, "none", cur.slice_c(0, 64))
    conv(d[0].slice_c(0, 64), d[1].slice_c(0, 64), h, w, "none", feat)
    conv(T(64), T(64), 2 * h, 2 * w, "lrelu")
    conv(T(64), T(64), 4 * h, 4 * w, "lrelu")
    conv(T(64), T(64), 4 * h, 4 * w, "lrelu")
    conv(T(64), T(32, f32=True), 4 * h, 4 * w, "none")
    assert len(out) == len(names)
    return out


def served_configurations():
    """(configuration name, launches) in a fixed order."""
    for dtype in ENGINES:
        for variant in YOLOX_VARIANTS:
            for n in YOLOX_BATCHES:
                yield f"{variant} n={n} {dtype}", yolox_launches(variant, n, dtype)
        for n in EVA_BATCHES:
            yield f"eva-vitl n={n} {dtype}", eva_launches(n, dtype)
        for h, w in ESRGAN_CROPS:
            yield f"rrdbnet {h}x{w} {dtype}", esrgan_launches(h, w, dtype)


# ---- choices and signatures -----------------------------------------------------------------------------------------------------------------
def as_form(f):
    """A launch with the fields conv_case_search's helpers read."""
    return dict(ccs.FORM_DEFAULTS, **f)


def choice(f):
    """What launch_conv would run for launch f under the default options (views: through the views' pixel strides); None = refused."""
    g = as_form(f)
    return ccs.predict_view(g) if "views" in g else ccs.predict(g)


def signature(f, c):
    return (f["dtype"], c["key"], c["S"], f["k"], f["stride"], f["res_mode"], f["out_f32"], f["act"])


def row_signature(r):
    """The signature of a row of SERVED_CASES."""
    return (r["dtype"], r["key"], r["S"], r["k"], r["stride"], r["res_mode"], r["out_f32"], r["act"])


def signature_name(sig):
    dtype, key, S, k, stride, res, f32, act = sig
    return f"{dtype}/{key}{'@S%d' % S if S > 1 else ''}/k{k}s{stride}/res{res}/{'f32rows' if f32 else 'own'}/{act}"


def census():
    """{signature: [(configuration, launch), ...]} over every served launch, in the order met.  A refused launch is an error."""
    _capi.debug_option("reset", 0)
    seen, memo = {}, {}
    for cfg, launches in served_configurations():
        for f in launches:
            geo = tuple(sorted((k, str(v)) for k, v in f.items() if k != "name"))
            if geo not in memo:
                c = choice(f)
                if c is None:
                    raise RuntimeError(f"{cfg}: {f['name']} is refused: {_capi.lib().rtd_last_error(None)}")
                memo[geo] = c
            seen.setdefault(signature(f, memo[geo]), []).append((cfg, f))
    return seen


def existing_signatures():
    """{signature: row} of the plain one-input rows of CASES and VIEW_CASES (the first row that has it)."""
    from tests.conv_cases import CASES
    from tests.conv_view_cases import VIEW_CASES
    have = {}
    for r in list(CASES) + list(VIEW_CASES):
        if r["C2"] or r["x_up2"] or r.get("Cnext") or r.get("avg") or r.get("pool"):
            continue
        out_f32 = int(r["out_f32"] and r["dtype"] != "f32")
        have.setdefault((r["dtype"], r["key"], r["S"], r["k"], r["stride"], r["res_mode"], out_f32, r["act"]), r)
    return have


# ---- the search ---------------------------------------------------------------------------------------------------------------------------------
W_DIVISORS = (1, 2, 3, 4, 6, 8, 12, 16)


def shrunk_views(f):
    """The served slice offsets shrunk to one 32-channel group each - kept only if the pixel strides stay pairwise different (and were)."""
    if "views" not in f:
        return None
    width = dict(x=f["Cin"], y=f["Cout"], res=f["Cout"])
    small = {t: (min(c0, 32), min(c1, 32)) for t, (c0, c1) in f["views"].items()}
    lds = lambda v: [width[t] + sum(v[t]) for t in v]
    served_differ = len(set(lds(f["views"]))) == len(f["views"])
    if served_differ and len(set(lds(small))) == len(small):
        return small
    return f["views"]


def candidates(f):
    """(B, H, W) no larger than the served launch's: every H, W in a few whole fractions (a linear layer: every row count)."""
    k = f["k"]
    if f["H"] == 1:
        return [(1, 1, w) for w in range(1, f["W"] + 1)]
    widths = sorted({-(-f["W"] // d) for d in W_DIVISORS if -(-f["W"] // d) >= k})
    return [(b, h, w) for b in range(1, f["B"] + 1) for h in range(k, f["H"] + 1) for w in widths]


def shrink(sig, f):
    """The row for signature sig from served launch f: (row, None), or (None, MACs of the cheapest launch found) above the cap."""
    key, S = sig[1], sig[2]
    base = as_form({k: v for k, v in f.items() if k not in ("name", "ldx", "ldy", "ldres")})
    views = shrunk_views(f)
    if views is not None:
        base["views"] = views
    served = choice(dict(base, views=f["views"]) if views is not None else base)
    pix = ccs.tile_extent(served)[0] if ccs.FAMILY[served["family"]] not in ("reg3x3", "reg3x3_64") else 1
    oh, ow = ccs.out_hw(base)
    want_rem = (base["B"] * oh * ow) % pix
    floor = min(base["B"] * oh * ow, (ccs.MIN_PIXEL_TILES - 1) * pix + 1)      # at least 3 pixel tiles, as conv_case_search asks, where the served launch has them
    cands = sorted((ccs.macs(dict(base, B=b, H=h, W=w)), b, h, w) for b, h, w in candidates(base))
    fallback, over_cap = None, None
    for m, b, h, w in cands:
        if m > ccs.MAX_MACS and (fallback is not None or over_cap is not None):
            break
        g = dict(base, B=b, H=h, W=w)
        c = choice(g)
        if c is None or c["key"] != key or c["S"] != S:
            continue
        if m > ccs.MAX_MACS:
            over_cap = m
            break
        goh, gow = ccs.out_hw(g)
        if b * goh * gow < floor:
            continue
        if (b * goh * gow) % pix == want_rem:
            return finish(sig, g, c), None
        score = tuple(-r for r in ccs.raggedness(g, c)) + (m,)
        if fallback is None or score < fallback[0]:
            fallback = (score, g, c)
    if fallback is not None:
        return finish(sig, fallback[1], fallback[2]), None
    return None, over_cap


def finish(sig, g, c):
    row = dict(name=signature_name(sig), key=c["key"], S=c["S"], grid=c["grid"], opts={})
    row.update({k: g[k] for k in ("dtype", "B", "H", "W", "Cin", "Cout", "k", "stride", "pad", "C2", "x_up2", "Cnext", "avg", "pool", "res_mode", "out_f32", "act")})
    if "views" in g:
        row["views"] = g["views"]
    return row


# The widths at which a tile's channel or K tail can go wrong, as the served networks have them: Cout = 96 (the cls pred rows), 5504 (fc1),
# 10 016 (the head: 313 x 32, no whole number of 64-wide tiles); K = 608 (patch embed), 2752 (fc2), 4608 (3 x 3 x 512).  A signature's
# first served launch need not have them, so each edge width a signature is served with gets a row of its own (`edge`).
EDGE_N, EDGE_K = (96, 5504, 10016), (608, 2752, 4608)


def edges_of(f):
    return {("N", f["Cout"])} & {("N", n) for n in EDGE_N} | {("K", f["k"] ** 2 * f["Cin"])} & {("K", k) for k in EDGE_K}


def variants_of(launches):
    """The distinct (Cin, Cout, views) among a signature's served launches, in the order met: [(launch, labels of up to three such)]."""
    out = {}
    for cfg, f in launches:
        v = out.setdefault((f["Cin"], f["Cout"], str(f.get("views"))), (f, []))
        label = f"{cfg}: {f['name']}"
        if len(v[1]) < 3 and label not in v[1]:
            v[1].append(label)
    return list(out.values())


def build_tables(seen=None):
    """(SERVED_CASES, COVERED_ELSEWHERE, UNREACHED_SERVED, EDGES_ABOVE_CAP) for the census `seen`."""
    seen = census() if seen is None else seen
    have = existing_signatures()
    rows, covered, unreached, edges_above = [], {}, {}, {}
    for sig in sorted(seen):
        variants = variants_of(seen[sig])
        if sig in have:
            covered[sig] = have[sig]["name"]
            done = edges_of(have[sig])
        else:
            row, overs = None, []
            for f, labels in variants:                       # the first channel variant that a launch below the cap reaches
                row, over = shrink(sig, f)
                if row is not None:
                    break
                overs.append((f, over))
            if row is None:
                f, over = min(overs, key=lambda t: t[1] or float("inf"))
                unreached[sig] = (f"no launch of {f['name']}'s channels ({f['Cin']} -> {f['Cout']}, k = {f['k']}, stride {f['stride']}) with B <= {f['B']}, H <= {f['H']} "
                                  f"and W <= {f['W']} lands on {sig[1]} (S = {sig[2]}) below MAX_MACS", over)
                done = set()
            else:
                row["served"] = labels
                rows.append(row)
                done = edges_of(row)
        for f, labels in variants:
            new = edges_of(f) - done
            if not new:
                continue
            row, over = shrink(sig, f)
            name = f"{signature_name(sig)}/{f['Cin']}to{f['Cout']}"
            if row is None:
                edges_above[name] = over
                continue
            row["name"] = name
            row["served"], row["edge"] = labels, sorted(new)
            rows.append(row)
            done |= edges_of(f)
    _capi.debug_option("reset", 0)
    return rows, covered, unreached, edges_above


HEADER = '''"""One small launch per launch signature of the served networks (YOLOX-s / -l at 640 x 640, EVA02 ViT-L/14-336, RRDBNet crops; both
engines) that tests/conv_cases.py and tests/conv_view_cases.py do not already launch: GENERATED by tools/served_conv_census.py from the
library's own choice functions - edit the tool's table of served configurations, not this file.
signature: (dtype, kernel key, split-K slices S, k, stride, residual mode, fp32 rows out, activation).  key / S / grid: what
rtd_debug_conv_choice (rows with `views`: rtd_debug_conv_choice_views) answers for the launch under the default options.
served: up to three served launches the row stands for.  views: per tensor (c0, c1), the channels before and behind its slice.
edge: the row is one more launch of its signature, at a served width where a tile's tail can go wrong (('N', Cout) or ('K', k k Cin))."""

'''


def render(rows, covered, unreached, edges_above):
    fmt = lambda v: pprint.pformat(v, width=1000, sort_dicts=False)
    text = HEADER + "# signature -> (why no launch below MAX_MACS reaches it, the MACs of the cheapest launch found or None)\nUNREACHED_SERVED = {\n"
    text += "".join(f"    {fmt(k)}: {fmt(v)},\n" for k, v in unreached.items()) + "}\n\n"
    text += "# signature -> the row of CASES / VIEW_CASES that has it\nCOVERED_ELSEWHERE = {\n"
    text += "".join(f"    {fmt(k)}: {fmt(v)},\n" for k, v in covered.items()) + "}\n\n"
    text += "# edge-width launches no launch below MAX_MACS reaches: name -> the MACs of the cheapest launch found (their signatures have a row)\nEDGES_ABOVE_CAP = {\n"
    text += "".join(f"    {fmt(k)}: {fmt(v)},\n" for k, v in edges_above.items()) + "}\n\n"
    text += "SERVED_CASES = [\n" + "".join("    " + fmt(r) + ",\n" for r in rows) + "]\n"
    return text


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with tests/conv_served_cases.py instead of writing it")
    args = ap.parse_args()
    seen = census()
    rows, covered, unreached, edges_above = build_tables(seen)
    print(f"{sum(len(v) for v in seen.values())} served launches, {len(seen)} signatures: {sum('edge' not in r for r in rows)} rows + {sum('edge' in r for r in rows)} edge "
          f"rows, {len(covered)} covered elsewhere, {len(unreached)} unreached, {len(edges_above)} edge widths above the cap")
    for sig, why in unreached.items():
        print("  unreached:", signature_name(sig), why)
    ok = ccs.write_or_check(os.path.join(ROOT, "tests", "conv_served_cases.py"), render(rows, covered, unreached, edges_above), args.check)
    return 0 if ok and len(unreached) <= MAX_UNREACHED else 1


if __name__ == "__main__":
    sys.exit(main())
