"""The conv kernels across the pair format's range: which rows run with scaled operands, how the scales are drawn, and the per-element
gate (pure Python and torch on the CPU; tests/test_gpu_conv_range.py launches, tests/test_conv_range_host.py holds the gate itself).

The pair format is not scale-free: hi = fp16(x), lo = fp16(x - hi) carries 22 significant bits only for |x| >= 2^-3, an absolute
2^-25 below that, and saturates at +-65504 (csrc/common.h).  A tensor-wide bound (max err / max |y|) cannot see a channel whose
magnitude is 2^-10 of the largest one's.  So the operands get per-channel power-of-two scales and every output element i is held to
    |got_i - want_i| <= F rho A_i + floor_i,
  A_i     = sum_k |x_k| |w_k| + |b_i| (+ |res_i|) in fp64 on the values the kernel sees: it carries the scales, so the bound is scale-free;
  rho     = max(max_i |y32_i - want_i| / A_i, 2^-24) with y32 the same computation in torch fp32 on the CPU: the yardstick;
  floor_i = 2^-25 where the output is a pair and |want_i| < 2^-3 (the format's documented floor), else 0;
  F       = 8 for pairs, the factor of tests/test_gpu_eva.py (4 for the two significant bits the pair lacks against fp32, times 2 for the
            dropped lo * lo term and the spread of a maximum).
            fp32: 3.4.  That file's 2 (accumulation order only) is too tight for the order these kernels have: one accumulator per
            element, walked sequentially over K as a chain of fp32 fused multiply-adds, against torch's blocked sums.
            tools/conv_f32_order.py restates that chain on the CPU; the kernels' outputs (ws.f32.s2.bn128 3x3 at K = 288, 4 194 304
            elements; tile.f32.64x64.smallc0 3x3 at K = 576, 6144 elements) equal it BIT FOR BIT, so the restatement's ratio is the
            kernel's by construction.  Its worst over the fp32 rows is 1.70 (K = 576) with the yardstick of the build host's torch,
            and F = 2 x 1.70.  rho depends on the host's torch: with the MI355X host's CPU the same bits read 2.35 at most
            (EXPERIMENTS.md has every figure)."""
import torch
import torch.nn.functional as F

from tests.conv_cases import CASES
from tests.conv_reference import conv_ref, epilogue_ref
from tests.conv_served_cases import SERVED_CASES

FACTOR = {"f16x2": 8.0, "f32": 3.4}             # f32: 2 x 1.70, tools/conv_f32_order.py
RHO_MIN = 2.0 ** -24
PAIR_FLOOR, PAIR_FLOOR_BELOW, PAIR_MAX = 2.0 ** -25, 2.0 ** -3, 65504.0
E_RANGE, F_RANGE = (-8, 4), (-10, 6)             # exponents of the input channels / of the output channels, both ends included
SATURATING_F = 16                                # part B: the last 32-channel group's exponent


# ---- the rows ----------------------------------------------------------------------------------------------------------------------------
def family(key):
    p = key.split(".")
    if p[0] in ("wsf", "wsx"):
        return f"{p[0]}.{p[1]}"                  # wsf.s2, wsf.s3, wsx.s2, wsx.s4
    if p[0] in ("wsq", "sx"):
        return p[0]
    if p[0] in ("tile", "ws"):
        return f"{p[0]}.{p[1]}"                  # tile.f32, ws.f32
    assert p[0].startswith("reg3x3"), key
    return key                                   # each direct 3x3 kernel on its own


def out_extents(r):
    return (r["H"] + 2 * r["pad"] - r["k"]) // r["stride"] + 1, (r["W"] + 2 * r["pad"] - r["k"]) // r["stride"] + 1


def macs(r):
    OH, OW = out_extents(r)
    return r["B"] * OH * OW * r["Cout"] * (r["k"] * r["k"] * r["Cin"] + r["C2"] + r["Cnext"])


def signature(r):
    """(dtype, family, residual mode, fp32 rows out, S > 1, follower, avg, second input, x_up2, pool)"""
    return (r["dtype"], family(r["key"]), r["res_mode"], r["out_f32"], r["S"] > 1, r["Cnext"] > 0, r["avg"], r["C2"] > 0, r["x_up2"], r["pool"])


def candidates():
    """bf16 shares fp32's exponent range: left out"""
    return [r for r in CASES + SERVED_CASES if r["dtype"] != "bf16"]


def choose_rows():
    """The cheapest row (MACs) of every signature; then, per (dtype, family), the cheapest row of each activation the family has in the
    tables and the choice lacks."""
    rows = candidates()
    best = {}
    for r in rows:
        s = signature(r)
        if s not in best or macs(r) < macs(best[s]):
            best[s] = r
    chosen = list(best.values())
    for dt, fam in sorted({(r["dtype"], family(r["key"])) for r in rows}):
        of_family = [r for r in rows if (r["dtype"], family(r["key"])) == (dt, fam)]
        have = {r["act"] for r in chosen if (r["dtype"], family(r["key"])) == (dt, fam)}
        for act in sorted({r["act"] for r in of_family} - have):
            chosen.append(min((r for r in of_family if r["act"] == act), key=macs))
    return sorted(chosen, key=lambda r: r["name"])


RANGE_CASES = choose_rows()


def family_rows():
    """Part B: per kernel family the cheapest of RANGE_CASES - with relu where the family has a relu row in the tables, else the row's
    own activation (the activation is a kernel argument: it does not enter the kernel choice, and the tests assert the key) - and the
    cheapest two-pass split-K row, whose epilogue is k_splitk_reduce's."""
    out = []
    groups = sorted({family(r["key"]) for r in RANGE_CASES})
    for fam in groups:
        r = min((r for r in RANGE_CASES if family(r["key"]) == fam), key=macs)
        relu = any(c["act"] == "relu" for c in candidates() if family(c["key"]) == fam)
        out.append(dict(r, act="relu" if relu else r["act"], family=fam))
    r = min((r for r in RANGE_CASES if r["S"] > 1), key=macs)
    out.append(dict(r, act="relu", family="splitk"))
    r = min((r for r in RANGE_CASES if r["Cnext"]), key=macs)     # the follower's own epilogue (next_act, always relu): y1
    out.append(dict(r, act="relu", family="sx.next"))
    return out


FAMILY_CASES = family_rows()


# ---- the scales ----------------------------------------------------------------------------------------------------------------------------
def draw_scales(g, r):
    """The hook of Operands(row, scales): integer exponents from the row-seeded generator, after the operands' own draws."""
    draw = lambda n, lo_hi: torch.randint(lo_hi[0], lo_hi[1] + 1, (n,), generator=g)
    e = draw(r["Cin"], E_RANGE)
    f = draw(r["Cout"], F_RANGE)
    e2 = draw(r["C2"], E_RANGE) if r["C2"] else None
    return dict(e=e, e2=e2, f=f)


def draw_saturating_scales(g, r):
    """... with the last 32-channel group's pre-activations beyond +-65504"""
    s = draw_scales(g, r)
    s["f"][-32:] = SATURATING_F
    return s


# ---- the references of a row (ops: an Operands of tests/test_gpu_conv_instances.py) ------------------------------------------------------------
def references(ops):
    """(want fp64, y32 = the same in torch fp32 as fp64, A = sum |x| |w| + |b| (+ |res|)) of the row's y, on the seen values"""
    r = ops.row
    conv = lambda dtype: conv_ref(ops.xv, ops.wv, ops.b, r["k"], r["pad"], ops.x2v, r["stride"], r["x_up2"], dtype=dtype)
    want = epilogue_ref(conv(torch.float64), r["act"], r["res_mode"], ops.rv)
    y32 = epilogue_ref(conv(torch.float32), r["act"], r["res_mode"], ops.rv).double()
    A = conv_ref(ops.xv.abs(), ops.wv.abs(), ops.b.abs(), r["k"], r["pad"], ops.x2v.abs() if ops.x2v is not None else None, r["stride"], r["x_up2"])
    if r["res_mode"]:
        A = A + ops.rv.double().abs()
    return want, y32, A


def follower_references(ops, got):
    """... of y1 = relu(W1 y + b1), from the kernel's own y"""
    w1, b1 = ops.w1v.double(), ops.b1.double()
    want = F.relu(got @ w1.t() + b1)
    y32 = F.relu(got.float() @ ops.w1v.t() + ops.b1).double()
    return want, y32, got.abs() @ w1.abs().t() + b1.abs()


def columns(ops):
    """fp32 [M, K]: the unfolded input of a row without a second input, tap-major / channel-minor (conv_ref's columns)"""
    r, xv = ops.row, ops.xv
    assert not r["C2"] and not r["x_up2"]
    B, H, W, Cin = xv.shape
    k = r["k"]
    if k == 1 and r["stride"] == 1:
        return xv.reshape(B * H * W, Cin)
    u = F.unfold(xv.permute(0, 3, 1, 2), k, padding=r["pad"], stride=r["stride"])
    return u.reshape(B, Cin, k * k, u.shape[-1]).permute(0, 3, 2, 1).reshape(-1, k * k * Cin)


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------
def yardstick(want, y32, A):
    """rho: the worst error of torch fp32 against fp64 in units of A (NaN elements of the reference left out)"""
    q = (y32.double() - want).abs() / A
    q = q[~torch.isnan(want)]
    return max(float(q.max()), RHO_MIN)


def bounds(want, A, rho, pair_out):
    """(rho A_i, floor_i) per element"""
    floor = torch.where(want.abs() < PAIR_FLOOR_BELOW, PAIR_FLOOR, 0.0).to(torch.float64) if pair_out else torch.zeros_like(want)
    return rho * A, floor


def worst_ratio(got, want, rhoA, floor):
    """max_i (err_i - floor_i) / (rho A_i) over the elements whose reference is a number"""
    ok = ~torch.isnan(want)
    return float((((got - want).abs() - floor) / rhoA)[ok].max())


def assert_gate(what, got, want, rhoA, floor, factor):
    """every element whose reference is a number: a number, and |got - want| <= factor rho A + floor; returns (and prints) the ratio"""
    ok = ~torch.isnan(want)
    ratio = worst_ratio(got, want, rhoA, floor)
    print(f"{what}: max (err - floor) / (rho A) {ratio:.2f} (gate {factor:g})")
    assert torch.isfinite(got[ok]).all(), (what, "non-finite elements where the reference is finite")
    bad = ((got - want).abs() > factor * rhoA + floor) & ok
    assert not bad.any(), (what, ratio, factor, int(bad.sum()), bad.nonzero()[:4].tolist())
    return ratio


def tensor_wide_ok(got, want):
    """the bound the other conv tests hold pairs to: max err / max |y| < 2e-5 and rel-l2 < 1e-5"""
    err = (got - want).abs().max().item() / want.abs().max().item()
    rel = (torch.linalg.norm(got - want) / torch.linalg.norm(want)).item()
    return err < 2e-5 and rel < 1e-5


# ---- the pair arithmetic on the CPU (the host test's honest kernel and its mutants) --------------------------------------------------------
FP16_MIN_NORMAL = 2.0 ** -14


def split2(v):
    """fp32 -> (hi, lo) as fp32 tensors holding fp16 values: csrc/common.h split2"""
    v = v.float().clamp(-PAIR_MAX, PAIR_MAX)
    hi = v.half().float()
    return hi, (v - hi).half().float()


def flush_subnormal(t):
    return torch.where(t.abs() < FP16_MIN_NORMAL, torch.zeros_like(t), t)


def pair_gemm(x, w, b, res=None, act=lambda t: t, res_mode=0, mutant=None):
    """y = split2(epilogue(x w^T + b)) as the pair kernels compute it: hi hi + hi lo + lo hi with fp32 accumulation (every product of
    two fp16 values is exact in fp32), bias, residual and activation in fp32, one hi / lo rounding of the output.  x [M, K], w [N, K]:
    seen (pair) values.  mutant: None, or
      'flush_lo_out'   the epilogue flushes subnormal lo halves of the output,
      'drop_lo_hi'     the x_lo * w_hi term is lost in the last 32 K-columns,
      'drop_hi_lo'     the x_hi * w_lo term is lost in the last 32 K-columns,
      'flush_operands' the matrix cores flush fp16 subnormal operands."""
    xh, xl = split2(x)
    wh, wl = split2(w)
    if mutant == "flush_operands":
        xh, xl, wh, wl = (flush_subnormal(t) for t in (xh, xl, wh, wl))
    xl_lh, wl_hl = xl, wl
    if mutant == "drop_lo_hi":
        xl_lh = xl.clone()
        xl_lh[:, -32:] = 0
    if mutant == "drop_hi_lo":
        wl_hl = wl.clone()
        wl_hl[:, -32:] = 0
    v = (xh @ wl_hl.t() + xl_lh @ wh.t()) + xh @ wh.t() + b.float()
    if res_mode == 1:
        v = v + res.float()
    v = act(v)
    if res_mode == 2:
        v = v + res.float()
    hi, lo = split2(v)
    if mutant == "flush_lo_out":
        lo = flush_subnormal(lo)
    return (hi + lo).double()
