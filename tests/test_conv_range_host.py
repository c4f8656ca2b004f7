"""Host: the row choice of tests/conv_range_cases.py is pinned, and its per-element gate can fail - it passes the pair arithmetic
restated on the CPU (hi hi + hi lo + lo hi in fp32, one hi / lo rounding of the output) under per-channel power-of-two scales, and
rejects four ways a pair kernel can be subtly wrong, one of which the tensor-wide bound of the other conv tests accepts."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_range_cases as cr

EPILOGUES = {                                    # name -> (activation, residual mode)
    "none": (lambda t: t, 0),
    "silu+post-residual": (F.silu, 2),
    "gelu+pre-residual": (F.gelu, 1),
    "lrelu": (lambda t: F.leaky_relu(t, 0.2), 0),
}
MUTANTS = ("flush_lo_out", "drop_lo_hi", "drop_hi_lo", "flush_operands")
M, N = 96, 64                                    # pixels, output channels


def test_the_row_choice_is_pinned():
    rows, cands = cr.RANGE_CASES, cr.candidates()
    by_signature = {}
    for r in cands:
        by_signature.setdefault(cr.signature(r), []).append(r)
    assert len(by_signature) == 58
    chosen_by_signature = {}
    for r in rows:
        chosen_by_signature.setdefault(cr.signature(r), []).append(r)
    # every signature has a row, and its cheapest one
    assert set(chosen_by_signature) == set(by_signature)
    for s, rs in by_signature.items():
        assert min(cr.macs(r) for r in rs) == min(cr.macs(r) for r in chosen_by_signature[s]), s
    # every activation a (dtype, family) has in the tables
    fam = lambda r: (r["dtype"], cr.family(r["key"]))
    for key in {fam(r) for r in cands}:
        assert {r["act"] for r in cands if fam(r) == key} == {r["act"] for r in rows if fam(r) == key}, key
    assert {r["act"] for r in rows} == {"none", "relu", "silu", "gelu", "lrelu"}
    assert len(rows) == 68 and len({r["name"] for r in rows}) == 68
    assert all(r["dtype"] in ("f16x2", "f32") for r in rows)
    assert sum(cr.macs(r) for r in rows) < 50e9 and max(cr.macs(r) for r in rows) < 4e9
    # part B: one row per family and the split-K epilogue
    assert [r["family"] for r in cr.FAMILY_CASES] == ["reg3x3.cog1", "reg3x3.cog2", "reg3x3.cog2.pool", "reg3x3_64", "sx", "tile.f32", "ws.f32",
                                                      "wsf.s2", "wsf.s3", "wsq", "wsx.s2", "wsx.s4", "splitk", "sx.next"]
    assert [r["act"] for r in cr.FAMILY_CASES if r["act"] != "relu"] == ["silu"]      # reg3x3.cog2 has no relu row
    by_family = {r["family"]: r for r in cr.FAMILY_CASES}
    assert by_family["splitk"]["S"] > 1 and by_family["sx.next"]["Cnext"] > 0 and by_family["sx.next"]["key"].startswith("sx.")   # k_splitk_reduce's and the follower's epilogue
    assert by_family["reg3x3.cog2.pool"]["pool"] == 1


def test_the_scales_leave_the_draws_alone():
    g, h = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    a = torch.randn(5, generator=g)
    s = cr.draw_scales(g, dict(Cin=64, Cout=96, C2=32))
    assert torch.equal(a, torch.randn(5, generator=h))
    assert s["e"].shape == (64,) and s["e2"].shape == (32,) and s["f"].shape == (96,)
    assert -8 <= int(s["e"].min()) and int(s["e"].max()) <= 4 and -10 <= int(s["f"].min()) and int(s["f"].max()) <= 6
    assert cr.draw_scales(g, dict(Cin=64, Cout=96, C2=0))["e2"] is None
    sat = cr.draw_saturating_scales(torch.Generator().manual_seed(3), dict(Cin=64, Cout=96, C2=0))
    assert (sat["f"][-32:] == 16).all() and int(sat["f"][:-32].max()) <= 6


_CASES = {}


def case(K, epilogue):
    """Seen operands under the scales, the fp64 reference, the fp32 yardstick and the per-element bounds - computed once."""
    if (K, epilogue) not in _CASES:
        act, res_mode = EPILOGUES[epilogue]
        g = torch.Generator().manual_seed(1000 + K)
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * (1.0 / K) ** 0.5
        b, res = torch.randn(N, generator=g) * 0.1, torch.randn(M, N, generator=g)
        s = cr.draw_scales(g, dict(Cin=K, Cout=N, C2=0))
        p2 = lambda e: torch.ldexp(torch.ones(e.shape), e)
        seen = lambda t: sum(cr.split2(t))
        x, w = seen(x * p2(s["e"])), seen(w * p2(s["f"][:, None] - s["e"][None, :]))
        b, res = b * p2(s["f"]), seen(res * p2(s["f"]))

        def epi(v):
            v = v + res.to(v.dtype) if res_mode == 1 else v
            v = act(v)
            return v + res.to(v.dtype) if res_mode == 2 else v

        want = epi(x.double() @ w.double().t() + b.double())
        y32 = epi(x @ w.t() + b)
        A = x.double().abs() @ w.double().abs().t() + b.double().abs() + (res.double().abs() if res_mode else 0.0)
        rho = cr.yardstick(want, y32, A)
        _CASES[(K, epilogue)] = dict(x=x, w=w, b=b, res=res, act=act, res_mode=res_mode, want=want, bounds=cr.bounds(want, A, rho, True))
    return _CASES[(K, epilogue)]


def emulate(c, mutant=None):
    return cr.pair_gemm(c["x"], c["w"], c["b"], c["res"], c["act"], c["res_mode"], mutant)


@pytest.mark.parametrize("epilogue", list(EPILOGUES))
@pytest.mark.parametrize("K", [128, 1152, 2752])
def test_the_gate_passes_the_honest_pair_arithmetic(K, epilogue):
    c = case(K, epilogue)
    ratio = cr.assert_gate(f"K = {K}, {epilogue}", emulate(c), c["want"], *c["bounds"], cr.FACTOR["f16x2"])
    assert ratio > 0.1, "a gate this far from the honest arithmetic sees nothing"


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("epilogue", list(EPILOGUES))
@pytest.mark.parametrize("K", [128, 1152, 2752])
def test_the_gate_rejects_the_mutants(K, epilogue, mutant):
    c = case(K, epilogue)
    got = emulate(c, mutant)
    print(f"K = {K}, {epilogue}, {mutant}: ratio {cr.worst_ratio(got, c['want'], *c['bounds']):.0f}")
    with pytest.raises(AssertionError):
        cr.assert_gate(f"K = {K}, {epilogue}, {mutant}", got, c["want"], *c["bounds"], cr.FACTOR["f16x2"])


@pytest.mark.parametrize("epilogue", list(EPILOGUES))
@pytest.mark.parametrize("K", [128, 1152, 2752])
def test_the_tensor_wide_bound_accepts_the_flushed_lo_mutant(K, epilogue):
    """... which is why the per-element gate exists: the damaged channels are small next to max |y|."""
    c = case(K, epilogue)
    assert cr.tensor_wide_ok(emulate(c, "flush_lo_out"), c["want"])
    assert cr.tensor_wide_ok(emulate(c), c["want"])


def test_the_gate_keeps_nan_elements_out_of_the_yardstick_and_in_the_check():
    c = case(128, "none")
    want = c["want"].clone()
    want[3] = float("nan")
    got = emulate(c)
    got[3] = float("nan")
    cr.assert_gate("NaN row", got, want, *c["bounds"], cr.FACTOR["f16x2"])
    got[5, 7] = float("nan")                     # a NaN where the reference has a number
    with pytest.raises(AssertionError):
        cr.assert_gate("stray NaN", got, want, *c["bounds"], cr.FACTOR["f16x2"])
