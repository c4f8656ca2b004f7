"""CPU: the conv case table (tests/conv_cases.py) against the library's own choice functions.  rtd_debug_conv_choice runs
launch_conv's checks and choose_plain / choose_pair on the host, so none of this needs a GPU: every row of the table still lands on
the instantiation it names, the table covers every instantiation the launchers can name, and the search tool reproduces it.
The same for the view table (tests/conv_view_cases.py) through rtd_debug_conv_choice_views: every row lands on the key, S and grid it
names, the matrix of forms and families is covered (or a cell is listed as unreached and still refused), the tool reproduces it."""
import numpy as np
import pytest
import torch

from telescope_cam_detection_amd import _capi
from tests import conv_cases, conv_view_cases
from tests.conv_cases import CASES, UNREACHED
from tests.conv_view_cases import UNREACHED_VIEWS, VIEW_CASES
from tools import conv_case_search as search

PAIR_TILE_FAMILIES = ("wsf", "wsq", "wsx")


@pytest.fixture(autouse=True)
def options_back_to_default():
    try:
        yield
    finally:
        _capi.debug_option("reset", 0)


@pytest.mark.parametrize("row", CASES, ids=[r["name"] for r in CASES])
def test_row_lands_on_the_kernel_it_names(row):
    try:
        search.set_options(row["opts"])
        c = search.predict(row)
        assert c is not None, _capi.lib().rtd_last_error(None)
        assert (c["key"], c["S"], c["grid"]) == (row["key"], row["S"], row["grid"])
        if "@" in row["name"]:
            group, s = row["name"].split("@S")
            assert row["key"].startswith(group + ".") or row["key"] == group
            assert int(s) == row["S"] and row["S"] in (2, 4)
        else:
            assert row["name"] == row["key"] and row["S"] == 1
        assert search.macs(row) <= 8e9
    finally:
        _capi.debug_option("reset", 0)


def test_table_covers_every_instantiation():
    inst = _capi.conv_instantiations()
    assert len(inst) == len(set(inst)) == 12 + 6 + 16 + 4 + 20 + 7 + 4      # tile, ws, sx, direct 3x3, wsf, wsq, wsx
    one_pass = {r["key"] for r in CASES if r["S"] == 1}
    assert one_pass == set(inst) - set(UNREACHED), (set(inst) - set(UNREACHED)) ^ one_pass
    names = [r["name"] for r in CASES]
    assert len(names) == len(set(names))
    # every (stages, bn) group of the flexible and the fixed pair tiles: two-pass split-K in 2 and in 4 slices
    groups = {k.rsplit(".mt", 1)[0] for k in inst if k.startswith("wsf.")} | {k for k in inst if k.startswith("wsx.")}
    assert len(groups) == 3 + 4
    assert {f"{g}@S{s}" for g in groups for s in (2, 4)} <= set(names)


def test_unreached_is_small_and_still_unreached():
    assert len(UNREACHED) <= 2 and all(isinstance(v, str) and v for v in UNREACHED.values())
    assert not [k for k in UNREACHED if k.split(".")[0] in PAIR_TILE_FAMILIES]
    assert UNREACHED == search.UNREACHED and set(UNREACHED) <= set(_capi.conv_instantiations())
    if UNREACHED:
        try:
            assert not search.search(only_keys=set(UNREACHED))
        finally:
            _capi.debug_option("reset", 0)


def test_every_family_sees_every_residual_mode_and_output_type():
    fam = lambda r: r["key"].split(".")[0]
    seen = {}
    for r in CASES:
        seen.setdefault(fam(r), set()).add((r["res_mode"], r["dtype"], r["out_f32"]))
    for f in ("tile", "ws", "wsf", "wsq", "wsx"):
        assert {m for m, _, _ in seen[f]} == {0, 1, 2}, f
        outs = {(dt, o) for _, dt, o in seen[f]}
        assert outs == ({("bf16", 0), ("bf16", 1), ("f32", 0)} if f in ("tile", "ws") else {("f16x2", 0), ("f16x2", 1)}), (f, outs)
    # the streaming kernel: residual and fp32 rows are template arguments (its keys); both residual modes among the residual variants
    assert {m for m, _, _ in seen["sx"]} == {0, 1, 2} and {o for _, _, o in seen["sx"]} == {0, 1}
    # the direct 3x3 kernels take neither a residual nor fp32 rows
    assert seen["reg3x3"] == {(0, "f16x2", 0)} and seen["reg3x3_64"] == {(0, "f16x2", 0)}


def test_search_tool_reproduces_the_committed_table():
    try:
        text = search.render(search.finish_rows(search.search()))
    finally:
        _capi.debug_option("reset", 0)
    assert text == open(conv_cases.__file__).read()


# ---- the view table (tests/conv_view_cases.py): the families on channel-slice views, pinned through rtd_debug_conv_choice_views ----
@pytest.mark.parametrize("row", VIEW_CASES, ids=[r["name"] for r in VIEW_CASES])
def test_view_row_lands_on_the_kernel_it_names(row):
    form, cell = row["name"].split(":")[0], row["name"]
    try:
        search.set_options(row["opts"])
        c = search.predict_view(row)
        assert c is not None, _capi.lib().rtd_last_error(None)
        assert (c["key"], c["S"], c["grid"]) == (row["key"], row["S"], row["grid"])
        assert row["form"] == form and cell in search.cells_of(row, c)
        # on such a view the choice is the dense one (the GPU test runs both launches and compares their bits)
        d = search.predict(dict(row, Cnext=0, avg=0, pool=0))
        assert d is not None and (d["key"], d["S"], d["grid"]) == (c["key"], c["S"], c["grid"])
    finally:
        _capi.debug_option("reset", 0)
    # the geometry of a view: [c0 | C | c1] with c0, c1 > 0 in whole 32-channel groups (the small-channel loader's input: 8-channel chunks)
    assert row["B"] >= 2 and search.macs(row) <= search.MAX_MACS
    assert set(row["views"]) == {"x", "y"} | ({"res"} if row["res_mode"] else set()) | ({"x2"} if row["C2"] else set())
    for t, (c0, c1) in row["views"].items():
        unit = 8 if t == "x" and row["Cin"] % 32 else 32
        assert c0 > 0 and c1 > 0 and c0 % unit == 0 and c1 % unit == 0, (t, c0, c1)
    lds = [search.view_ld(row, t) for t in row["views"]]
    assert len(set(lds)) == len(lds), lds                        # pairwise different pixel strides
    oh, ow = search.out_hw(row)
    if form in ("V", "R"):
        assert row["stride"] == 1 and not row["C2"] and bool(row["res_mode"]) == (form == "R")
    if form == "S2":
        assert (row["k"], row["stride"], row["pad"]) == (3, 2, 1) and row["H"] % 2 == row["W"] % 2 == (1 if cell.endswith(":odd") else 0)
        # odd extents: the last window's bottom / right taps are padding; even: they are the last row / column
        assert (2 * (oh - 1) + 1 == row["H"]) == cell.endswith(":odd") and (2 * (ow - 1) + 1 == row["W"]) == cell.endswith(":odd")
    if form == "K":
        assert row["S"] == int(cell.split("@S")[1]) and row["S"] in (2, 4) and row["res_mode"] in (1, 2) and row["act"] == "silu" and row["k"] == 3
    if form in ("D", "U"):
        assert row["C2"] > 0 and search.view_ld(row, "x2") > row["C2"] and row["x_up2"] == (form == "U")
    if form == "U":
        assert row["k"] == 1 and row["H"] % 2 == 0 and row["W"] % 2 == 0


def test_view_table_covers_the_matrix():
    cells = search.view_cells()
    assert len(cells) == len(set(cells)) == 12 + 8 + 2 * 7 + 2 * 2 + 4 + 2        # V, R, S2 (odd, even), K (S = 2, 4), D, U
    assert {"V:tile.bf16.smallc0", "V:tile.f32.smallc1", "V:reg3x3_64", "R:sx", "S2:wsq:odd", "S2:ws.f32:even", "K:wsf@S2", "K:wsx@S4", "D:sx", "D:pair", "U:ws",
            "U:pair"} <= set(cells)
    names = [r["name"] for r in VIEW_CASES]
    assert len(names) == len(set(names)) and set(names) == set(cells) - set(UNREACHED_VIEWS), set(names) ^ set(cells)
    # a missing cell is a condition, not a convenience: it names the refusing rule and is still refused
    assert UNREACHED_VIEWS == search.UNREACHED_VIEWS and set(UNREACHED_VIEWS) <= set(cells)
    assert all(isinstance(v, str) and len(v) > 20 for v in UNREACHED_VIEWS.values())
    if UNREACHED_VIEWS:
        try:
            assert not search.search_views(only_cells=set(UNREACHED_VIEWS))
        finally:
            _capi.debug_option("reset", 0)
    by_form = lambda f: [r for r in VIEW_CASES if r["form"] == f]
    assert {r["key"] for r in by_form("D") if r["key"].startswith("sx.")} == {"sx.x2.x2_2.res0.next0.f32_0.avg0"}
    # residual modes: both among the R rows, and both per family and per slice count among the K rows
    assert {r["res_mode"] for r in by_form("R")} == {1, 2}
    for pick in (lambda r: r["key"].split(".")[0], lambda r: r["S"]):
        seen = {}
        for r in by_form("K"):
            seen.setdefault(pick(r), set()).add(r["res_mode"])
        assert len(seen) == 2 and all(v == {1, 2} for v in seen.values()), seen
    # fp32 rows out and every activation somewhere on views
    assert {r["out_f32"] for r in VIEW_CASES if r["dtype"] != "f32"} == {0, 1} and {r["act"] for r in VIEW_CASES} == {"none", "relu", "silu", "gelu"}


def test_search_tool_reproduces_the_committed_view_table():
    try:
        text = search.render_views(search.finish_view_rows(search.search_views()))
    finally:
        _capi.debug_option("reset", 0)
    assert text == open(conv_view_cases.__file__).read()


def test_view_choice_refuses_what_the_launchers_refuse():
    """rtd_debug_conv_choice_views runs launch_conv's own checks on the strides it is given."""
    L = _capi.lib()
    assert _capi.conv_choice_views(_capi.DT_F16X2, 2, 16, 16, 64, 64, ldx=128, ldy=160)["key"] == _capi.conv_choice(_capi.DT_F16X2, 2, 16, 16, 64, 64)["key"]
    assert _capi.conv_choice_views(_capi.DT_F16X2, 2, 16, 16, 64, 64, ldx=72, ldy=160) is None            # pair slices: whole 32-channel groups
    assert b"pair kernels" in L.rtd_last_error(None)
    assert _capi.conv_choice_views(_capi.DT_F16X2, 2, 16, 16, 64, 64, ldx=32, ldy=160) is None            # ldx < Cin
    assert b"pixel strides" in L.rtd_last_error(None)
    assert _capi.conv_choice_views(_capi.DT_BF16, 2, 16, 16, 64, 64, ldx=68, ldy=96) is None              # bf16: 16-byte chunks
    assert b"16-byte chunk" in L.rtd_last_error(None)
    assert _capi.conv_choice_views(_capi.DT_F16X2, 2, 16, 16, 64, 64, ldx=96, ldy=96, x_up2=1) is None    # x_up2 without a second input


def test_refusals_are_the_launchers_own():
    """A launch launch_conv refuses is refused by the prediction with the same message, and predicts nothing."""
    L = _capi.lib()
    try:
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 16, 16, 48, 64) is None                       # Cin % 32
        assert b"pair kernels" in L.rtd_last_error(None)
        assert _capi.conv_choice(_capi.DT_BF16, 1, 16, 16, 64, 64, Cnext=64) is None              # follower on bf16 operands
        assert b"F16X2 operands only" in L.rtd_last_error(None)
        _capi.debug_option("split_sx", 0)
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 80, 80, 64, 256, Cnext=64) is None            # follower without the streaming kernel
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 80, 80, 128, 256, res_mode=1, avg=1) is None  # average without it
        _capi.debug_option("reset", 0)
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 80, 80, 128, 256, res_mode=1, avg=1)["key"] == "sx.x4.x2_0.res1.next0.f32_0.avg1"
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 81, 80, 128, 256, res_mode=1, avg=1) is None  # odd H
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 58, 98, 32, 64, 3, 1, 1, pool=1)["key"] == "reg3x3.cog2.pool"
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 57, 98, 32, 64, 3, 1, 1, pool=1) is None      # odd H
        assert _capi.conv_choice(_capi.DT_F16X2, 1, 56, 96, 32, 64, 3, 1, 1, pool=1) is None      # 21 tiles
    finally:
        _capi.debug_option("reset", 0)


def test_pair_storage_helper_matches_the_host_mirror():
    """tests/test_gpu_conv_instances.py rounds its operands to hi + lo with torch (threads); same words as _capi.to_split."""
    from tests.test_gpu_conv_instances import pair_words, pair_values
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 5, 96, generator=g) * torch.tensor([1e-6, 1.0, 3e4]).view(3, 1, 1)
    x[0, 0, 0], x[1, 2, 3] = 1e9, -1e9                                       # saturate
    words = pair_words(x)
    np.testing.assert_array_equal(words.numpy().view(np.uint16), _capi.to_split(x.numpy()))
    np.testing.assert_array_equal(pair_values(words).numpy(), _capi.from_split(words.numpy().view(np.uint16)))
