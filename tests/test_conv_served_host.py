"""CPU: the served-launch table (tests/conv_served_cases.py) against the library's own choice functions and against the census of
tools/served_conv_census.py.  Every row still lands on the key, S and grid it names under the default options; the tool reproduces the
committed file; every launch signature the served networks make is in exactly one of SERVED_CASES, COVERED_ELSEWHERE and
UNREACHED_SERVED; what is listed as covered or unreached still is.  A failure here after a change to choose_pair, choose_plain or a
plan builder means: run tools/served_conv_census.py and commit the table it writes."""
import pytest

from telescope_cam_detection_amd import _capi
from tests import conv_served_cases
from tests.conv_served_cases import COVERED_ELSEWHERE, EDGES_ABOVE_CAP, SERVED_CASES, UNREACHED_SERVED
from tools import conv_case_search as search
from tools import served_conv_census as census


@pytest.fixture(autouse=True)
def options_back_to_default():
    try:
        yield
    finally:
        _capi.debug_option("reset", 0)


@pytest.fixture(scope="module")
def seen():
    return census.census()


row_signature = census.row_signature


@pytest.mark.parametrize("row", SERVED_CASES, ids=[r["name"] for r in SERVED_CASES])
def test_row_lands_on_the_kernel_it_names(row):
    assert row["opts"] == {}                                     # the served networks run under the default options
    search.set_options(row["opts"])
    c = census.choice(row)
    assert c is not None, _capi.lib().rtd_last_error(None)
    assert (c["key"], c["S"], c["grid"]) == (row["key"], row["S"], row["grid"])
    assert row["name"].startswith(census.signature_name(row_signature(row)))
    assert search.macs(row) <= search.MAX_MACS
    assert not (row["C2"] or row["x_up2"] or row["Cnext"] or row["avg"] or row["pool"])
    assert 1 <= len(row["served"]) <= 3
    if "views" in row:                                           # whole 32-channel groups around the slice, as Tensor::slice_c of pair tensors needs
        assert set(row["views"]) == {"x", "y"} | ({"res"} if row["res_mode"] else set())
        assert all(c0 % 32 == 0 and c1 % 32 == 0 for c0, c1 in row["views"].values()) and any(v != (0, 0) for v in row["views"].values())
    if "edge" in row:
        assert set(row["edge"]) <= census.edges_of(row) and row["edge"]


def test_tool_reproduces_the_committed_table(seen):
    text = census.render(*census.build_tables(seen))
    assert text == open(conv_served_cases.__file__).read(), "run tools/served_conv_census.py: the served table is stale"


def test_every_served_signature_is_in_exactly_one_set(seen):
    rows = [row_signature(r) for r in SERVED_CASES if "edge" not in r]
    assert len(rows) == len(set(rows))
    names = [r["name"] for r in SERVED_CASES]
    assert len(names) == len(set(names))
    sets = (set(rows), set(COVERED_ELSEWHERE), set(UNREACHED_SERVED))
    assert sets[0] | sets[1] | sets[2] == set(seen), (sets[0] | sets[1] | sets[2]) ^ set(seen)
    assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])
    # an edge row is one more launch of a signature that already has its place
    assert {row_signature(r) for r in SERVED_CASES if "edge" in r} <= sets[0] | sets[1]
    # every edge width a signature is served with: a row that has it (its own, an edge row, the covering row), or listed as above the cap
    have = census.existing_signatures()
    for sig, launches in seen.items():
        if sig in UNREACHED_SERVED:
            continue
        got = set().union(*[census.edges_of(r) for r in SERVED_CASES if row_signature(r) == sig], census.edges_of(have[sig]) if sig in have else set())
        for _, f in launches:
            for e in census.edges_of(f) - got:
                assert f"{census.signature_name(sig)}/{f['Cin']}to{f['Cout']}" in EDGES_ABOVE_CAP, (sig, e)


def test_covered_elsewhere_names_a_row_with_that_signature():
    from tests.conv_cases import CASES
    from tests.conv_view_cases import VIEW_CASES
    by_name = {r["name"]: r for r in list(CASES) + list(VIEW_CASES)}
    for sig, name in COVERED_ELSEWHERE.items():
        r = by_name[name]
        assert (r["dtype"], r["key"], r["S"], r["k"], r["stride"], r["res_mode"], int(r["out_f32"] and r["dtype"] != "f32"), r["act"]) == sig
        assert not (r["C2"] or r["x_up2"] or r.get("Cnext") or r.get("avg") or r.get("pool"))


def test_unreached_is_small_and_still_unreached(seen):
    """At most 6 signatures, none of them a two-pass split-K launch or the classifier's head; each is still not found below the cap.
    (Two are the classifier's `proj` at n = 14: 1024 -> 1024 needs 7681 rows for wsq.8x8 and 8065 for ws.f32.s2.bn128, 0.7 % and 5.7 %
    above MAX_MACS.  proj has a row on every other key it is served on.)"""
    assert len(UNREACHED_SERVED) <= census.MAX_UNREACHED
    for sig, (why, macs) in UNREACHED_SERVED.items():
        assert sig in seen and isinstance(why, str) and len(why) > 20
        assert sig[2] == 1, "a split-K signature may not be unreached"
        assert not sig[6], "the head / pred signatures (fp32 rows out) may not be unreached"
        assert macs is None or macs > search.MAX_MACS
        for f, _ in census.variants_of(seen[sig]):
            row, over = census.shrink(sig, f)
            assert row is None and (over is None or over > search.MAX_MACS), (sig, row)
    for name, macs in EDGES_ABOVE_CAP.items():
        assert macs is None or macs > search.MAX_MACS, name


def test_plan_convs_need_a_run_first():
    """rtd_debug_*_plan_convs: bound, and a null handle is refused (the lists themselves: tests/test_gpu_conv_served.py)"""
    L = _capi.lib()
    for prefix in ("yolox", "eva", "esrgan"):
        assert getattr(L, f"rtd_debug_{prefix}_plan_convs")(None, None, 0, None) != _capi.RTD_OK
