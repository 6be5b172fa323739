"""The executable contract of the device view decisions (tests/view_decide_contract.py) on the CPU: its boxes equal the host path
(src/image_preprocess.py: decide_views) on every case and the fixture on the 21 recipes, and every sum, mean, quantile and median
it writes out equals numpy's own value bit for bit -- the trace of the whole-frame borders call on every case, and the building
blocks on random region slices, where numpy takes the same orders as inside the recursion.  Checked with numpy 2.2.6."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import view_decide_cases as cases  # noqa: E402
import view_decide_contract as C  # noqa: E402
from src import image_preprocess as ip  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "view_preprocess.json")


def numpy_trace(var, count, m):
    """the eight trace values as the host path computes them"""
    avg = np.asarray(count).astype(np.float64) / m
    q, mean = np.quantile(avg, 0.95), avg.mean()
    threshold = min(max(q, 0.2), mean + 0.35)
    edges = (avg > threshold).astype(np.float32)
    h, w = var.shape
    return np.array([q, mean, threshold, edges.mean(), var.mean(1)[h // 2], var.mean(0)[w // 2], edges.mean(1)[h // 2],
                     edges.mean(0)[w // 2]], np.float64)


@pytest.mark.parametrize("name", cases.names())
def test_contract_equals_the_host_path(name):
    case = cases.get(name)
    boxes, status, trace = cases.expected(name)
    changed, want = ip.decide_views(case["var"], case["count"], case["m"], case["n"])
    if name in cases.ENGINEERED:
        assert status == 1 and boxes == [] and len(want) > case["max_views"]
    else:
        assert status == 0, "a case that needs more than 64 views or pending regions: pick another seed"
        assert boxes == [tuple(int(v) for v in b) for b in want]
        h, w = case["var"].shape
        assert changed == (boxes != [(0, h, 0, w)])
    if case["n"] < C.MIN_FRAMES:
        assert (trace.view(np.uint8) == 0xFF).all()
    else:
        assert np.array_equal(C.bits(trace), C.bits(numpy_trace(case["var"], case["count"], case["m"]))), (trace, numpy_trace(case["var"], case["count"], case["m"]))


def test_recipes_equal_the_fixture():
    with open(FIXTURE) as f:
        fixture = {c["name"]: c for c in json.load(f)["cases"]}
    assert sorted(fixture) == sorted(cases.RECIPES) and len(cases.RECIPES) == 21
    for name in cases.RECIPES:
        boxes, status, _ = cases.expected("recipe_" + name)
        assert status == 0 and [list(b) for b in boxes] == fixture[name]["boxes"], name
        h, w = cases.get("recipe_" + name)["var"].shape
        assert (boxes != [(0, h, 0, w)]) == fixture[name]["changed"], name


def test_cases_cover_what_they_claim():
    shapes = {n: cases.get(n)["var"].shape for n in cases.names()}
    assert {shapes[f"width_{w}"][1] for w in cases.WIDTHS} == set(cases.WIDTHS)
    assert [shapes[n][0] * shapes[n][1] for n in ("pixels_8192", "pixels_8193", "pixels_3x8192_5")] == [8192, 8193, 3 * 8192 + 5]
    assert shapes["letterbox_720p"] == (720, 1280)
    assert {cases.get(f"samples_{m}")["m"] for m in (1, 7, 20)} == {1, 7, 20}
    assert cases.get("frames_4")["n"] == 4 and cases.get("frames_5")["n"] == 5
    assert cases.expected("frames_4")[0] == [(0, 150, 0, 190)] and cases.expected("frames_5")[0] == [(19, 129, 0, 190)]
    assert len(cases.expected("grid_2x2")[0]) == 4 and len(cases.expected("stack3")[0]) == 3
    assert cases.expected("letterbox_720p")[0] == [(91, 629, 0, 1280)]
    assert all(max(shapes[n]) <= cases.EMULATED_MAX or n.startswith("pixels_") for n in cases.names(large=False))
    multi = [n for n in cases.names() if len(cases.expected(n)[0]) > 1]
    assert len(multi) >= 12, multi


def test_building_blocks_equal_numpy_on_region_slices():
    rng = np.random.default_rng(5)
    var = rng.uniform(0.0, 3000.0, (300, 411))
    count = rng.integers(0, 21, (300, 411)).astype(np.uint16)
    avg = count.astype(np.float64) / 20
    regions = [(0, 300, 0, 411), (0, 300, 3, 411), (7, 8, 0, 411), (0, 300, 5, 6), (10, 30, 0, 410), (1, 299, 1, 410)]
    for _ in range(40):
        y0, x0 = int(rng.integers(0, 280)), int(rng.integers(0, 390))
        regions.append((y0, int(rng.integers(y0 + 1, 301)), x0, int(rng.integers(x0 + 1, 412))))
    for y0, y1, x0, x1 in regions:
        v, a, c = var[y0:y1, x0:x1], avg[y0:y1, x0:x1], count[y0:y1, x0:x1]
        assert np.array_equal(C.bits(C.row_means(v)), C.bits(v.mean(1)))
        assert np.array_equal(C.bits(C.col_means(v)), C.bits(v.mean(0)))
        assert C.bits(C.flat_sum(a) / np.float64(a.size)) == C.bits(a.mean())
        assert C.bits(C.flat_sum(v)) == C.bits(v.sum())
        assert C.bits(C.quantile95(c, 20)) == C.bits(np.quantile(a, 0.95))
        for extra in (0.35, 0.3):
            q, mean, threshold, edges = C.edge_maps(c, 20, extra)
            want = min(max(np.quantile(a, 0.95), 0.2), a.mean() + extra)
            assert C.bits(threshold) == C.bits(want)
            e32 = (a > want).astype(np.float32)
            e_all, e_rows, e_cols = C.edge_means(edges)
            assert e_all.dtype == np.float32 and e_all == e32.mean()
            assert np.array_equal(e_rows, e32.mean(1)) and np.array_equal(e_cols, e32.mean(0))
            for p in (e_rows, e_cols):
                for lo, hi in ((0, len(p)), (1, len(p) - 1), (len(p) // 3, len(p) // 3 + 9), (2, 2)):
                    s = p[lo:hi]
                    got, ref = C.mean1d(s), s.mean() if s.size else np.float32(np.nan)
                    assert got.dtype == np.float32 and (got == ref or (np.isnan(got) and np.isnan(ref)))
                assert (np.float32(0.125) + C.mean1d(p)) == (0.125 + p.mean()) and (0.125 + p.mean()).dtype == np.float32
        for p in (v.mean(1), v.mean(0)):
            for lo, hi in ((0, len(p)), (1, len(p)), (0, len(p) - 1), (len(p) // 2, len(p) // 2 + 1)):
                s = p[lo:hi]
                if s.size:
                    assert C.bits(C.median(s)) == C.bits(np.median(s)) and C.bits(C.mean1d(s)) == C.bits(s.mean())
    assert np.isnan(C.median(var[0, 0:0])) and np.isnan(C.mean1d(var[0, 0:0]))


def test_rounding_of_the_margin_is_half_to_even():
    for d in range(5, 4096):
        assert int(np.rint(np.float64(d) * np.float64(0.3))) == round(d * 0.3)


def test_transposed_maps_give_other_boxes():
    """rows and columns are not interchangeable: a kernel that swaps the axes fails the cases"""
    case = cases.get("stack3")
    boxes, _ = C.decide(case["var"].T.copy(), case["count"].T.copy(), case["m"], case["n"])
    assert boxes == [(x0, x1, y0, y1) for y0, y1, x0, x1 in cases.expected("stack3")[0]] and boxes != cases.expected("stack3")[0]


def test_flag_defaults_are_host():
    assert inspect.signature(ip.detect_views).parameters["decisions"].default == "host"
    assert inspect.signature(ip.HipViews.__init__).parameters["decisions"].default == "host"
    assert ip.VIEW_DECISIONS == ("host", "hip")
    import extract_query_feats
    ap = extract_query_feats.build_parser()
    action = next(a for a in ap._actions if a.dest == "view_decisions")
    assert action.default == "host" and tuple(action.choices) == ("host", "hip")
    with pytest.raises(ValueError, match="decisions"):
        ip.detect_views(np.zeros((6, 4, 4, 3), np.uint8), decisions="device")
    script = open(os.path.join(os.path.dirname(HERE), "vsc22-submission_amd", "infer_query.sh")).read()
    assert '--view_decisions "${VIEW_DECISIONS:-host}"' in script
