"""Segment extraction (connected components + RANSAC), CPU side: the executable contract (tests/seg_contract.py) against the
fixture pinned on the reference (tests/golden/match_segments.json), its subset stream against sklearn's own sampler, and the
`backend` argument of src.matching.generate_matching_result."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import seg_cases  # noqa: E402
import seg_contract  # noqa: E402

from src import matching  # noqa: E402

# Tier A score bound: the reference takes std in fp32 over at most 224 * 224 = 50 176 values; pairwise summation error is about
# log2(n) * 2^-24 ~ 1e-6 relative on values <= 1, times std_ratio <= 2, plus the fp32 rounding of max - std * ratio (6e-8).
TIER_A_SCORE = 4e-6


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "match_segments.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def contract_runs(fixture):
    """(case name, pass index) -> (sorted contract rows, report)"""
    out = {}
    for case in fixture["cases"]:
        m = seg_cases.matrix(case)
        for t, p in enumerate(case["passes"]):
            rows, report = seg_contract.segments(m, p["threshold"], p["std_ratio"])
            out[case["name"], t] = (sorted(rows), report)
    return out


def test_fixture_inputs_reproduce_and_conditions_hold(fixture):
    recipes = seg_cases.by_name()
    assert [c["name"] for c in fixture["cases"]] == list(recipes)
    assert [tuple(p) for p in fixture["passes"]] == [tuple(p) for p in seg_cases.PASSES]
    entries, tiers, knife, seg_ab = 0, {"A": 0, "B": 0, "C": 0}, 0, 0
    for case in fixture["cases"]:
        assert seg_cases.digest(seg_cases.matrix(recipes[case["name"]])) == case["digest"], case["name"]
        assert case["h"] <= seg_cases.MAX_SIDE and case["w"] <= seg_cases.MAX_SIDE
        for p in case["passes"]:
            entries += 1
            tiers[p["tier"]] += 1
            knife += p["margin"] is not None and p["margin"] < fixture["knife_edge"]
            seg_ab += len(p["rows"]) if p["tier"] in "AB" else 0
    assert fixture["knife_edge"] == 1e-9 and fixture["twin_delta"] == 1e-9
    assert entries >= 150 and tiers["C"] <= 0.25 * entries and tiers["A"] >= 40 and seg_ab >= 150 and knife <= 0.02 * entries, \
        (entries, tiers, seg_ab, knife)
    assert fixture["summary"]["tiers"] == tiers and fixture["summary"]["entries"] == entries
    families = {c["family"] for c in fixture["cases"]}
    assert families == {"clean", "thin", "thick", "edge"}
    slopes = {b[3] for c in fixture["cases"] for b in c["bands"]}
    assert {1.0, 0.5, 2.0, 1.25, -1.0} <= slopes


def test_contract_equals_reference_on_tiers_a_and_b(fixture, contract_runs):
    """Tier A (no boundary point in any executed trial) and tier B (the reference gives the same endpoints at 2 +- 1e-9):
    endpoints identical; tier A also agrees in score to fp32 noise."""
    checked = 0
    for case in fixture["cases"]:
        for t, p in enumerate(case["passes"]):
            rows, report = contract_runs[case["name"], t]
            assert (p["tier"] == "A") == (not report["boundary"]), (case["name"], t)
            if p["tier"] == "C":
                continue
            assert [r[:4] for r in rows] == [r[:4] for r in p["rows"]], (case["name"], p["threshold"], p["tier"])
            checked += len(rows)
            if p["tier"] == "A":
                for got, want in zip(rows, p["rows"]):
                    print(f"{case['name']} thr {p['threshold']}: score {got[4]!r} vs reference {want[4]!r}")
                    assert abs(got[4] - want[4]) <= TIER_A_SCORE, (case["name"], p["threshold"], got, want)
    assert checked >= 150


def test_agreement_on_tiers_b_and_c_is_what_the_fixture_recorded(fixture, contract_runs):
    """Where sklearn's own answer may hang on rounding noise the agreement is a recorded fact, not a bound: the contract
    reproduces exactly what the generator saw (endpoints equal or not, score difference, margin)."""
    seen = {"B": [0, 0, 0.0], "C": [0, 0, 0.0]}
    for case in fixture["cases"]:
        for t, p in enumerate(case["passes"]):
            rows, report = contract_runs[case["name"], t]
            margin = None if report["margin"] == float("inf") else report["margin"]
            assert (margin is None) == (p["margin"] is None) and (margin is None or margin == pytest.approx(p["margin"], rel=1e-6, abs=1e-15))
            assert report["group_sizes"] == p["group_sizes"]
            if p["tier"] == "A":
                continue
            same = [r[:4] for r in rows] == [r[:4] for r in p["rows"]]
            assert same == p["endpoints_equal"], (case["name"], p["threshold"])
            seen[p["tier"]][0] += same
            seen[p["tier"]][1] += 1
            if same:
                diff = max([abs(a[4] - b[4]) for a, b in zip(rows, p["rows"])], default=0.0)
                assert diff == pytest.approx(p["score_diff"], abs=1e-12)
                seen[p["tier"]][2] = max(seen[p["tier"]][2], diff)
    for tier, (same, total, diff) in seen.items():
        print(f"tier {tier}: endpoints equal in {same} of {total}, largest score difference {diff:.3e}")
        assert f"{same} of {total}" == fixture["summary"]["endpoints_equal"][tier]


def _sklearn_subsets(n, count):
    from sklearn.utils.random import sample_without_replacement
    rs = np.random.RandomState(seg_contract.SEED)
    return [tuple(int(v) for v in sample_without_replacement(n, 2, random_state=rs)) for _ in range(count)]


def _contract_subsets(n, count):
    draw = seg_contract.subsets(n)
    return [next(draw) for _ in range(count)]


def test_subsets_equal_sklearns_sampler(fixture):
    """Trial t of a group of n points uses what sample_without_replacement(n, 2, random_state=rs) returns on its t-th call."""
    sizes = set(range(4, 401))
    sizes |= {n for c in fixture["cases"] for p in c["passes"] for n in p["group_sizes"]}
    sizes |= {int(v) for v in np.random.RandomState(1).randint(401, 50177, size=60)} | {50176, 50175, 1000, 4096, 65535 // 2}
    for n in sorted(sizes):
        count = 200 if n in (4, 5, 199, 200, 201, 50176) else 12
        assert _contract_subsets(n, count) == _sklearn_subsets(n, count), n


def test_single_diagonal_and_empty_inputs():
    m = np.zeros((40, 50), np.float32)
    for t in range(20):
        m[5 + t, 8 + t] = 0.9
    rows, report = seg_contract.segments(m, 0.35, 0.5)
    assert len(rows) == 1 and rows[0][:4] == [5, 8, 24, 27] and abs(rows[0][4] - 0.9) < 1e-6 and not report["boundary"]
    host = matching.generate_matching_result([["Q1", "R1", m, None]], 0.35, 0.5, backend="host")   # no boundary point: the host path agrees
    assert [int(v) for v in host[0][2:6]] == rows[0][:4] and abs(host[0][6] - rows[0][4]) <= TIER_A_SCORE
    assert seg_contract.segments(np.zeros((8, 8), np.float32), 0.35, 0.5)[0] == []
    assert seg_contract.segments(np.zeros((0, 5), np.float32), 0.35, 0.5)[0] == []
    assert seg_contract.matching_result([], 0.35, 0.5) == []


def _some_maps(fixture, names):
    by = seg_cases.by_name()
    return [[f"Q{i}", f"R{i}", seg_cases.matrix(by[n]), None] for i, n in enumerate(names)]


def test_backend_host_is_the_default_path(fixture):
    names = ["clean_01_60x80", "thin_02_120x90", "thick_00_120x90", "edge_specks_only"]
    maps = _some_maps(fixture, names)
    recorded = {c["name"]: c for c in fixture["cases"]}
    for t, (thr, ratio) in enumerate(seg_cases.PASSES):
        default = matching.generate_matching_result(maps, threshold=thr, std_ratio=ratio)
        host = matching.generate_matching_result(maps, threshold=thr, std_ratio=ratio, backend="host")
        assert [list(map(float, r[2:])) for r in host] == [list(map(float, r[2:])) for r in default] and [r[:2] for r in host] == [r[:2] for r in default]
        for i, n in enumerate(names):         # ... which is the reference's output
            got = sorted([int(r[2]), int(r[3]), int(r[4]), int(r[5])] for r in host if r[0] == f"Q{i}")
            assert got == [r[:4] for r in recorded[n]["passes"][t]["rows"]]


def test_unknown_backend_raises(fixture):
    with pytest.raises(ValueError, match="backend"):
        matching.generate_matching_result(_some_maps(fixture, ["clean_01_60x80"]), 0.35, 0.5, backend="cuda")


def test_backend_hip_needs_a_device_and_neither_scipy_nor_sklearn(fixture, monkeypatch):
    """backend="hip" reaches the device check without importing scipy or sklearn; without a device it raises
    HipPathUnavailable (there is no quiet fall-back to the host path), with one it returns the contract's rows."""
    import torch
    from vsc_hip._lib import HipPathUnavailable
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "sklearn", None)
    maps = _some_maps(fixture, ["clean_01_60x80"])
    if torch.cuda.is_available():
        got = matching.generate_matching_result(maps, 0.35, 0.5, backend="hip")
        assert [r[:6] for r in got] == [r[:6] for r in seg_contract.matching_result(maps, 0.35, 0.5)]
    else:
        with pytest.raises(HipPathUnavailable):
            matching.generate_matching_result(maps, 0.35, 0.5, backend="hip")
        with pytest.raises(HipPathUnavailable):
            matching.generate_matching_results_hip(maps, seg_cases.PASSES)
