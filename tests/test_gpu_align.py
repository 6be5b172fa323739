"""DP and HV temporal alignment on the HIP path (vsc_align_dp_f32 / vsc_align_hv_f32, vsc_hip.alignment, the HipVCSL* localization
classes and `sscd_baseline --alignment hip --alignment_model DP`) against the reference's own `dp` and `hv`, recorded in
tests/golden/align_dp_hv.json, and against the executable contract (tests/align_contract.py) for MaxSim."""
import json
import os

import numpy as np
import pytest

import align_cases
import align_contract
from tools import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "align_dp_hv.json")
DP_FIELDS = ("discontinue", "min_sim", "ave_sim", "min_length", "diagonal_thres")
HV_FIELDS = ("min_sim", "iou_thresh", "max_peaks")
DP_SLOTS = 100


@pytest.fixture(scope="module")
def dev():
    import torch

    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def mats(fixture):
    out = [align_cases.matrix(c) for c in fixture["cases"]]
    for c, m in zip(fixture["cases"], out):
        assert align_cases.digest(m) == c["digest"], c["name"]
    return out


@pytest.fixture(scope="module")
def expected(fixture, mats):
    """{name: (boxes, maxsim)} of the contract, computed once; its boxes are the fixture's (tests/test_align_cpu.py)."""
    out = {}
    for c, m in zip(fixture["cases"], mats):
        fn = align_contract.dp_contract if c["model"] == "DP" else align_contract.hv_contract
        boxes, maxsim = fn(m, c["bias"], **c["params"])
        assert boxes == c["boxes"], c["name"]
        out[c["name"]] = (boxes, np.array(maxsim, dtype=np.float32))
    return out


def _layout(items, dev):
    import torch
    sizes = [m.size for m in items]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    table = np.array([[o, m.shape[0], m.shape[1]] for o, m in zip(offs, items)], dtype=np.int64).reshape(-1, 3)
    data = np.concatenate([m.reshape(-1) for m in items]) if items else np.zeros(0, np.float32)
    return torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(dev), table


def _call(model, params, flat, table, bias, slots=DP_SLOTS, handle=None):
    from vsc_hip import ops
    if model == "DP":
        return ops.dp_align(flat, table, bias, *(params[k] for k in DP_FIELDS), max_boxes=slots, handle=handle)
    return ops.hv_align(flat, table, bias, *(params[k] for k in HV_FIELDS), handle=handle)


def _groups(cases, mats):
    groups = {}
    for c, m in zip(cases, mats):
        fields = DP_FIELDS if c["model"] == "DP" else HV_FIELDS
        groups.setdefault((c["model"], c["bias"]) + tuple(c["params"][k] for k in fields), []).append((c, m))
    return groups


def _run(cases, mats, dev, slots=DP_SLOTS, handle=None):
    """All `cases` in one call per (model, bias, parameter set) -> {name: (boxes found, stored boxes, stored maxsim, raw bytes)}."""
    out = {}
    for items in _groups(cases, mats).values():
        c0 = items[0][0]
        flat, table = _layout([m for _, m in items], dev)
        boxes, counts, maxsim = (t.cpu().numpy() for t in _call(c0["model"], c0["params"], flat, table, c0["bias"], slots, handle))
        for i, (c, _) in enumerate(items):
            n = min(int(counts[i]), boxes.shape[1])
            assert (boxes[i, n:] == 0).all() and (maxsim[i, n:] == 0).all(), c["name"]       # unused slots
            out[c["name"]] = (int(counts[i]), boxes[i, :n].tolist(), maxsim[i, :n].copy(), boxes[i].tobytes() + maxsim[i].tobytes())
    return out


@pytest.fixture(scope="module")
def batched(fixture, mats, dev):
    return _run(fixture["cases"], mats, dev)


def test_fixture_boxes_identical(fixture, batched):
    bad = [(c["name"], batched[c["name"]][1][:3], c["boxes"][:3]) for c in fixture["cases"]
           if batched[c["name"]][1] != c["boxes"] or batched[c["name"]][0] != len(c["boxes"])]
    assert not bad, f"{len(bad)} of {len(fixture['cases'])} cases differ from the reference: {bad[:3]}"
    assert sum(len(c["boxes"]) for c in fixture["cases"]) > 700


def test_maxsim_bits_are_the_contracts(fixture, batched, expected):
    n = empty = 0
    for c in fixture["cases"]:
        got, want = batched[c["name"]][2], expected[c["name"]][1]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c["name"], got[:4], want[:4])
        n += len(want)
        empty += int(np.isneginf(want).sum())
    assert n > 700 and empty > 20           # one-cell diagonals of HV: -inf over the empty half-open extent


def test_counts_above_max_boxes_are_reported(fixture, mats, dev):
    picks = [(c, m) for c, m in zip(fixture["cases"], mats) if c["model"] == "DP" and len(c["boxes"]) > 2]
    assert len(picks) >= 4
    got = _run([c for c, _ in picks], [m for _, m in picks], dev, slots=2)
    full = _run([c for c, _ in picks], [m for _, m in picks], dev)
    for c, _ in picks:
        count, boxes, maxsim, _ = got[c["name"]]
        assert count == len(c["boxes"]) and boxes == c["boxes"][:2], c["name"]
        assert np.array_equal(maxsim.view(np.uint32), full[c["name"]][2][:2].view(np.uint32)), c["name"]
    from vsc_hip.alignment import DpAlignment
    c, m = picks[0]
    with pytest.raises(RuntimeError, match="max_boxes"):
        DpAlignment(max_boxes=2, **c["params"]).forward_sim([("k", m + c["bias"])])
    assert DpAlignment(**c["params"]).forward_sim([("k", m + c["bias"])]) == [("k", c["boxes"])]


def _small(fixture, mats, model):
    return [(c, m) for c, m in zip(fixture["cases"], mats) if c["model"] == model and c["q"] * c["r"] <= 20000]


def test_same_call_twice_same_bytes(fixture, mats, batched, dev):
    items = _small(fixture, mats, "DP")[::3] + _small(fixture, mats, "HV")[::5]
    again = _run([c for c, _ in items], [m for _, m in items], dev)
    for c, _ in items:
        assert again[c["name"]][3] == batched[c["name"]][3], c["name"]


def _scratch_need(model, q, r):
    """Scratch bytes of one pair, as vsc_hip.h states them (rounded up to 16)."""
    need = 6 * q * r + 16 * q + 8 * r if model == "DP" else 5 * (q + r - 1)
    return (need + 15) // 16 * 16


def test_capped_scratch_splits_the_launch_same_bytes(fixture, mats, batched, dev):
    from vsc_hip import ops
    for model in ("DP", "HV"):
        group = max(_groups(*zip(*_small(fixture, mats, model))).values(), key=len)
        needs = [_scratch_need(model, c["q"], c["r"]) for c, _ in group]
        cap = max(max(needs), sum(needs) // 4)
        want, used, most = 1, 0, 0              # a launch takes pairs while they fit the cap, and at least one
        for need in needs:
            if used and used + need > cap:
                want, used = want + 1, 0
            used += need
            most = max(most, used)
        assert want >= 3, (model, needs, cap)
        with ops.AlignHandle() as h:
            assert h.scratch(cap) == (0, 0)
            got = _run([c for c, _ in group], [m for _, m in group], dev, handle=h)
            assert h.scratch() == (want, most), model
        for c, _ in group:
            assert got[c["name"]][3] == batched[c["name"]][3], c["name"]


def test_seventy_mixed_pairs_in_one_call(fixture, mats, expected, dev):
    for model in ("DP", "HV"):
        group = max(_groups(*zip(*_small(fixture, mats, model))).values(), key=len)
        c0 = group[0][0]
        items, want = [], []
        for i in range(70):
            if i % 9 == 4:              # empty-sided pairs among them
                items.append(np.zeros([(0, 5), (6, 0), (0, 0)][i % 3], np.float32))
                want.append(([], np.zeros(0, np.float32)))
            else:
                c, m = group[(i * 7) % len(group)]
                items.append(m)
                want.append(expected[c["name"]])
        flat, table = _layout(items, dev)
        boxes, counts, maxsim = (t.cpu().numpy() for t in _call(model, c0["params"], flat, table, c0["bias"]))
        for i, (wb, wm) in enumerate(want):
            assert int(counts[i]) == len(wb) and boxes[i, :len(wb)].tolist() == wb, (model, i)
            assert np.array_equal(maxsim[i, :len(wb)].view(np.uint32), wm.view(np.uint32)), (model, i)


def test_handle_on_a_side_stream(fixture, mats, batched, dev):
    import torch

    from vsc_hip import ops
    side = torch.cuda.Stream(device=dev)
    for model in ("DP", "HV"):
        group = max(_groups(*zip(*_small(fixture, mats, model))).values(), key=len)[:12]
        with torch.cuda.stream(side):
            with ops.AlignHandle() as h:          # bound to the side stream, which is current here
                got = _run([c for c, _ in group], [m for _, m in group], dev, handle=h)
        side.synchronize()
        for c, _ in group:
            assert got[c["name"]][3] == batched[c["name"]][3], c["name"]


def _planted_videos(seed=5, dim=64):
    """Queries that copy segments of some references (small noise), plus unrelated videos."""
    from vsc.index import VideoFeature
    rs = np.random.RandomState(seed)
    refs = [VideoFeature(f"R{i:06d}", np.arange(60.0), synth.descriptor_bank(300 + i, 60, dim)) for i in range(8)]
    queries, planted = [], []
    for i in range(6):
        f = synth.descriptor_bank(600 + i, 40, dim)
        if i < 4:
            r, q0, r0, ln = 1 + i, 3 + i, 10 + 2 * i, 20 + i
            f[q0:q0 + ln] = refs[r].feature[r0:r0 + ln] + 0.02 * rs.randn(ln, dim).astype(np.float32)
            f[q0:q0 + ln] /= np.linalg.norm(f[q0:q0 + ln], axis=1, keepdims=True)
            planted.append((f"Q{i:06d}", refs[r].video_id))
        queries.append(VideoFeature(f"Q{i:06d}", np.arange(40.0), f))
    return queries, refs, planted


def _candidates(queries, refs):
    from vsc.metrics import CandidatePair
    return [CandidatePair(q.video_id, r.video_id, float(0.9 - 0.01 * j)) for j, (q, r) in
            enumerate((q, r) for q in queries for r in refs[:6])]


@pytest.mark.parametrize("model_type,options", [("DP", dict(min_length=4, min_sim=1.0, ave_sim=1.3)), ("DP", dict()),
                                                ("HV", dict(max_peaks=3, min_sim=0.7)), ("HV", dict(iou_thresh=0.3, max_peaks=2))])
def test_vcsl_interface_equals_device_classes(dev, model_type, options):
    from vsc.baseline.localization import (HipVCSLLocalizationCandidateScore, HipVCSLLocalizationMaxSim,
                                           VCSLLocalizationCandidateScore, VCSLLocalizationMaxSim)
    queries, refs, planted = _planted_videos()
    cands = _candidates(queries, refs)
    model = align_contract.ContractModel(model_type, **options)
    want = VCSLLocalizationMaxSim(queries, refs, model_type, similarity_bias=0.5, model=model).localize_all(cands)
    got = HipVCSLLocalizationMaxSim(queries, refs, model_type, similarity_bias=0.5, **options).localize_all(cands)
    assert got == want and len(got) >= len(planted)
    assert [type(m.score) for m in got] == [type(m.score) for m in want]
    assert {(q, r) for q, r in planted} <= {(m.query_id, m.ref_id) for m in got}
    want = VCSLLocalizationCandidateScore(queries, refs, model_type, model=model).localize_all(cands)
    got = HipVCSLLocalizationCandidateScore(queries, refs, model_type, **options).localize_all(cands)
    assert got == want
    assert HipVCSLLocalizationMaxSim(queries, refs, model_type).localize_all([]) == []


def test_maxsim_on_an_empty_extent_raises_as_the_reference(dev):
    from vsc.baseline.localization import HipVCSLLocalizationMaxSim, VCSLLocalizationMaxSim
    queries, refs, _ = _planted_videos()
    cands = _candidates(queries, refs)[:3]
    with pytest.raises(ValueError):          # numpy: the maximum of an empty slice
        VCSLLocalizationMaxSim(queries, refs, "HV", similarity_bias=0.5, model=align_contract.ContractModel("HV")).localize_all(cands)
    with pytest.raises(ValueError, match=f"{cands[0].query_id}-{cands[0].ref_id}"):
        HipVCSLLocalizationMaxSim(queries, refs, "HV", similarity_bias=0.5).localize_all(cands)


def test_tn_model_type_is_the_tn_classes(dev):
    from vsc.baseline.localization import HipTNLocalizationMaxSim, HipVCSLLocalizationMaxSim
    queries, refs, _ = _planted_videos()
    cands = _candidates(queries, refs)
    want = HipTNLocalizationMaxSim(queries, refs, similarity_bias=0.5, tn_max_step=5, min_length=4).localize_all(cands)
    got = HipVCSLLocalizationMaxSim(queries, refs, "TN", similarity_bias=0.5, tn_max_step=5, min_length=4).localize_all(cands)
    assert got == want and got


def test_entry_point_writes_matches_csv_with_dp(dev, tmp_path):
    import vsc.baseline.sscd_baseline as entry
    from vsc.metrics import Dataset, Match
    from vsc.storage import load_features, store_features
    queries, refs, planted = _planted_videos(seed=7)
    store_features(tmp_path / "q.npz", queries)
    store_features(tmp_path / "r.npz", refs)
    args = entry.build_parser().parse_args(["--query_features", str(tmp_path / "q.npz"), "--ref_features", str(tmp_path / "r.npz"),
                                            "--output_path", str(tmp_path / "out"), "--overwrite", "--alignment", "hip",
                                            "--alignment_model", "DP"])
    entry.main(args)
    path = tmp_path / "out" / "matches.csv"
    assert path.exists()
    q, r = load_features(str(tmp_path / "q.npz"), Dataset.QUERIES), load_features(str(tmp_path / "r.npz"), Dataset.REFS)
    want = entry.localize_and_verify(q, r, entry.search(q, r), alignment_model="DP",
                                     model=align_contract.ContractModel("DP", min_length=4))
    assert want
    Match.write_csv(want, str(tmp_path / "want.csv"))
    assert path.read_bytes() == (tmp_path / "want.csv").read_bytes()
