"""Temporal-network (TN) alignment on the HIP path (vsc_tn_align_f32, vsc_hip.alignment, the HipTN* localization classes and
`sscd_baseline --alignment hip`) against the reference's own `tn`, recorded in tests/golden/tn_align.json."""
import json
import os
import time

import numpy as np
import pytest

import tn_cases
from tools import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tn_align.json")
FIELDS = ("tn_max_step", "tn_top_k", "max_path", "min_sim", "min_length", "max_iou")


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


def _run(cases, mats, dev):
    """All `cases` in one launch per TN parameter set -> {name: (boxes, maxsim)}."""
    import torch

    from vsc_hip import ops
    out = {}
    groups = {}
    for c, m in zip(cases, mats):
        groups.setdefault((c["bias"],) + tuple(c["params"][k] for k in FIELDS), []).append((c, m))
    for key, items in groups.items():
        bias, p = key[0], dict(zip(FIELDS, key[1:]))
        sizes = [m.size for _, m in items]
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        table = np.array([[o, m.shape[0], m.shape[1]] for o, (_, m) in zip(offs, items)], dtype=np.int64).reshape(-1, 3)
        flat = torch.from_numpy(np.concatenate([m.reshape(-1) for _, m in items])).to(dev)
        boxes, counts, maxsim = ops.tn_align(flat, table, bias, p["tn_max_step"], p["tn_top_k"], p["max_path"], p["min_sim"],
                                             p["min_length"], p["max_iou"])
        boxes, counts, maxsim = boxes.cpu().numpy(), counts.cpu().numpy(), maxsim.cpu().numpy()
        for i, (c, _) in enumerate(items):
            out[c["name"]] = (boxes[i, :counts[i]].tolist(), maxsim[i, :counts[i]].copy())
    return out


@pytest.fixture(scope="module")
def batched(fixture, dev):
    mats = [tn_cases.matrix(c) for c in fixture["cases"]]
    return mats, _run(fixture["cases"], mats, dev)


def test_fixture_boxes_identical(fixture, batched):
    mats, got = batched
    bad = []
    for c, m in zip(fixture["cases"], mats):
        assert tn_cases.digest(m) == c["digest"], c["name"]
        if got[c["name"]][0] != c["boxes"]:
            bad.append((c["name"], got[c["name"]][0], c["boxes"]))
    assert not bad, f"{len(bad)} of {len(mats)} cases differ from the reference: {bad[:3]}"
    assert sum(len(c["boxes"]) for c in fixture["cases"]) > 300


def test_maxsim_bit_equal_to_host(fixture, batched):
    mats, got = batched
    n = 0
    for c, m in zip(fixture["cases"], mats):
        boxes, maxsim = got[c["name"]]
        bias = np.float32(c["bias"])
        for (x1, y1, x2, y2), s in zip(boxes, maxsim):
            want = np.float32((m + c["bias"])[x1:x2, y1:y2].max() - bias)
            assert want.view(np.uint32) == np.float32(s).view(np.uint32), (c["name"], (x1, y1, x2, y2), s, want)
            n += 1
    assert n > 300


def test_one_launch_equals_one_by_one(fixture, batched, dev):
    mats, got = batched
    picks = [i for i, c in enumerate(fixture["cases"]) if c["q"] * c["r"] < 50000][::4]
    for i in picks:
        c = fixture["cases"][i]
        alone = _run([c], [mats[i]], dev)[c["name"]]
        assert alone[0] == got[c["name"]][0], c["name"]
        assert np.array_equal(alone[1].view(np.uint32), got[c["name"]][1].view(np.uint32)), c["name"]


def test_forward_sim_interface(fixture, batched):
    from vsc_hip.alignment import TnAlignment
    mats, got = batched
    items = [(c, m) for c, m in zip(fixture["cases"], mats) if c["params"] == tn_cases.TN_SSCD and c["q"] * c["r"] < 50000]
    model = TnAlignment(**tn_cases.TN_SSCD)
    res = model.forward_sim([(c["name"], m + c["bias"]) for c, m in items])
    assert [k for k, _ in res] == [c["name"] for c, _ in items]
    assert all(boxes == c["boxes"] for (c, _), (_, boxes) in zip(items, res))
    assert model.forward_sim([]) == []


def _planted_videos(seed=5, dim=64):
    """Queries that copy segments of some references (small noise), plus unrelated videos."""
    from vsc.index import VideoFeature
    rs = np.random.RandomState(seed)
    refs = [VideoFeature(f"R{i:06d}", np.arange(60.0), synth.descriptor_bank(300 + i, 60, dim)) for i in range(12)]
    queries, planted = [], []
    for i in range(8):
        f = synth.descriptor_bank(600 + i, 40, dim)
        if i < 5:
            r, q0, r0, ln = 2 + i, 3 + i, 10 + 2 * i, 20 + i
            f[q0:q0 + ln] = refs[r].feature[r0:r0 + ln] + 0.02 * rs.randn(ln, dim).astype(np.float32)
            f[q0:q0 + ln] /= np.linalg.norm(f[q0:q0 + ln], axis=1, keepdims=True)
            planted.append((f"Q{i:06d}", refs[r].video_id, q0, q0 + ln - 1, r0, r0 + ln - 1))
        queries.append(VideoFeature(f"Q{i:06d}", np.arange(40.0), f))
    return queries, refs, planted


def _candidates(queries, refs):
    from vsc.metrics import CandidatePair
    return [CandidatePair(q.video_id, r.video_id, float(0.9 - 0.01 * j)) for j, (q, r) in
            enumerate((q, r) for q in queries for r in refs[:8])]


def test_vcsl_interface_equals_device_classes(dev):
    from vsc.baseline.localization import (HipTNLocalizationCandidateScore, HipTNLocalizationMaxSim,
                                           VCSLLocalizationCandidateScore, VCSLLocalizationMaxSim)
    from vsc_hip.alignment import TnAlignment
    queries, refs, planted = _planted_videos()
    cands = _candidates(queries, refs)
    model = TnAlignment(tn_max_step=5, min_length=4)
    want = VCSLLocalizationMaxSim(queries, refs, "TN", similarity_bias=0.5, model=model).localize_all(cands)
    got = HipTNLocalizationMaxSim(queries, refs, similarity_bias=0.5, tn_max_step=5, min_length=4).localize_all(cands)
    assert got == want and len(got) >= len(planted)
    assert [type(m.score) for m in got] == [type(m.score) for m in want]
    want = VCSLLocalizationCandidateScore(queries, refs, "TN", model=model).localize_all(cands)
    got = HipTNLocalizationCandidateScore(queries, refs, tn_max_step=5, min_length=4).localize_all(cands)
    assert got == want
    assert HipTNLocalizationMaxSim(queries, refs).localize_all([]) == []


def test_localize_and_verify_hip_both_branches(dev):
    import vsc.baseline.sscd_baseline as entry
    from vsc_hip.alignment import TnAlignment
    queries, refs, planted = _planted_videos(seed=6)
    cands = _candidates(queries, refs)
    for norm in (True, False):
        got = entry.localize_and_verify(queries, refs, cands, localize_per_query=8.0, score_normalization=norm,
                                        alignment="hip")
        want = entry.localize_and_verify(queries, refs, cands, localize_per_query=8.0, score_normalization=norm,
                                         model=TnAlignment(tn_max_step=5, min_length=4))
        assert got == want and got, norm
        hit = {(m.query_id, m.ref_id) for m in got}
        assert {(q, r) for q, r, *_ in planted} <= hit, norm
    with pytest.raises(ValueError, match="alignment"):
        entry.localize_and_verify(queries, refs, cands, alignment="dtw")


def _main(tmp_path, queries, refs, out):
    import vsc.baseline.sscd_baseline as entry
    from vsc.storage import store_features
    store_features(tmp_path / "q.npz", queries)
    store_features(tmp_path / "r.npz", refs)
    args = entry.build_parser().parse_args(["--query_features", str(tmp_path / "q.npz"), "--ref_features",
                                            str(tmp_path / "r.npz"), "--output_path", str(tmp_path / out), "--overwrite",
                                            "--alignment", "hip"])
    entry.main(args)
    return tmp_path / out / "matches.csv"


def test_entry_point_writes_matches_csv(dev, tmp_path):
    from vsc.metrics import Match, format_video_id, Dataset
    queries, refs, planted = _planted_videos(seed=7)
    path = _main(tmp_path, queries, refs, "out")
    assert path.exists()
    rows = Match.read_csv(path)
    assert rows
    for q, r, qs, qe, rs_, re_ in planted:
        qid, rid = format_video_id(q, Dataset.QUERIES), format_video_id(r, Dataset.REFS)
        own = [m for m in rows if (m.query_id, m.ref_id) in ((q, r), (qid, rid))]
        assert own, (q, r)
        cover = max(min(m.query_end, qe) - max(m.query_start, qs) for m in own)
        assert cover >= 0.6 * (qe - qs), (q, r, own)
        cover = max(min(m.ref_end, re_) - max(m.ref_start, rs_) for m in own)
        assert cover >= 0.6 * (re_ - rs_), (q, r, own)
    again = _main(tmp_path, queries, refs, "out2")
    assert again.read_bytes() == path.read_bytes()


def test_mixed_batch_wall_bound(dev):
    """512 pairs, shapes of the issue's CPU timings plus one 1000 x 4000 pair, under a stated bound (first call included)."""
    import torch

    from vsc_hip.alignment import TnAlignment
    shapes = [(30, 60), (60, 180), (120, 600)] * 170 + [(45, 90)] + [(1000, 4000)]
    assert len(shapes) == 512
    sizes = np.array([q * r for q, r in shapes], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    table = np.stack([offs, [q for q, _ in shapes], [r for _, r in shapes]], axis=1).astype(np.int64)
    g = torch.Generator(device=dev).manual_seed(11)
    flat = torch.rand(int(sizes.sum()), generator=g, device=dev) - 0.45
    model = TnAlignment(tn_max_step=5, min_length=4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    boxes, counts, maxsim = model.align(flat, table, 0.5)
    counts = counts.cpu()
    wall = time.perf_counter() - t0
    assert counts.shape == (512,) and int(counts.min()) >= 0 and int(counts.max()) <= 11
    assert wall < 2.0, f"512-pair TN batch took {wall:.2f} s (0.12 s measured on an MI355X)"
