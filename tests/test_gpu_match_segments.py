"""Segment extraction on the device (vsc_match_segments_f32, csrc/match_segments.hip) against the executable contract
(tests/seg_contract.py) on the fixture's maps (tests/golden/match_segments.json), and the layers above it:
src.matching.generate_matching_result(backend="hip"), match_refine's device maps, infer_matching.run(localize="hip")."""
import json
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import seg_cases  # noqa: E402
import seg_contract  # noqa: E402

pytestmark = pytest.mark.gpu

# Kernel vs contract score bound: both are float64; the sums (at most 224 * 224 = 50 176 terms) are taken in another order, which
# moves them by about n * 2^-53 ~ 6e-12 relative -- 1e-9 leaves two orders of magnitude.
SCORE_TOL = 1e-9
PASSES = seg_cases.PASSES


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "match_segments.json")) as f:
        return json.load(f)


def _pack(maps):
    """list of fp32 [h, w] arrays -> (flat device tensor, items int64 [n, 3])"""
    import torch
    items, off = [], 0
    for m in maps:
        items.append((off, m.shape[0], m.shape[1]))
        off += m.size
    flat = np.concatenate([np.ascontiguousarray(m, np.float32).reshape(-1) for m in maps]) if maps else np.zeros(0, np.float32)
    return torch.from_numpy(flat).cuda(), np.array(items, dtype=np.int64).reshape(-1, 3)


def _rows(segments, scores, counts, i, t):
    k = int(counts[i, t])
    return [[*(int(v) for v in segments[i, t, j]), float(scores[i, t, j])] for j in range(k)]


def _launch(maps, passes=PASSES, max_segments=8):
    from vsc_hip import ops
    flat, items = _pack(maps)
    seg, sc, cnt = ops.match_segments(flat, items, [p[0] for p in passes], [p[1] for p in passes], max_segments)
    return seg.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()


def test_kernel_equals_contract_on_every_fixture_entry(fixture):
    """All three tiers: the kernel implements the contract, whatever sklearn's rounding noise would have decided.  Entries whose
    contract margin is a knife-edge (< 1e-9) are left out: a float64 decision there may turn on the summation order."""
    cases = fixture["cases"]
    maps = [seg_cases.matrix(c) for c in cases]
    seg, sc, cnt = _launch(maps)
    compared = segments = 0
    worst = 0.0
    for i, case in enumerate(cases):
        for t, p in enumerate(case["passes"]):
            if p["margin"] is not None and p["margin"] < fixture["knife_edge"]:
                continue
            want, _ = seg_contract.segments(maps[i], p["threshold"], p["std_ratio"])     # group order = raster order of first pixels
            got = _rows(seg, sc, cnt, i, t)
            assert len(got) == len(want), (case["name"], p["threshold"], got, want)
            for g, w in zip(got, want):
                assert g[:4] == w[:4], (case["name"], p["threshold"], got, want)
                worst = max(worst, abs(g[4] - w[4]))
                assert abs(g[4] - w[4]) <= SCORE_TOL, (case["name"], p["threshold"], g, w)
            compared += 1
            segments += len(want)
    print(f"{compared} entries, {segments} segments, largest score difference {worst:.3e}")
    assert compared >= 200 and segments >= 200


def test_one_launch_equals_one_by_one_and_runs_repeat(fixture):
    cases = [c for c in fixture["cases"] if c["h"] * c["w"] <= 130 * 130][:24]
    maps = [seg_cases.matrix(c) for c in cases]
    a = _launch(maps)
    b = _launch(maps)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for i, m in enumerate(maps):
        seg, sc, cnt = _launch([m])
        assert np.array_equal(cnt[0], a[2][i])
        for t in range(len(PASSES)):
            assert _rows(seg, sc, cnt, 0, t) == _rows(*a, i, t), cases[i]["name"]


def test_small_max_segments_reports_the_true_count(fixture):
    from vsc_hip import ops
    by = seg_cases.by_name()
    m = np.zeros((224, 224), np.float32)
    for b, (q0, r0) in enumerate([(2, 5), (50, 120), (100, 20), (160, 150)]):      # four clean copies far apart
        for t in range(40):
            m[q0 + t, r0 + t] = 0.9 - 0.05 * b - 0.002 * t
    want, _ = seg_contract.segments(m, 0.35, 0.5)
    assert len(want) == 4
    flat, items = _pack([m, seg_cases.matrix(by["clean_01_60x80"])])
    thr, ratio = np.array([0.35], np.float32), np.array([0.5], np.float64)
    seg, sc, cnt = ops.match_segments_once(flat, items, thr, ratio, 1)
    assert int(cnt[0, 0]) == 4 and seg.shape == (2, 1, 1, 4)                          # uncapped count, one slot written
    assert [int(v) for v in seg[0, 0, 0].cpu()] == want[0][:4]
    seg, sc, cnt = ops.match_segments(flat, items, thr, ratio, 1)                     # the wrapper re-runs wider
    assert seg.shape[2] == 4 and [[int(v) for v in s] for s in seg[0, 0].cpu()] == [w[:4] for w in want]
    seg0, _, cnt0 = ops.match_segments_once(flat, items, thr, ratio, 0)               # count only
    assert int(cnt0[0, 0]) == 4 and seg0.numel() == 0


def test_limits_are_refused():
    import torch
    from vsc_hip import ops
    from vsc_hip._lib import VscHipError
    flat = torch.zeros(225 * 4, device="cuda")
    with pytest.raises(VscHipError, match="limit"):
        ops.match_segments(flat, [(0, 225, 4)], [0.35], [0.5])
    with pytest.raises(VscHipError, match="outside"):
        ops.match_segments(flat, [(0, 224, 224)], [0.35], [0.5])
    seg, sc, cnt = ops.match_segments(flat, np.zeros((0, 3), np.int64), [0.35], [0.5])
    assert cnt.shape == (0, 1)


def test_generate_matching_result_backend_hip(fixture, monkeypatch):
    from src import matching
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "sklearn", None)
    by = seg_cases.by_name()
    names = ["clean_01_60x80", "thin_02_120x90", "thick_00_120x90", "edge_specks_only", "edge_empty", "thin_05_200x224"]
    maps = [[f"Q{i}", f"R{i}", seg_cases.matrix(by[n]), None] for i, n in enumerate(names)]
    for thr, ratio in PASSES:
        got = matching.generate_matching_result(maps, threshold=thr, std_ratio=ratio, backend="hip")
        want = seg_contract.matching_result(maps, thr, ratio)
        assert [r[:6] for r in got] == [r[:6] for r in want]
        assert np.allclose([r[6] for r in got], [r[6] for r in want], rtol=0, atol=SCORE_TOL)
    allp = matching.generate_matching_results_hip(maps, PASSES)
    assert [len(r) for r in allp] == [len(seg_contract.matching_result(maps, t, r)) for t, r in PASSES]
    assert matching.generate_matching_result([], 0.35, 0.5, backend="hip") == []


def _planted_map(h, w, seed):
    """A clean planted copy per map: a thin line of slope 1, zero background (no boundary points in typical trials)."""
    rs = np.random.RandomState(seed)
    m = np.zeros((h, w), np.float32)
    n = int(rs.randint(12, min(h, w) - 4))
    q0, r0 = int(rs.randint(0, h - n)), int(rs.randint(0, w - n))
    for t in range(n):
        m[q0 + t, r0 + t] = np.float32(0.9) - np.float32(0.003) * np.float32(t)
    return m, (q0, r0, q0 + n - 1, r0 + n - 1)


def test_infer_matching_run_localize_hip(monkeypatch):
    """infer_matching.run with the probability maps fed at the match_refine seam (planted copies; everything before it runs
    as usual on synthetic descriptors and random-weight classifiers): localize="hip" imports neither scipy nor sklearn, keeps
    the maps on the device, finds every planted segment, and equals localize="host" where no trial met a boundary point."""
    import torch
    import cnn_synth
    import infer_matching
    from src import matching
    from vsc.baseline.score_normalization import ref_score_normalize
    from vsc.index import VideoFeature
    rng = np.random.RandomState(7)
    d = 512
    mk = lambda pre, i, n: VideoFeature(video_id=f"{pre}{i:06d}", timestamps=np.arange(n, dtype=np.float32),
                                        feature=rng.randn(n, d).astype(np.float32))
    refs = [mk("R", 200000 + i, n) for i, n in enumerate((30, 44, 25))]
    norm = [mk("R", 100000 + i, 20) for i in range(4)]
    queries = [mk("Q", 300000 + i, n) for i, n in enumerate((18, 27))]
    queries[0].feature[3:15] = refs[1].feature[10:22] + 0.05 * rng.randn(12, d).astype(np.float32)
    sn_refs = ref_score_normalize(refs, norm, beta=1.5, nk=10)
    cls_models, _ = matching.load_match_models([cnn_synth.mobilenetv3_small_state(40)], [], "cuda")
    monkeypatch.setattr(infer_matching, "MATCH_CLS_THRESHOLD", -1.0)            # every candidate reaches the refinement step
    planted, calls = {}, []

    def fake_refine(refine_models, match_meta, device="cuda", device_maps=False, **kw):
        calls.append(device_maps)
        rows = []
        for k, (qid, rid, qf, rf) in enumerate(match_meta):
            m, seg = _planted_map(min(len(qf), 224), min(len(rf), 224), 100 + k)
            planted[qid, rid] = (m, seg)
            rows.append([qid, rid, m, None])
        return matching._to_device_maps(rows) if device_maps else rows

    monkeypatch.setattr(matching, "match_refine", fake_refine)
    host = infer_matching.run(queries, norm, refs, sn_refs, cls_models, [], localize="host")
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "sklearn", None)
    hip = infer_matching.run(queries, norm, refs, sn_refs, cls_models, [], localize="hip")
    assert calls == [False, True] and len(planted) >= 1
    for (qid, rid), (m, (qs, rs, qe, re_)) in planted.items():
        assert any(r[:2] == [qid, rid] and (r[2], r[3], r[4], r[5]) == (qs, qe, rs, re_) for r in hip), (qid, rid, hip)
    # the contract's rows, through the same grouping as run()
    want = {}
    for (qid, rid), (m, _) in planted.items():
        for thr, ratio in PASSES:
            for x1, y1, x2, y2, s in seg_contract.segments(m, thr, ratio)[0]:
                key = (qid, rid, float(x1), float(x2), float(y1), float(y2))
                want[key] = max(want.get(key, -np.inf), s)
    assert sorted(want) == sorted(tuple(r[:6]) for r in hip)
    for r in hip:
        assert abs(r[6] - want[tuple(r[:6])]) <= SCORE_TOL
    clean = {k for k, (m, _) in planted.items() if not any(seg_contract.segments(m, t, r)[1]["boundary"] for t, r in PASSES)}
    assert clean, "no map without boundary points: the comparison with the host path would be empty"
    pick = lambda rows: sorted((tuple(r[:6]), r[6]) for r in rows if (r[0], r[1]) in clean)
    assert [k for k, _ in pick(hip)] == [k for k, _ in pick(host)]
    assert np.allclose([s for _, s in pick(hip)], [s for _, s in pick(host)], rtol=0, atol=4e-6)
    with pytest.raises(ValueError, match="localize"):
        infer_matching.run(queries, norm, refs, sn_refs, cls_models, [], localize="gpu")


def test_infer_matching_cli_localize_hip_writes_the_csv(monkeypatch, tmp_path):
    """`python infer_matching.py ... --localize hip` through main(): argument parsing, run(), the csv -- with scipy and sklearn
    unimportable.  The networks are the seam: load_match_models hands back a random-weight classifier, match_refine planted maps."""
    import argparse
    import csv
    import cnn_synth
    import infer_matching
    from src import matching
    from vsc.baseline.score_normalization import ref_score_normalize
    from vsc.index import VideoFeature
    from vsc.storage import store_features
    rng = np.random.RandomState(7)
    d = 512
    mk = lambda pre, i, n: VideoFeature(video_id=f"{pre}{i:06d}", timestamps=np.arange(n, dtype=np.float32),
                                        feature=rng.randn(n, d).astype(np.float32))
    refs = [mk("R", 200000 + i, n) for i, n in enumerate((30, 44, 25))]
    norm = [mk("R", 100000 + i, 20) for i in range(4)]
    queries = [mk("Q", 300000 + i, n) for i, n in enumerate((18, 27))]
    queries[0].feature[3:15] = refs[1].feature[10:22] + 0.05 * rng.randn(12, d).astype(np.float32)
    paths = {}
    for name, feats in (("q", queries), ("norm", norm), ("refs", refs), ("sn", ref_score_normalize(refs, norm, beta=1.5, nk=10))):
        paths[name] = str(tmp_path / f"{name}.npz")
        store_features(paths[name], feats)
    cls_models, _ = matching.load_match_models([cnn_synth.mobilenetv3_small_state(40)], [], "cuda")
    monkeypatch.setattr(matching, "load_match_models", lambda cls_sds, refine_sds, device="cuda": (cls_models, []))
    monkeypatch.setattr(infer_matching, "load_state_dict", lambda path: {})
    monkeypatch.setattr(infer_matching, "MATCH_CLS_THRESHOLD", -1.0)
    planted = {}

    def fake_refine(refine_models, match_meta, device="cuda", device_maps=False, **kw):
        assert device_maps
        rows = []
        for k, (qid, rid, qf, rf) in enumerate(match_meta):
            m, seg = _planted_map(min(len(qf), 224), min(len(rf), 224), 100 + k)
            planted[qid, rid] = seg
            rows.append([qid, rid, m, None])
        return matching._to_device_maps(rows)

    monkeypatch.setattr(matching, "match_refine", fake_refine)
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "sklearn", None)
    out = tmp_path / "out" / "matches.csv"
    infer_matching.main(argparse.Namespace(query_features=paths["q"], norm_refs=paths["norm"], refs=paths["refs"], sn_refs=paths["sn"],
                                           cls_models=["cls.pt"], refine_models=["refine.pt"], query_frames=None,
                                           candidates_csv=str(tmp_path / "cands.csv"), output=str(out), localize="hip"))
    assert sys.modules["scipy"] is None and sys.modules["sklearn"] is None
    with open(out) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["query_id", "ref_id", "query_start", "query_end", "ref_start", "ref_end", "score"] and planted
    found = {(r[0], r[1], float(r[2]), float(r[3]), float(r[4]), float(r[5])) for r in rows[1:]}
    for (qid, rid), (qs, rs, qe, re_) in planted.items():
        assert (qid, rid, float(qs), float(qe), float(rs), float(re_)) in found, (qid, rid, rows)


def test_match_refine_device_maps_equal_the_host_rows():
    """match_refine(device_maps=True): the same cropped maps as the default, on the device as a flat buffer plus a table."""
    import cnn_synth
    from src import matching
    rng = np.random.RandomState(3)
    _, refine_models = matching.load_match_models([], [cnn_synth.hrnet_refine_state(33)], "cuda")
    meta = []
    for qn, rn in ((20, 36), (7, 11), (230, 40)):
        q, r = rng.randn(qn, 64).astype(np.float32), rng.randn(rn, 64).astype(np.float32)
        meta.append((f"Q{qn}", f"R{rn}", q / np.linalg.norm(q, axis=1, keepdims=True), r / np.linalg.norm(r, axis=1, keepdims=True)))
    host = matching.match_refine(refine_models, meta, batch_size=2, device="cuda")
    dev = matching.match_refine(refine_models, meta, batch_size=2, device="cuda", device_maps=True)
    assert dev.ids == [(a, b) for a, b, _, _ in host] and len(dev) == 3
    flat = dev.flat.cpu().numpy()
    for (off, h, w), (_, _, prob, _) in zip(dev.items, host):
        assert (h, w) == prob.shape and np.array_equal(flat[off:off + h * w].reshape(h, w), prob)
    assert int(dev.items[-1, 0] + dev.items[-1, 1] * dev.items[-1, 2]) == flat.size


def _full_size_maps(count, seed=900):
    out = []
    for i in range(count):
        rs = np.random.RandomState(seed + i)
        case = dict(seed=seed + i, h=224, w=224, noise=0.03, specks=12, thick=i % 3,
                    bands=seg_cases._bands(rs, 224, 224, 1 + i % 3, seg_cases.SLOPES))
        out.append(seg_cases.matrix(case))
    return out


def test_full_size_batch_repeats_bit_for_bit():
    """every new kernel gets a full-size repeat test -- 24 maps of 224 x 224 at the three thresholds, 5 passes."""
    maps = _full_size_maps(24)
    first = _launch(maps)
    assert int(first[2].sum()) > 24
    for _ in range(4):
        again = _launch(maps)
        for x, y in zip(first, again):
            assert x.tobytes() == y.tobytes()


def test_hip_path_beats_the_host_path_on_64_full_size_maps():
    """64 maps of 224 x 224 at the three thresholds: the device path -- maps already on the device, as match_refine leaves them,
    one launch, segments copied back -- against the host path (scipy + sklearn) timed here on the same maps."""
    import torch
    from src import matching
    maps = _full_size_maps(64, seed=1200)
    rows = [[f"Q{i}", f"R{i}", m, None] for i, m in enumerate(maps)]
    dev = matching._to_device_maps(rows)
    matching.generate_matching_results_hip(dev, PASSES)                               # warm-up: module load, scratch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hip = matching.generate_matching_results_hip(dev, PASSES)
    torch.cuda.synchronize()
    t_hip = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = [matching.generate_matching_result(rows, threshold=t, std_ratio=r) for t, r in PASSES]
    t_host = time.perf_counter() - t0
    print(f"64 maps x 3 thresholds: hip {t_hip * 1e3:.1f} ms ({64 / t_hip:.0f} maps/s), host {t_host * 1e3:.1f} ms ({64 / t_host:.1f} maps/s); "
          f"segments hip {[len(r) for r in hip]}, host {[len(r) for r in host]}")
    assert sum(len(r) for r in hip) > 64
    assert t_hip < t_host
