"""Best view + network input canvases on the device (vsc_match_maps_f32, csrc/match_maps.hip) against the executable contract
(tests/match_maps_contract.py) on the planted items (tests/match_maps_cases.py), and the layers above it:
src.matching.classify_candidates_hip / refine_candidates_hip against the host functions, infer_matching.run(maps="hip").
Every comparison is on uint32 views, bit for bit; no case is left out -- selection by `>` on identically rounded fp32 values
has no knife edges."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import match_maps_cases as cases  # noqa: E402
import match_maps_contract as C  # noqa: E402

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def _reference(resolution):
    """(items, flat, table, contract's view starts, contract's canvases with the transpose) per canvas side: computed once."""
    if resolution not in _REFERENCE:
        items = cases.planted(resolution)
        flat, table = cases.pack(items)
        starts, out = C.match_maps(flat, table, resolution, True)
        for a in (flat, table, starts, out):
            a.setflags(write=False)
        _REFERENCE[resolution] = (items, flat, table, starts, out)
    return _REFERENCE[resolution]


def _launch(sims, table, resolution, with_transpose):
    """One call over `table` on the device tensor `sims`, into an output pre-filled with NaN -> (view starts, canvases) as numpy."""
    import torch
    from vsc_hip import ops
    n = len(table)
    out = torch.full((n * (2 if with_transpose else 1), resolution, resolution, 3), float("nan"), dtype=torch.float32, device="cuda")
    maps, starts = ops.match_maps(sims, table, resolution, with_transpose, out=out)
    assert maps.shape == (out.shape[0], 3, resolution, resolution) and maps.data_ptr() == out.data_ptr()
    assert maps.permute(0, 2, 3, 1).is_contiguous()          # what vsc_hip.cnn._nhwc takes without a copy
    return starts.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("resolution", [160, 224, 8])
def test_kernel_equals_contract_on_every_planted_item(resolution):
    """Single views smaller / taller / wider than the canvas, r_rows = 1, frames 1 .. 170 with 2, 3 and 5 views, negative
    similarities, identical views, the summation-order pair, the tile edges, empty items; offsets non-zero and odd."""
    import torch
    items, flat, table, want_starts, want = _reference(resolution)
    sims = torch.tensor(flat, device="cuda")
    starts, out = _launch(sims, table, resolution, True)
    wrong = [(it[0], int(a), int(b)) for it, a, b in zip(items, starts, want_starts) if a != b]
    assert not wrong, wrong
    assert not np.isnan(out).any(), "an element of the output was not written"
    for p, it in enumerate(items):
        assert np.array_equal(C.bits(out[2 * p:2 * p + 2]), C.bits(want[2 * p:2 * p + 2])), it[0]
    starts0, out0 = _launch(sims, table, resolution, False)           # without the transpose: the even slices
    assert np.array_equal(starts0, want_starts)
    assert np.array_equal(C.bits(out0), C.bits(want[0::2]))
    assert sum(int(s) > 0 for s in want_starts) >= 10, "hardly any planted item chooses a later view"


def test_no_items():
    import torch
    from vsc_hip import ops
    maps, starts = ops.match_maps(torch.zeros(4, device="cuda"), np.zeros((0, 4), np.int64), 160, True)
    assert maps.shape == (0, 3, 160, 160) and starts.shape == (0,)


def test_more_items_than_one_launch_carries():
    """The item table travels in the kernel arguments, 128 items per launch: 300 items cross two chunk boundaries."""
    import torch
    rs = np.random.RandomState(17)
    items = [(f"i{k}", rs.uniform(-1, 1, ((1 + k % 4) * (1 + k % 5), 1 + k % 11)).astype(np.float32), 1 + k % 5) for k in range(300)]
    flat, table = cases.pack(items)
    want_starts, want = C.match_maps(flat, table, 8, True)
    starts, out = _launch(torch.from_numpy(flat).cuda(), table, 8, True)
    assert np.array_equal(starts, want_starts) and np.array_equal(C.bits(out), C.bits(want))


def test_one_launch_equals_item_by_item_and_runs_repeat():
    import torch
    items, flat, table, want_starts, want = _reference(160)
    sims = torch.tensor(flat, device="cuda")
    starts, out = _launch(sims, table, 160, True)
    again = _launch(sims, table, 160, True)
    assert starts.tobytes() == again[0].tobytes() and out.tobytes() == again[1].tobytes()
    for p, it in enumerate(items):
        s1, o1 = _launch(sims, table[p:p + 1], 160, True)
        assert s1[0] == starts[p] and o1.tobytes() == out[2 * p:2 * p + 2].tobytes(), it[0]


def test_refusals():
    import torch
    from vsc_hip import ops
    from vsc_hip._lib import VscHipError
    sims = torch.zeros(100, device="cuda")
    with pytest.raises(VscHipError, match="ragged"):
        ops.match_maps(sims, [(0, 10, 3, 4)], 8, False)
    with pytest.raises(VscHipError, match="outside"):
        ops.match_maps(sims, [(50, 10, 6, 10)], 8, False)
    with pytest.raises(VscHipError, match="frames"):
        ops.match_maps(sims, [(0, 10, 3, 0)], 8, False)
    with pytest.raises(VscHipError, match="no columns"):
        ops.match_maps(sims, [(0, 8, 0, 4)], 8, False)
    with pytest.raises(VscHipError, match="resolution"):
        ops.match_maps(sims, [(0, 2, 2, 2)], 1025, False)


# ---- the layers above the kernel ---------------------------------------------------------------------------------------------
def _unit_rows(rs, n, d):
    x = rs.randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _synthetic_videos(seed=21, d=64):
    """Queries with one, two and three views and references, with lengths either side of 160 and of 224 -> (query, ref, len_map,
    candidates): every (query, reference) pair is a candidate."""
    rs = np.random.RandomState(seed)
    query, len_map = {}, {}
    for k, (frames, views, rows) in enumerate([(12, 1, 12), (150, 2, 300), (170, 3, 510), (230, 1, 230), (230, 2, 460), (100, 1, 60)]):
        qid = f"Q{300000 + k}"
        query[qid], len_map[qid] = _unit_rows(rs, rows, d), frames
    ref = {f"R{200000 + k}": _unit_rows(rs, n, d) for k, n in enumerate((30, 159, 161, 223, 226))}
    for qid, rid, at in (("Q300001", "R200001", 150), ("Q300002", "R200003", 340), ("Q300004", "R200004", 230)):   # copies inside later views
        n = min(60, len(ref[rid]))
        query[qid][at:at + n] = ref[rid][:n]
    candidates = [(qid, rid, np.float32(0.5)) for qid in query for rid in ref]
    return query, ref, len_map, candidates


@pytest.fixture(scope="module")
def networks():
    import cnn_synth
    from src import matching
    return matching.load_match_models([cnn_synth.mobilenetv3_small_state(40), cnn_synth.mobilenetv3_small_state(41)],
                                      [cnn_synth.hrnet_refine_state(33)], "cuda")


def test_candidate_lists_equal_the_host_functions(networks, monkeypatch):
    """The test the parent fails: classify_candidates_hip / refine_candidates_hip return exactly what
    generate_candidates_classfiy_feature + match_classify and generate_matching_feature + match_refine return."""
    from src import matching
    cls_models, refine_models = networks
    query, ref, len_map, candidates = _synthetic_videos()
    feats, infos = matching.generate_candidates_classfiy_feature(query, ref, candidates, len_map)
    host = matching.match_classify(cls_models, feats, [(q, r) for q, r, _ in infos])
    hip = matching.classify_candidates_hip(cls_models, query, ref, candidates, len_map)
    assert len(hip) == 2 * len(candidates) and hip == host
    assert len({p for _, _, p in hip}) > len(candidates), "the classifier hardly tells the maps apart"
    with monkeypatch.context() as m:
        m.setattr(matching, "MATCH_MAPS_FLOAT_BUDGET", 100000)             # most groups split, some items exceed it alone
        assert matching.classify_candidates_hip(cls_models, query, ref, candidates, len_map) == host
    assert matching.classify_candidates_hip(cls_models, query, ref, candidates, len_map, batch_size=14) == \
        matching.match_classify(cls_models, feats, [(q, r) for q, r, _ in infos], batch_size=14)

    picked = candidates[3:23]                                               # every query, every reference, two network batches
    meta = matching.generate_matching_feature(query, ref, len_map, picked)
    assert any(len(m[2]) != len(query[m[0]]) and not np.array_equal(m[2], query[m[0]][:len(m[2])]) for m in meta), "no later view chosen"
    host_rows = matching.match_refine(refine_models, meta)
    hip_rows = matching.refine_candidates_hip(refine_models, query, ref, len_map, picked)
    assert len(hip_rows) == len(host_rows) == len(picked)
    for a, b in zip(hip_rows, host_rows):
        assert a[:2] == b[:2] and a[2].shape == b[2].shape and a[3].shape == b[3].shape, (a[:2], b[:2])
        assert np.array_equal(C.bits(a[2]), C.bits(b[2])) and np.array_equal(C.bits(a[3]), C.bits(b[3])), a[:2]
    host_dev = matching.match_refine(refine_models, meta, device_maps=True)
    hip_dev = matching.refine_candidates_hip(refine_models, query, ref, len_map, picked, device_maps=True)
    assert hip_dev.ids == host_dev.ids and np.array_equal(hip_dev.items, host_dev.items)
    assert np.array_equal(C.bits(hip_dev.flat.cpu().numpy()), C.bits(host_dev.flat.cpu().numpy()))
    assert matching.classify_candidates_hip(cls_models, query, ref, [], len_map) == []
    assert matching.refine_candidates_hip(refine_models, query, ref, len_map, []) == []


def _planted_copy_set(seed=7, d=512):
    """6 query videos (two of them with several views) x 8 reference videos, a planted copy in every query."""
    from vsc.index import VideoFeature
    rs = np.random.RandomState(seed)

    def video(pre, i, frames, views=1):
        return VideoFeature(video_id=f"{pre}{i:06d}", timestamps=np.tile(np.arange(frames, dtype=np.float32), views),
                            feature=rs.randn(frames * views, d).astype(np.float32))
    refs = [video("R", 200000 + i, n) for i, n in enumerate((30, 44, 25, 52, 18, 37, 60, 41))]
    norm = [video("R", 100000 + i, 20) for i in range(4)]
    queries = [video("Q", 300000 + i, n, v) for i, (n, v) in enumerate(((18, 1), (27, 2), (33, 1), (22, 3), (40, 1), (15, 1)))]
    for k, q in enumerate(queries):
        frames = len(np.unique(q.timestamps))
        n, at = min(12, frames - 3), len(q.feature) - frames + 2            # inside the LAST view
        q.feature[at:at + n] = refs[k].feature[5:5 + n] + 0.05 * rs.randn(n, d).astype(np.float32)
    return queries, norm, refs


@pytest.mark.parametrize("localize", ["host", "hip"])
def test_infer_matching_run_maps_hip_returns_the_rows_of_maps_host(networks, monkeypatch, localize):
    """run(maps="hip") against run(maps="host") under either localisation: the same rows, and on the way the same classifier
    probabilities for every candidate and the same probability maps from the refinement networks, bit for bit.  Under
    localize="host" only the 14 best candidates go on: scipy + sklearn cost ~0.1 s per candidate."""
    import infer_matching
    from src import matching
    from vsc.baseline.score_normalization import ref_score_normalize
    cls_models, refine_models = networks
    queries, norm, refs = _planted_copy_set()
    sn_refs = ref_score_normalize(refs, norm, beta=1.5, nk=10)
    monkeypatch.setattr(infer_matching, "MATCH_CLS_THRESHOLD", -1.0)         # every candidate reaches the refinement step
    if localize == "host":
        search = matching.search_candidate_pairs
        monkeypatch.setattr(matching, "search_candidate_pairs", lambda *a, **kw: search(*a, **kw)[:14])
    calls, returned = [], {}
    for name in ("generate_candidates_classfiy_feature", "match_classify", "generate_matching_feature", "match_refine",
                 "classify_candidates_hip", "refine_candidates_hip"):
        def spy(*a, _f=getattr(matching, name), _n=name, **kw):
            calls.append(_n)
            returned[_n] = _f(*a, **kw)
            return returned[_n]
        monkeypatch.setattr(matching, name, spy)
    host = infer_matching.run(queries, norm, refs, sn_refs, cls_models, refine_models, localize=localize, maps="host")
    assert calls == ["generate_candidates_classfiy_feature", "match_classify", "generate_matching_feature", "match_refine"]
    del calls[:]
    hip = infer_matching.run(queries, norm, refs, sn_refs, cls_models, refine_models, localize=localize, maps="hip")
    assert calls == ["classify_candidates_hip", "refine_candidates_hip"]
    n = len(returned["match_classify"]) // 2
    assert n >= 14 and returned["classify_candidates_hip"] == returned["match_classify"]
    rows_of = {q.video_id: len(q.feature) for q in queries}
    assert any(len(m[2]) < rows_of[m[0]] for m in returned["generate_matching_feature"]), "no multi-view candidate"
    a, b = returned["refine_candidates_hip"], returned["match_refine"]
    if localize == "hip":
        assert len(a) == n and a.ids == b.ids and np.array_equal(a.items, b.items)
        assert np.array_equal(C.bits(a.flat.cpu().numpy()), C.bits(b.flat.cpu().numpy()))
    else:
        assert len(a) == len(b) == n
        for x, y in zip(a, b):
            assert x[:2] == y[:2] and np.array_equal(C.bits(x[2]), C.bits(y[2])) and np.array_equal(C.bits(x[3]), C.bits(y[3]))
    print(f"localize={localize}: {n} candidates, {len(host)} rows")
    assert hip == host
    with pytest.raises(ValueError, match="maps must be"):
        infer_matching.run(queries, norm, refs, sn_refs, cls_models, refine_models, localize=localize, maps="device")
    ragged = {queries[1].video_id: 20}                                       # 54 rows in views of 20
    with pytest.raises(ValueError, match=queries[1].video_id):
        infer_matching.run(queries, norm, refs, sn_refs, cls_models, refine_models, query_frames=ragged, localize=localize, maps="hip")


def test_hip_path_beats_the_host_path_on_2048_candidates(networks):
    """Step 3 (feature building + classification) on 2 048 candidates, a third of the queries with three views: the device path
    against the host path -- the code of before this path existed, unchanged -- timed here in the same process, on the same
    candidates, after a small warm-up of both.  Same rows; the ratio is printed (DESIGN 4.12 records it)."""
    import torch
    from src import matching
    cls_models, _ = networks
    rs = np.random.RandomState(5)
    query, ref, len_map = {}, {}, {}
    for k in range(64):
        frames, views = int(rs.randint(20, 201)), 3 if k % 3 == 0 else 1
        query[f"Q{k}"], len_map[f"Q{k}"] = _unit_rows(rs, frames * views, 128), frames
    for k in range(32):
        ref[f"R{k}"] = _unit_rows(rs, int(rs.randint(20, 201)), 128)
    candidates = [(q, r, np.float32(0.5)) for q in query for r in ref]
    assert len(candidates) == 2048

    def host_path(cands):
        feats, infos = matching.generate_candidates_classfiy_feature(query, ref, cands, len_map)
        return matching.match_classify(cls_models, feats, [(q, r) for q, r, _ in infos])

    def hip_path(cands):
        return matching.classify_candidates_hip(cls_models, query, ref, cands, len_map)

    host_path(candidates[:40]), hip_path(candidates[:40])                    # warm-up: module load, scratch, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hip = hip_path(candidates)
    torch.cuda.synchronize()
    t_hip = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = host_path(candidates)
    torch.cuda.synchronize()
    t_host = time.perf_counter() - t0
    print(f"2048 candidates -> 4096 maps: hip {t_hip * 1e3:.1f} ms ({4096 / t_hip:.0f} maps/s), host {t_host * 1e3:.1f} ms "
          f"({4096 / t_host:.0f} maps/s), ratio {t_host / t_hip:.1f}x")
    assert hip == host
    assert t_hip < t_host
