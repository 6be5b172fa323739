"""The contract of vsc_match_maps_f32 (tests/match_maps_contract.py) against the host path it replaces: src.matching._best_view
and the two datasets, item by item and bit for bit -- plus the host logic of the device path that needs no device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import match_maps_cases as cases  # noqa: E402
import match_maps_contract as C  # noqa: E402


def _numpy_pair_similarity(q_bank, r_bank, pairs):
    """The pair_similarity seam of src.matching in numpy.  The tests below feed it a matrix S as the query "descriptors" and an
    identity matrix as the reference's: every product then has one non-zero term, so q @ r.T is S exactly, in any summation order."""
    offsets, parts = [0], []
    for q0, qn, r0, rn in pairs:
        parts.append((q_bank[q0:q0 + qn] @ r_bank[r0:r0 + rn].T).astype(np.float32).reshape(-1))
        offsets.append(offsets[-1] + parts[-1].size)
    return (np.concatenate(parts) if parts else np.zeros(0, np.float32)), np.array(offsets, np.int64)


def _host_path(s, frames, resolution):
    """(view start, classifier canvases [2, 3, R, R], refinement canvas [3, R, R], h, w) of the host path for one matrix."""
    from src import matching
    query, ref, len_map = {"Q": s}, {"R": np.eye(s.shape[1], dtype=np.float32)}, {"Q": frames}
    cand = [("Q", "R", np.float32(0))]
    feats, infos = matching.generate_candidates_classfiy_feature(query, ref, cand, len_map, _numpy_pair_similarity)
    ds = matching.MatchClassifyDataset(feats, infos, (resolution, resolution))
    meta = matching.generate_matching_feature(query, ref, len_map, cand, _numpy_pair_similarity)
    fea, _, _, h, w = matching.MatchRefineDataset(meta, (resolution, resolution), _numpy_pair_similarity)[0]
    start = matching._best_view(s, frames) if s.shape[0] != frames else 0
    return start, np.stack([ds[0][0], ds[1][0]]), fea, h, w


def _random_items(seed, count):
    rs = np.random.RandomState(seed)
    frames_set = list(range(1, 13)) + [40, 170]
    for k in range(count):
        frames = frames_set[k % len(frames_set)]
        views = 1 + (k // len(frames_set)) % 5
        r_rows = int(rs.randint(1, 40 if frames == 170 else 260))
        if k % 7 == 3:                                             # coarse values: equal maxima, equal scores, first view wins
            s = (rs.randint(-6, 7, (frames * views, r_rows)) / 4.0).astype(np.float32)
        elif k % 7 == 5:                                           # all negative
            s = -rs.uniform(0.01, 1.0, (frames * views, r_rows)).astype(np.float32)
        else:
            s = rs.uniform(-1.0, 1.0, (frames * views, r_rows)).astype(np.float32)
        yield s, frames, (160, 224, 8)[k % 3]


def test_contract_equals_the_host_path_on_random_items():
    """frames 1 .. 12, 40 and 170 with 1 .. 5 views each: the contract's view, classifier canvases (map + transpose) and refinement
    canvas are the host path's, bit for bit; so are the valid height and width."""
    count = views_seen = 0
    for s, frames, R in _random_items(2024, 2800):
        start, cls, fea, h, w = _host_path(s, frames, R)
        item = [(0, s.shape[0], s.shape[1], frames)]
        vs, out = C.match_maps(s.reshape(-1), item, R, True)
        assert int(vs[0]) == start, (s.shape, frames)
        assert np.array_equal(C.bits(out.transpose(0, 3, 1, 2)), C.bits(cls)), (s.shape, frames, R)
        vs0, out0 = C.match_maps(s.reshape(-1), item, R, False)
        assert int(vs0[0]) == start and np.array_equal(C.bits(out0[0].transpose(2, 0, 1)), C.bits(fea))
        assert C.valid_hw(s.shape[0], s.shape[1], frames, R) == (h, w)
        count += 1
        views_seen += start > 0
    assert count == 2800 and views_seen > 500, "the random items hardly ever chose a later view"


def test_view_score_is_numpy_mean_of_the_sorted_tail():
    """The spelled-out pairwise order IS np.sort(x)[-10:].mean() in float32, for every length the tail can have."""
    rs = np.random.RandomState(1)
    for k in range(20000):
        x = rs.uniform(-1.0, 1.0, 1 + k % 24).astype(np.float32)
        want = np.sort(x)[-10:].mean()
        assert want.dtype == np.float32 and C.bits(C.view_score(x)) == C.bits(want), x


@pytest.mark.parametrize("resolution", [160, 224, 8])
def test_contract_equals_the_host_path_on_the_planted_items(resolution):
    for name, s, frames in cases.planted(resolution):
        if s.shape[1] == 0 or s.shape[0] == 0:
            continue                                   # the host path has no empty videos; the contract pads them with zeros
        start, cls, fea, h, w = _host_path(s, frames, resolution)
        vs, out = C.match_maps(s.reshape(-1), [(0, s.shape[0], s.shape[1], frames)], resolution, True)
        assert int(vs[0]) == start, name
        assert np.array_equal(C.bits(out.transpose(0, 3, 1, 2)), C.bits(cls)), name
        assert np.array_equal(C.bits(out[0].transpose(2, 0, 1)), C.bits(fea)), name


def test_planted_items_plant_what_they_say():
    by = {name: (s, frames) for name, s, frames in cases.planted(160)}
    s, frames = by["identical_views"]
    assert C.view_start(s, frames) == frames and np.array_equal(s[frames:2 * frames], s[2 * frames:3 * frames])
    s, frames = by["sum_order"]
    tops = [np.sort(s[v * 10:(v + 1) * 10].max(1)) for v in range(2)]
    assert not np.array_equal(tops[0], tops[1]) and C.view_start(s, frames) == 10
    seq = [cases._sum_sequential(t) for t in tops]
    assert not seq[1] > seq[0], "a one-by-one sum would pick the same view: the item decides nothing"
    s, frames = by["all_negative"]
    assert s.max() < 0 and s.shape[0] > frames
    flat, table = cases.pack(cases.planted(8))
    assert (table[:, 0] % 2 == 1).all() and table[0, 0] > 0
    for (off, q, r, _), (_, m, _) in zip(table, cases.planted(8)):
        assert np.array_equal(flat[off:off + q * r].reshape(q, r), m)


def test_contract_refuses_what_the_entry_refuses():
    flat = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="ragged"):
        C.match_maps(flat, [(0, 10, 3, 4)], 8, False)
    with pytest.raises(ValueError, match="outside"):
        C.match_maps(flat, [(50, 10, 6, 10)], 8, False)
    with pytest.raises(ValueError, match="frames"):
        C.match_maps(flat, [(0, 10, 3, 0)], 8, False)
    vs, out = C.match_maps(flat, np.zeros((0, 4), np.int64), 8, True)
    assert vs.shape == (0,) and out.shape == (0, 8, 8, 3)


def test_ragged_views_are_refused_by_name_before_any_device_work():
    """--query_frames can make a video's rows ragged: the device path names the video; the host path still serves it."""
    from src import matching
    query = {"Q000001": np.zeros((10, 4), np.float32), "Q000002": np.zeros((8, 4), np.float32)}
    ref = {"R000001": np.zeros((5, 4), np.float32)}
    assert matching._map_shape(query, ref, ("Q000002", "R000001", 0.0), {"Q000002": 4}, 160) == (8, 5, 4)
    assert matching._map_shape(query, ref, ("Q000002", "R000001", 0.0), {"Q000002": 8}, 6) == (6, 5, 8)
    with pytest.raises(ValueError, match="Q000001.*whole views"):
        matching.classify_candidates_hip([], query, ref, [("Q000001", "R000001", 0.0)], {"Q000001": 4})
    with pytest.raises(ValueError, match="Q000001.*whole views"):
        matching.refine_candidates_hip([], query, ref, {"Q000001": 4}, [("Q000001", "R000001", 0.0)])
    import infer_matching
    with pytest.raises(ValueError, match="maps must be"):
        infer_matching.run([], [], [], [], [], [], maps="gpu")
