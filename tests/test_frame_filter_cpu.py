"""The frame filter's contract (tests/frame_filter_contract.py) held against numpy and against the host path it replaces
(src/query_postprocess.py: greedy_select), the planted cases held to what they claim, and the host plumbing of
``frame_filter="host" | "hip"`` -- all without a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_filter_cases as cases  # noqa: E402
import frame_filter_contract as C  # noqa: E402
from src.query_postprocess import FRAME_FILTERS, FRAME_THRESHOLD, greedy_select  # noqa: E402

SMALL = cases.names(cases.EMULATED_MAX)
TIE_FREE = [n for n in cases.names() if cases.get(n)["tie_free"]]
TIED = [n for n in cases.names() if not cases.get(n)["tie_free"]]


def host_sim(s):
    """what select_frames hands greedy_select"""
    return s - np.eye(len(s), dtype=np.float32)


@pytest.mark.parametrize("name", cases.names())
def test_contract_means_are_numpys_bit_for_bit(name):
    s = cases.get(name)["s"]
    if len(s) == 0:
        assert C.means(s).shape == (0,)
        return
    assert np.array_equal(C.diagonal_removed(s).view(np.uint32), host_sim(s).view(np.uint32))
    want = host_sim(s).mean(0)
    assert want.dtype == np.float32 and np.array_equal(C.bits(C.means(s)), C.bits(want))


def test_the_chain_starts_from_the_first_row_and_the_division_is_float32():
    """the -0.0 corner: the chain starts from v[0][j], numpy's reduction from +0.0; the two differ only on a column of nothing but
    -0.0, which no matrix has -- v[j][j] = s[j][j] - 1.0f is never -0.0 -- so columns that BEGIN with -0.0 agree; and numpy's float64
    division rounded to float32 is the float32 division, on sums and lengths that do not divide evenly"""
    s = np.full((3, 3), -0.0, np.float32)
    s[np.arange(3), np.arange(3)] = 1.0
    s[:, 2] = [-0.0, -0.0, 1.0]                       # v[:, 2] = -0.0, -0.0, 0.0: ((-0.0 + -0.0) + 0.0) = +0.0
    m, want = C.means(s), host_sim(s).mean(0)
    assert np.array_equal(C.bits(m), C.bits(want))
    rng = np.random.default_rng(3)
    for L in (3, 7, 1499):
        sums = rng.uniform(-L, L, 4096).astype(np.float32)
        assert np.array_equal(C.bits(sums / np.float32(L)), C.bits((sums.astype(np.float64) / L).astype(np.float32)))
    col = np.array([[-0.0], [-0.0]], np.float32)
    assert not np.signbit(col.mean(0)[0]) and np.signbit((col[0] + col[1])[0])     # the unreachable corner itself
    assert not np.signbit(np.float32(1.0) - np.float32(1.0)) and np.float32(-0.0) == np.float32(0.0)


@pytest.mark.parametrize("name", TIE_FREE)
def test_contract_equals_the_host_path_where_no_means_tie(name):
    case = cases.get(name)
    s, L = case["s"], len(case["s"])
    kept, mean, order = C.keep(s, case["thr"])
    assert len(np.unique(mean)) == L, "the tie-free generator produced a tie"
    if L:
        assert np.array_equal(order, host_sim(s).mean(0).argsort()[::-1])
    assert kept.tolist() == greedy_select(host_sim(s), case["thr"])


@pytest.mark.parametrize("name", TIED)
def test_tied_cases_tie_and_follow_the_stable_rule(name):
    case = cases.get(name)
    kept, mean, order = C.keep(case["s"], case["thr"])
    L = len(mean)
    assert len(np.unique(mean)) < L
    # descending mean, descending index among equals
    for a, b in zip(order[:-1], order[1:]):
        assert mean[a] > mean[b] or (mean[a] == mean[b] and a > b)
    assert sorted(order.tolist()) == list(range(L))


def test_the_cases_tell_rows_from_columns_and_the_tie_rule_matters():
    """a filter that read column i for row i, or ranked by mean(1), gives another answer on the planted matrices; and on the
    tied_rule cases the opposite tie rule keeps other frames"""
    for name in ("planted_63", "planted_64", "planted_65", "planted_129", "planted_257", "planted_300"):
        case = cases.get(name)
        kept, mean, order = C.keep(case["s"], case["thr"])
        kept_t, mean_t, order_t = C.keep(np.ascontiguousarray(case["s"].T), case["thr"])
        assert 0 < len(kept) < len(mean), name                         # some frames go, some stay
        assert kept.tolist() != kept_t.tolist() and order.tolist() != order_t.tolist(), name
    for name in ("tied_rule_6", "tied_rule_65", "tied_rule_257"):
        case = cases.get(name)
        v, thr = C.diagonal_removed(case["s"]), np.float32(case["thr"])
        kept, mean, _ = C.keep(case["s"], case["thr"])
        removed = np.zeros(len(v), bool)
        for i in np.lexsort((np.arange(len(v)), -mean)):               # descending mean, ASCENDING index among equals
            if not removed[i]:
                removed |= v[i] > thr
        assert np.nonzero(~removed)[0].tolist() != kept.tolist(), name


def test_threshold_edges_of_the_planted_cases():
    """exactly float32(0.975) stays, one ulp above goes; thresholds at and below zero make frames remove themselves"""
    s = np.full((3, 3), 0.1, np.float32)
    s[np.arange(3), np.arange(3)] = 1.0
    s[0, 1] = np.float32(cases.THR)
    s[0, 2] = cases.ABOVE
    s[:, 0] += np.float32(0.5)                                           # frame 0 is visited first
    s[0, 0] = 1.0
    assert C.keep(s, cases.THR)[0].tolist() == [0, 1]
    assert len(C.keep(cases.get("none_above_65")["s"], cases.THR)[0]) == 65
    assert len(C.keep(cases.get("all_above_129")["s"], cases.THR)[0]) == 1
    neg = cases.get("negative_thr_64")
    kept = C.keep(neg["s"], neg["thr"])[0]
    assert 0 < len(kept) < 64 and all(k % 2 == 1 for k in kept)            # the frames with diagonal 1.0 removed themselves
    zero = cases.get("zero_thr_diag_63")
    kept = C.keep(zero["s"], zero["thr"])[0]
    assert not any(k % 3 == 2 for k in kept) and any(k % 3 == 0 for k in kept) and any(k % 3 == 1 for k in kept)
    assert C.keep(cases.get("constant_one_300")["s"], cases.THR)[0].tolist() == [299]
    assert len(C.keep(cases.get("constant_half_300")["s"], cases.THR)[0]) == 300


def test_batches_sit_at_offsets_that_are_no_multiples_of_64():
    flat, items = cases.batch(cases.default_thr_names(cases.EMULATED_MAX))
    assert any(off % 64 for off, rows in items if rows) and np.isnan(flat[: items[0][0]]).all()
    for (off, rows), name in zip(items, cases.default_thr_names(cases.EMULATED_MAX)):
        assert np.array_equal(flat[off:off + rows * rows].reshape(rows, rows), cases.get(name)["s"])
    flat, items, mats = cases.many_small()
    assert len(items) > 128 and (items[:, 1] == 0).any()


def test_frame_filter_option_plumbing(monkeypatch):
    """--frame_filter defaults to host, a namespace without the attribute takes the host path, a bad value raises"""
    import types
    import extract_query_feats as E
    from src import query_pipeline, query_postprocess
    args = ["--models", "tiny:hf_vit:a.pth", "--pca_model", "p.pkl", "--input_file", "q.txt"]
    assert FRAME_FILTERS == ("host", "hip") and FRAME_THRESHOLD == cases.THR
    assert E.build_parser().parse_args(args).frame_filter == "host"
    assert E.build_parser().parse_args(args + ["--frame_filter", "hip"]).frame_filter == "hip"
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(args + ["--frame_filter", "gpu"])
    assert getattr(types.SimpleNamespace(), "frame_filter", "host") == "host"
    import inspect
    assert 'getattr(args, "frame_filter", "host")' in inspect.getsource(E.main)
    for fn in (query_postprocess.select_frames, query_postprocess.process_query_video, query_postprocess.process_query_group,
               query_pipeline.run_query_videos):
        assert inspect.signature(fn).parameters["frame_filter"].default == "host", fn.__name__
    feats = np.eye(4, dtype=np.float32)
    with pytest.raises(ValueError, match="frame_filter must be one of"):
        query_postprocess.select_frames(feats, frame_filter="gpu")
    with pytest.raises(ValueError, match="frame_filter must be one of"):
        query_postprocess.process_query_video("Q1", [feats], np.arange(4), 1.0, lambda x: x, 0, frame_filter="device")
    with pytest.raises(ValueError, match="frame_filter must be one of"):
        query_postprocess.process_query_group(["Q1"], [[feats]], [np.arange(4)], [1.0], lambda x: x, 0, frame_filter="")
    with pytest.raises(ValueError, match="frame_filter must be one of"):
        query_pipeline.run_query_videos([], [], lambda x: x, {}, "cpu", frame_filter="HIP")

    class NumpyOps:
        normalize = staticmethod(lambda x: x)
        self_similarity = staticmethod(lambda x: x @ x.T)

    # ops other than the library's own take only the host filter: refused before any device work
    with pytest.raises(ValueError, match="needs the library's own ops"):
        query_pipeline.run_query_videos([], [], lambda x: x, {}, "cpu", ops=NumpyOps, frame_filter="hip")
    with pytest.raises(ValueError, match="needs the library's own ops"):
        query_postprocess.select_frames(feats, ops=NumpyOps, frame_filter="hip")
    assert query_postprocess.select_frames(feats, ops=NumpyOps) == [0, 1, 2, 3]      # the default is today's code
    # above the entry's row limit: refused by name before anything touches a device
    from vsc_hip import ops
    assert ops.FRAME_FILTER_MAX_ROWS == 4096
    with pytest.raises(ValueError, match=r"video Q000777 has 4097 descriptor rows .* at most 4096"):
        query_postprocess.check_filter_rows("Q000777", 4097)
    query_postprocess.check_filter_rows("Q000777", 4096)
