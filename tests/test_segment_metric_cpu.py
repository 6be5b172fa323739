"""The segment metric without a GPU: the executable contract (tests/segment_metric_contract.py) against the reference's recorded
results (tests/golden/segment_metric.json, written by tests/golden/gen_segment_metric_golden.py from the reference's own
match_metric), its decomposed form against its naive form, and the host side of vsc_hip/segment_metric.py -- packing, the final
arithmetic, the refusals -- against both.  The kernels themselves: tests/test_segment_metric_emulated.py (here) and
tests/test_gpu_segment_metric.py (on the device)."""
import json
import os

import numpy as np
import pytest

import segment_metric_cases as cases
import segment_metric_contract as C
from vsc.metrics import Match
from vsc_hip import _lib, segment_metric

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = {r["name"]: r for r in json.load(open(os.path.join(HERE, "golden", "segment_metric.json")))}
CASES = {name: (gts, preds) for name, gts, preds in cases.cases()}


def as_matches(gts, preds):
    return ([Match(q, r, 1.0, *box) for q, r, *box in gts], [Match(q, r, s, *box) for q, r, s, *box in preds])


def assert_golden(name, result):
    """result = (ap, precisions, recalls, scores): the reference's bits"""
    g = GOLDEN[name]
    assert float(result[0]).hex() == g["ap"], (name, result[0], float.fromhex(g["ap"]))
    for got, field in zip(result[1:], ("precisions", "recalls", "scores")):
        assert [float(v).hex() for v in got] == g[field], (name, field)


def test_golden_records_the_cases_of_this_tree():
    assert list(GOLDEN) == list(CASES)
    for name, (gts, preds) in CASES.items():
        assert GOLDEN[name]["gts"] == [list(g) for g in gts] and GOLDEN[name]["preds"] == [list(p) for p in preds], name
    assert sum(len(g) + len(p) for g, p in CASES.values()) < 5000 and os.path.getsize(os.path.join(HERE, "golden", "segment_metric.json")) < 300 << 10
    sizes_p = {sum(1 for p in preds if p[:2] == key) for gts, preds in CASES.values() for key in {p[:2] for p in preds} | {g[:2] for g in gts}}
    sizes_g = {sum(1 for g in gts if g[:2] == key) for gts, preds in CASES.values() for key in {p[:2] for p in preds} | {g[:2] for g in gts}}
    assert sizes_p >= {0, 1, 2, 63, 64, 65, 130} and sizes_g >= {0, 1, 64, 65}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("form", ["naive", "decomposed"])
def test_contract_equals_the_reference_bit_for_bit(name, form):
    fn = C.match_metric if form == "naive" else C.match_metric_decomposed
    if GOLDEN[name].get("raises"):
        with pytest.raises(ZeroDivisionError):
            fn(*CASES[name])
    else:
        assert_golden(name, fn(*CASES[name]))


@pytest.mark.parametrize("name", list(CASES))
def test_host_packing_equals_the_contract(name):
    """pair order (ground-truth pairs first, by first appearance), the stable descending sort, the CSR tables, the tie groups"""
    gts, preds = CASES[name]
    want, got = C.pack(gts, preds), segment_metric.pack(*as_matches(gts, preds))
    for field in ("pred_boxes", "pred_ptr", "pred_rank", "gt_boxes", "gt_ptr", "group_ends", "group_scores"):
        a, b = getattr(got, field), want[field]
        assert a.dtype == b.dtype and a.shape == b.shape and a.flags.c_contiguous, (field, a.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), field
    assert (got.n_pairs, got.n_gt_pairs) == (want["n_pairs"], want["n_gt_pairs"])


def test_host_packing_on_a_case_small_enough_to_read():
    G = [Match("Q2", "R2", 1.0, 0, 1, 0, 1), Match("Q1", "R1", 1.0, 0, 2, 0, 2), Match("Q2", "R2", 1.0, 5, 6, 5, 6)]
    P = [Match("Q3", "R3", 0.5, 0, 1, 0, 1), Match("Q1", "R1", 0.9, 1, 2, 1, 2), Match("Q2", "R2", 0.5, 2, 3, 2, 3), Match("Q1", "R1", -0.0, 3, 4, 3, 4),
         Match("Q3", "R3", 0.0, 4, 5, 4, 5), Match("Q1", "R1", 0.5, 6, 7, 6, 7)]
    k = segment_metric.pack(G, P)
    assert (k.n_pairs, k.n_gt_pairs) == (3, 2)                                    # Q2 (first in the ground truth), Q1, then Q3
    assert k.pred_boxes[:, 0].tolist() == [1, 0, 2, 6, 3, 4]                      # 0.9 | 0.5 0.5 0.5 in file order | -0.0 0.0 in file order
    assert k.pred_ptr.tolist() == [0, 1, 4, 6] and k.pred_rank.tolist() == [2, 0, 3, 4, 1, 5]
    assert k.gt_ptr.tolist() == [0, 2, 3, 3] and k.gt_boxes[:, 0].tolist() == [0, 5, 0]
    assert k.group_ends.tolist() == [0, 3, 5] and [float(s).hex() for s in k.group_scores] == [0.9.hex(), 0.5.hex(), (-0.0).hex()]


@pytest.mark.parametrize("name", list(CASES))
def test_host_arithmetic_on_the_contract_kernels_equals_the_reference(name):
    """vsc_hip.segment_metric.pack + finish around the contract's deltas / scan: everything of the product but the two kernels"""
    k = segment_metric.pack(*as_matches(*CASES[name]))

    def run():
        if not len(k.pred_boxes):
            return 0.0, [], [], []
        d, gt_len = C.deltas(k.pred_boxes, k.pred_ptr, k.pred_rank, k.gt_boxes, k.gt_ptr, k.n_pairs)
        totals = C.scan(gt_len[:k.n_gt_pairs], [k.n_gt_pairs - 1])[0] if k.n_gt_pairs else (0.0, 0.0)
        return segment_metric.finish(C.scan(d, k.group_ends), totals, k.group_scores)
    if GOLDEN[name].get("raises"):
        with pytest.raises(ZeroDivisionError):
            run()
    else:
        assert_golden(name, run())


def test_refusals_come_before_any_device_work():
    g = [Match("Q1", "R1", 1.0, 0.0, 1.0, 0.0, 1.0)]
    ok = Match("Q1", "R1", 0.5, 0.0, 1.0, 0.0, 1.0)
    for bad in (ok._replace(score=float("nan")), ok._replace(score=float("inf")), ok._replace(query_end=float("nan")),
                ok._replace(ref_start=float("-inf")), ok._replace(query_start=2.0), ok._replace(ref_end=-1.0)):
        with pytest.raises(ValueError):
            segment_metric.pack(g, [ok, bad])
    with pytest.raises(ValueError):
        segment_metric.pack([g[0]._replace(query_end=-3.0)], [ok])
    with pytest.raises(ValueError):
        segment_metric.pack([g[0]._replace(ref_end=float("nan"))], [ok])
    segment_metric.pack(g, [ok, ok._replace(query_end=0.0)])              # zero length is legal


def test_without_a_device_the_metric_raises(tmp_path):
    import torch
    if torch.cuda.is_available():
        return                                        # with a device the metric runs: tests/test_gpu_segment_metric.py
    from vsc.metrics import evaluate_matching_track, match_metric
    G, P = as_matches(*CASES["planted"])
    with pytest.raises(_lib.HipPathUnavailable):
        match_metric(G, P)
    Match.write_csv(G, tmp_path / "gt.csv")
    Match.write_csv(P, tmp_path / "pred.csv")
    with pytest.raises(_lib.HipPathUnavailable):
        evaluate_matching_track(str(tmp_path / "gt.csv"), str(tmp_path / "pred.csv"))


@pytest.mark.parametrize("name", list(CASES))
def test_csv_round_trip_scores_as_the_lists(tmp_path, monkeypatch, name):
    """evaluate_matching_track around the contract's kernels: Match.write_csv + the correctly rounded read give back every bit, so
    the file scores as the reference scores the lists"""
    from vsc.metrics import evaluate_matching_track

    def on_the_contract(gts, preds):
        k = segment_metric.pack(gts, preds)
        if not len(preds):
            return 0.0, [], [], []
        d, gt_len = C.deltas(k.pred_boxes, k.pred_ptr, k.pred_rank, k.gt_boxes, k.gt_ptr, k.n_pairs)
        totals = C.scan(gt_len[:k.n_gt_pairs], [k.n_gt_pairs - 1])[0] if k.n_gt_pairs else (0.0, 0.0)
        return segment_metric.finish(C.scan(d, k.group_ends), totals, k.group_scores)
    monkeypatch.setattr(segment_metric, "segment_ap", on_the_contract)
    G, P = as_matches(*CASES[name])
    Match.write_csv(G, tmp_path / "gt.csv")
    Match.write_csv(P, tmp_path / "pred.csv")
    if GOLDEN[name].get("raises"):
        with pytest.raises(ZeroDivisionError):
            evaluate_matching_track(str(tmp_path / "gt.csv"), str(tmp_path / "pred.csv"))
        return
    got = evaluate_matching_track(str(tmp_path / "gt.csv"), str(tmp_path / "pred.csv"))
    assert_golden(name, (got.segment_ap.ap, got.segment_ap.pr_curve.precisions, got.segment_ap.pr_curve.recalls, got.segment_ap.pr_curve.scores))
    assert 0.0 <= got.pairwise_micro_ap.ap <= 1.0


def test_entry_points_take_the_option():
    from vsc.baseline import sscd_baseline
    base = ["--query_features", "q.npz", "--ref_features", "r.npz", "--output_path", "out"]
    assert sscd_baseline.build_parser().parse_args(base).segment_metric == "none"
    assert sscd_baseline.build_parser().parse_args(base + ["--segment_metric", "hip"]).segment_metric == "hip"
    with pytest.raises(SystemExit):
        sscd_baseline.build_parser().parse_args(base + ["--segment_metric", "cpu"])
