"""Seeded cases of the segment metric, shared by the CPU, emulated and GPU tests and by tests/golden/gen_segment_metric_golden.py
(which records the reference's own results on them).  A case is (name, gts, preds) with gts = [(query_id, ref_id, q_start, q_end,
r_start, r_end)] and preds = [(query_id, ref_id, score, q_start, q_end, r_start, r_end)]; ids are the csv's strings.  The shapes are
the smallest at which the kernels can go wrong: lists of 0, 1, 2, 63, 64, 65 and 130 predictions and of 0, 1, 64 and 65 ground
truths in one pair (the wave's chunks of 64), pairs with only one of the two, and the planted geometry below."""
import numpy as np


def _box(rs, span, grid=None, zero=0.0):
    """a box inside [0, span)^2; on a grid it may touch others and, with probability `zero`, have zero length on an axis"""
    out = []
    for _ in range(2):
        a, b = sorted(rs.uniform(0, span, 2))
        if grid:
            a, b = np.floor(a / grid) * grid, np.ceil(b / grid) * grid
            if rs.uniform() < zero:
                b = a
        out += [float(a), float(b)]
    return out


def _pair(rs, q, r, n_pred, n_gt, span, grid=None, decimals=None, zero=0.0):
    qid, rid = f"Q{q:06d}", f"R{r:06d}"
    gts = [(qid, rid, *_box(rs, span, grid)) for _ in range(n_gt)]
    preds = []
    for _ in range(n_pred):
        s = float(rs.uniform())
        preds.append((qid, rid, s if decimals is None else float(np.round(s, decimals)), *_box(rs, span, grid, zero)))
    return gts, preds


def _shuffled(rs, gts, preds):
    """pairs interleaved, as in a csv: the order of first appearance is not the order of the ids"""
    return [gts[i] for i in rs.permutation(len(gts))], [preds[i] for i in rs.permutation(len(preds))]


def _sizes(seed, shapes, span, **kw):
    rs = np.random.RandomState(seed)
    gts, preds = [], []
    for k, (n_pred, n_gt) in enumerate(shapes):
        g, p = _pair(rs, 100 + k, 200 + 7 * k, n_pred, n_gt, span, **kw)
        gts += g
        preds += p
    return _shuffled(rs, gts, preds)


def _planted():
    q, r = "Q000001", "R000001"
    gts = [
        (q, r, 0.0, 10.0, 0.0, 10.0),            # considered from the first prediction on
        (q, r, 40.0, 50.0, 40.0, 50.0),          # considered only by the LAST prediction of the pair
        (q, r, 20.0, 30.0, 80.0, 90.0),          # overlapped on the query axis only: never considered
        (q, r, 10.0, 12.0, 10.0, 12.0),          # touches the first ground truth: one component once both count
        ("Q000002", "R000002", 0.0, 5.0, 0.0, 5.0),       # a pair with ground truth and no predictions
        ("Q000003", "R000003", 1.0, 2.0, 1.0, 2.0),
        ("Q000005", "R000005", 0.0, 1e-170, 0.0, 1e-170),     # never considered: the product of the overlaps is 0.0
    ]
    preds = [
        (q, r, 0.9, 2.0, 4.0, 2.0, 4.0),
        (q, r, 0.9, 4.0, 6.0, 4.0, 6.0),         # touching the one before (start == end')
        (q, r, 0.8, 3.0, 3.0, 3.0, 5.0),         # zero length on the query axis, not the pair's first
        (q, r, 0.8, 2.0, 4.0, 2.0, 4.0),         # identical to the first
        (q, r, 0.7, 2.5, 3.5, 2.5, 3.5),         # nested
        (q, r, 0.7, 20.0, 30.0, 20.0, 30.0),     # overlaps the third ground truth on the query axis only
        (q, r, 0.6, 11.0, 11.5, 11.0, 11.5),     # makes the touching ground truth count
        (q, r, 0.5, 6.0, 20.0, 6.0, 20.0),       # bridges components
        (q, r, 0.0, 45.0, 46.0, 45.0, 46.0),     # the late one; its score 0.0 ties with -0.0 of another pair
        ("Q000003", "R000003", -0.0, 1.5, 3.0, 1.5, 3.0),
        ("Q000003", "R000003", 0.9, 0.0, 1.0, 0.0, 1.0),      # tied across pairs with the first two; touches its ground truth, no area
        ("Q000004", "R000004", 0.8, 0.0, 9.0, 0.0, 9.0),      # a pair with predictions and no ground truth
        ("Q000004", "R000004", 0.75, 1e-200, 2e-200, 1e-200, 2e-200),
        ("Q000005", "R000005", 0.65, 0.0, 1.0, 0.0, 1.0),      # overlaps its ground truth by 1e-170 on both axes: the area underflows
    ]
    return gts, preds


def cases():
    """[(name, gts, preds)], the same lists on every call"""
    out = [("sizes_continuous", *_sizes(1, [(0, 1), (1, 0), (2, 1), (63, 64), (64, 65), (65, 1), (130, 65), (1, 1), (0, 2)], 300.0))]
    out.append(("sizes_grid_quarter", *_sizes(2, [(65, 64), (2, 65), (64, 1), (1, 64), (130, 0), (63, 2)], 40.0, grid=0.25, decimals=1,
                                              zero=0.15)))
    out.append(("many_pairs_ties2", *_sizes(3, [(n % 13, (n * 5) % 4) for n in range(40)], 60.0, decimals=2)))
    out.append(("many_pairs_grid_half", *_sizes(4, [((n * 7) % 17, n % 3) for n in range(30)], 12.0, grid=0.5, decimals=1, zero=0.2)))
    out.append(("planted", *_planted()))
    gts, preds = _sizes(5, [(3, 2), (0, 4)], 50.0)
    out.append(("no_predictions", gts, []))
    out.append(("zde_no_ground_truth", [], _sizes(6, [(5, 0), (2, 0)], 50.0)[1]))
    g = [("Q000001", "R000001", 0.0, 4.0, 0.0, 4.0)]
    out.append(("zde_first_group_covers_nothing", g, [("Q000001", "R000001", 0.9, 1.0, 1.0, 1.0, 3.0), ("Q000001", "R000001", 0.5, 1.0, 2.0, 1.0, 3.0)]))
    out.append(("zde_ground_truth_of_zero_length", [("Q000001", "R000001", 2.0, 2.0, 0.0, 4.0)], [("Q000001", "R000001", 0.9, 1.0, 3.0, 1.0, 3.0)]))
    return out


def workload(seed, n_pairs, per_pair, n_gt, span=1000.0, size=20.0, decimals=3):
    """(gts, preds) of the repeat test and of tools/micro/segment_metric.py: short boxes in a long video, so that a pair keeps many
    components; scores rounded to `decimals` (tie groups)"""
    rs = np.random.RandomState(seed)
    gts, preds = [], []
    for p in range(n_pairs):
        q, r = f"Q{p:06d}", f"R{p:06d}"
        for _ in range(n_gt):
            a, n = rs.uniform(0, span, 2), rs.uniform(0, 3 * size, 2)
            gts.append((q, r, float(a[0]), float(a[0] + n[0]), float(a[1]), float(a[1] + n[1])))
        for _ in range(per_pair):
            a, n = rs.uniform(0, span, 2), rs.uniform(0, size, 2)
            preds.append((q, r, float(np.round(rs.uniform(), decimals)), float(a[0]), float(a[0] + n[0]), float(a[1]), float(a[1] + n[1])))
    return gts, preds
