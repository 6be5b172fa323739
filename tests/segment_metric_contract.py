"""The matching-track segment AP as an executable contract, in plain Python / numpy (include/vsc_hip.h: vsc_segment_metric_*;
the reference is VSC22-Matching-Track-1st/infer/vsc/metrics.py:120-383, `match_metric`).  Two forms:

  naive        match_metric(gts, preds): per prediction, rebuild and merge every interval list of its video pair, as the metric
               is defined.  Quadratic in the predictions of a pair.
  decomposed   deltas(...) and scan(...), with the operands of the two device entries, + finish(...), the host arithmetic.

Every float is a Python float / np.float64 and every sum is written in the order the contract fixes, so both forms are held to
the reference's recorded results (tests/golden/segment_metric.json) and to each other bit for bit.  A box is
(q_start, q_end, r_start, r_end); a ground truth is (query_id, ref_id, *box), a prediction (query_id, ref_id, score, *box)."""
import math

import numpy as np


def merged(intervals):
    """connected components under start <= current_end (touching intervals merge), ascending"""
    out = []
    for s, e in sorted(intervals):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def length(components):
    acc = 0.0
    for s, e in components:
        acc = acc + (e - s)
    return acc


def overlaps(a, b):
    q = max(min(a[1], b[1]) - max(a[0], b[0]), 0.0)
    r = max(min(a[3], b[3]) - max(a[2], b[2]), 0.0)
    return abs(q * r) > 0.0


def pair_state(pred_boxes, gt_boxes):
    """{I_q, I_r, T_q, T_r} of one video pair after these predictions, everything rebuilt (VideoPair.add_prediction)"""
    considered = [b for b in gt_boxes if any(overlaps(b, p) for p in pred_boxes)]
    out = [0.0] * 4
    for axis in (0, 1):
        u = merged([(b[2 * axis], b[2 * axis + 1]) for b in pred_boxes])
        g = merged([(b[2 * axis], b[2 * axis + 1]) for b in considered])
        t = length(u)
        out[axis], out[2 + axis] = (t + length(g)) - length(merged([tuple(c) for c in u + g])), t
    return out


def pair_deltas(pred_boxes, gt_boxes):
    """One video pair, predictions in rank order: [n][4] = {dI_q, dI_r, dT_q, dT_r} and the pair's gt_len [2].  The merged sets
    are carried from one prediction to the next: the merged set of a merged set's components and further intervals is the merged
    set of everything (components and their bounds involve no rounding); the lengths are summed anew, left to right, every time."""
    pred_boxes, gt_boxes = [[float(x) for x in b] for b in pred_boxes], [[float(x) for x in b] for b in gt_boxes]
    out = np.zeros((len(pred_boxes), 4), np.float64)
    considered = [False] * len(gt_boxes)
    u, g, w = [[], []], [[], []], [[], []]
    i_prev, t_prev = [0.0, 0.0], [0.0, 0.0]
    for k, pred in enumerate(pred_boxes):
        fresh = [gt for j, gt in enumerate(gt_boxes) if not considered[j] and overlaps(gt, pred)]
        considered = [c or overlaps(gt, pred) for c, gt in zip(considered, gt_boxes)]
        for axis in (0, 1):
            new_p, new_g = [(pred[2 * axis], pred[2 * axis + 1])], [(b[2 * axis], b[2 * axis + 1]) for b in fresh]
            u[axis] = merged([tuple(c) for c in u[axis]] + new_p)
            g[axis] = merged([tuple(c) for c in g[axis]] + new_g)
            w[axis] = merged([tuple(c) for c in w[axis]] + new_p + new_g)
            t = length(u[axis])
            i = (t + length(g[axis])) - length(w[axis])
            out[k, axis], out[k, 2 + axis] = i - i_prev[axis], t - t_prev[axis]
            i_prev[axis], t_prev[axis] = i, t
    gt_len = [length(merged([(b[2 * axis], b[2 * axis + 1]) for b in gt_boxes])) for axis in (0, 1)]
    return out, gt_len


def deltas(pred_boxes, pred_ptr, pred_rank, gt_boxes, gt_ptr, n_pairs):
    """vsc_segment_metric_deltas_f64: (deltas [P][4] at the predictions' ranks, gt_len [n_pairs][2]).  n_preds == 0 writes nothing."""
    pred_boxes, gt_boxes = np.asarray(pred_boxes, np.float64).reshape(-1, 4), np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    out, gt_len = np.zeros((len(pred_boxes), 4), np.float64), np.zeros((n_pairs, 2), np.float64)
    for p in range(n_pairs if len(pred_boxes) else 0):
        ranks = np.asarray(pred_rank[pred_ptr[p]:pred_ptr[p + 1]], np.int64)
        d, gl = pair_deltas(pred_boxes[ranks], gt_boxes[gt_ptr[p]:gt_ptr[p + 1]])
        out[ranks] = d
        gt_len[p] = gl
    return out, gt_len


def scan(rows, ends):
    """vsc_segment_metric_scan_f64: out[e][c] = ((0.0 + rows[0][c]) + rows[1][c]) + ... + rows[ends[e]][c], strictly left to right"""
    rows = np.asarray(rows, np.float64)
    rows = rows.reshape(len(rows), -1)
    out = np.zeros((len(ends), rows.shape[1]), np.float64)
    acc, e = [0.0] * rows.shape[1], 0
    for i in range(len(rows)):
        acc = [a + float(x) for a, x in zip(acc, rows[i])]
        while e < len(ends) and ends[e] == i:
            out[e] = acc
            e += 1
    return out


def finish(groups, totals, group_scores):
    """The host arithmetic (metrics.py:338-383): groups [n_groups][4] = running {I_q, I_r, T_q, T_r} at the end of every tie
    group, totals [2] = ground-truth lengths.  Returns (ap, precisions, recalls, scores); ZeroDivisionError as the reference."""
    recall = metric = 0.0
    curve = ([], [], [])
    gq, gr = float(totals[0]), float(totals[1])
    for (iq, ir, tq, tr), score in zip(np.asarray(groups, np.float64).reshape(-1, 4).tolist(), group_scores):
        new_recall = math.sqrt((iq / gq) * (ir / gr))
        precision = math.sqrt((iq / tq) * (ir / tr))
        delta = new_recall - recall
        metric += precision * delta
        recall = new_recall
        if delta > 0:
            for lst, v in zip(curve, (precision, recall, float(score))):
                lst.append(v)
    return (metric,) + curve


def pack(gts, preds):
    """The operands of the two entries from lists of ground truths and predictions: pairs that have ground truth first, in order
    of first appearance, then the other pairs in order of first appearance among the predictions; rank = position in the stable
    descending sort by score; a tie group is a run of == scores."""
    pair_of = {}
    for m in gts:
        pair_of.setdefault((m[0], m[1]), len(pair_of))
    n_gt_pairs = len(pair_of)
    for m in preds:
        pair_of.setdefault((m[0], m[1]), len(pair_of))
    n_pairs = len(pair_of)
    order = sorted(range(len(preds)), key=lambda i: -preds[i][2])                 # sorted() is stable
    scores = [preds[i][2] for i in order]
    by_pair_p, by_pair_g = [[] for _ in range(n_pairs)], [[] for _ in range(n_pairs)]
    for rank, i in enumerate(order):
        by_pair_p[pair_of[(preds[i][0], preds[i][1])]].append(rank)
    for m in gts:
        by_pair_g[pair_of[(m[0], m[1])]].append(m[2:6])
    ends = [i for i in range(len(scores)) if i + 1 == len(scores) or scores[i] != scores[i + 1]]
    starts = [0] + [e + 1 for e in ends[:-1]] if ends else []
    return dict(
        pred_boxes=np.array([preds[i][3:7] for i in order], np.float64).reshape(-1, 4),
        pred_ptr=np.cumsum([0] + [len(x) for x in by_pair_p]).astype(np.int64),
        pred_rank=np.array([r for x in by_pair_p for r in x], np.int64),
        gt_boxes=np.array([b for x in by_pair_g for b in x], np.float64).reshape(-1, 4),
        gt_ptr=np.cumsum([0] + [len(x) for x in by_pair_g]).astype(np.int64),
        n_pairs=n_pairs, n_gt_pairs=n_gt_pairs, group_ends=np.array(ends, np.int64),
        group_scores=np.array([scores[s] for s in starts], np.float64))


def match_metric_decomposed(gts, preds):
    k = pack(gts, preds)
    if not len(preds):
        return 0.0, [], [], []
    d, gt_len = deltas(k["pred_boxes"], k["pred_ptr"], k["pred_rank"], k["gt_boxes"], k["gt_ptr"], k["n_pairs"])
    groups = scan(d, k["group_ends"])
    totals = scan(gt_len[:k["n_gt_pairs"]], [k["n_gt_pairs"] - 1])[0] if k["n_gt_pairs"] else [0.0, 0.0]
    return finish(groups, totals, k["group_scores"])


def match_metric(gts, preds):
    """The naive form: the metric as it is defined, one prediction at a time in score order over Python dicts."""
    preds = sorted(preds, key=lambda m: m[2], reverse=True)
    gt_of = {}
    for m in gts:
        gt_of.setdefault((m[0], m[1]), []).append(tuple(float(x) for x in m[2:6]))
    totals = [0.0, 0.0]
    for boxes in gt_of.values():
        for axis in (0, 1):
            totals[axis] += length(merged([(b[2 * axis], b[2 * axis + 1]) for b in boxes]))
    seen, prev = {}, {}
    running = [0.0] * 4
    groups, group_scores = [], []
    for i, m in enumerate(preds):
        key = (m[0], m[1])
        seen.setdefault(key, []).append(tuple(float(x) for x in m[3:7]))
        now = pair_state(seen[key], gt_of.get(key, []))            # the pair rebuilt from nothing
        running = [a + (x - y) for a, x, y in zip(running, now, prev.get(key, [0.0] * 4))]
        prev[key] = now
        if i + 1 == len(preds) or preds[i + 1][2] != m[2]:
            groups.append(list(running))
        if i == 0 or preds[i - 1][2] != m[2]:
            group_scores.append(m[2])
    return finish(groups, totals, group_scores)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)
