"""Executable contract of vsc_uap_rank_f64 / vsc_uap_curve_f64 (include/vsc_hip.h) in numpy: one function per entry with the entry's
own outputs, `pairwise` -- numpy's summation tree written out, the documentation of the order the device sums in -- and `finish`,
what the caller does with the two sums in host floats.  rank + curve + finish reproduce the reference's average_precision
(VSC22-Descriptor-Track-1st/infer/vsc/metrics.py:423-494) bit for bit: tests/test_uap_cpu.py holds them against what the reference
itself returned (tests/golden/uap_device.json).

Why sums[0] runs over the REVERSED tie groups: sklearn's average_precision_score takes precision_recall_curve's arrays, which are
reversed (recall decreasing, then a final (1, 0) point), and returns max(0, -np.sum(np.diff(recall) * precision[:-1])).  Negation is
exact, so that is np.sum([t_G, ..., t_1]) with t_j = (R_j - R_{j-1}) P_j -- but np.sum is a pairwise sum over chunks of 8192, whose rounding depends
on where each term sits.  Summing t_1 .. t_G forward gives the same value only to the last bits."""
import numpy as np

TILE = 2048
SIGN = np.uint64(1 << 63)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def score_keys(scores):
    """order-preserving 64-bit image of -score: ascending key <=> descending score; -0.0 and +0.0 share a key"""
    u = bits(scores) ^ SIGN
    u = np.where(u == SIGN, np.uint64(0), u)
    return np.where((u >> np.uint64(63)).astype(bool), ~u, u | SIGN)


def rank(scores, pred_keys, gt_keys, key_bits=64):
    """-> perm int64 [n], scores_ranked float64 [n], correct uint8 [n], status int64 [4]"""
    scores = np.ascontiguousarray(scores, np.float64)
    pred_keys, gt_keys = np.asarray(pred_keys, np.uint64), np.asarray(gt_keys, np.uint64)
    assert key_bits == 64 or (not len(pred_keys) or int(pred_keys.max()) < 1 << key_bits) and (not len(gt_keys) or int(gt_keys.max()) < 1 << key_bits)
    perm = np.argsort(score_keys(scores), kind="stable").astype(np.int64)
    ranked = scores[perm]
    gt_sorted = np.sort(gt_keys)
    at = np.searchsorted(gt_sorted, pred_keys[perm])
    correct = np.zeros(len(scores), np.uint8)
    inside = at < len(gt_sorted)
    correct[inside] = gt_sorted[at[inside]] == pred_keys[perm][inside]
    status = np.array([np.count_nonzero(~np.isfinite(scores)), len(pred_keys) - len(np.unique(pred_keys)),
                       len(gt_keys) - len(np.unique(gt_keys)), int(correct.sum())], np.int64)
    return perm, ranked, correct, status


def _leaf(a):
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res = res + v
        return res
    r = [a[k] for k in range(8)]
    i = 8
    while i < n - n % 8:
        for k in range(8):
            r[k] = r[k] + a[i + k]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + v
    return res


def _tree(a):
    n = len(a)
    if n <= 128:
        return _leaf(a)
    n2 = n // 2
    n2 -= n2 % 8
    return _tree(a[:n2]) + _tree(a[n2:])


CHUNK = 8192          # numpy's reduction hands its inner loop at most np.getbufsize() elements at a time


def pairwise(a):
    """np.sum of a contiguous float64 vector, association by association: the reduction starts from the identity 0.0 and adds
    the pairwise sums of consecutive chunks of 8192 elements one after the other"""
    a = np.ascontiguousarray(a, np.float64).tolist()        # Python floats: the same IEEE doubles
    res = 0.0
    for i in range(0, len(a), CHUNK):
        res = res + _tree(a[i:i + CHUNK])
    return np.float64(res)


def curve(scores_ranked, correct, n_gt):
    """-> sums float64 [2], counts int64 [2] = {n_pos, n_groups}, curve float64 [3][n_pos] (the written prefix of the entry's [3][n])"""
    s = np.ascontiguousarray(scores_ranked, np.float64)
    c = np.asarray(correct).astype(bool)
    n = len(s)
    if n == 0:
        return np.zeros(2), np.zeros(2, np.int64), np.zeros((3, 0))
    cum = np.cumsum(c).astype(np.int64)
    n_pos = int(cum[-1])
    precision = cum / (np.arange(n, dtype=np.int64) + 1)
    recall = cum / np.int64(n_gt)
    last = np.nonzero(np.r_[s[1:] != s[:-1], True])[0].astype(np.int64)
    tps = cum[last]
    R = tps / np.int64(n_pos) if n_pos else np.zeros(len(last))
    P = tps / (last + 1)
    t = (R - np.r_[0.0, R[:-1]]) * P
    sums = np.array([pairwise(t[::-1]), pairwise(precision * c)], np.float64)
    idx = np.nonzero(c)[0]
    return sums, np.array([n_pos, len(last)], np.int64), np.stack([precision[idx], recall[idx], s[idx]])


def finish(sums, counts, n_gt):
    """-> (ap, simple_ap) in host floats: sklearn's max(0.0, .), drivendata's rescale by predicted / actual positives, and the
    division of the tie-blind sum by the number of ground-truth pairs"""
    n_pos = int(counts[0])
    ap = max(0.0, float(sums[0])) * (n_pos / int(n_gt))
    return float(ap), float(float(sums[1]) / int(n_gt))
