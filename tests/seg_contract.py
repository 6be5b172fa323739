"""Executable statement of the segment-extraction contract (vsc_match_segments_f32, include/vsc_hip.h): connected
components + RANSAC localisation of one probability map at one threshold, numpy only.

It is sklearn 1.7's RANSACRegressor loop (the reference's utils.py:76-117) with the trial phase in exact integer
arithmetic: a point whose residual equals the residual threshold exactly is an inlier, where sklearn's float64 lstsq puts
it at 2 +- 1e-14 and decides by rounding noise.  `segments` returns the rows and a report with the margin (the smallest
distance of any float64 decision from its boundary), whether any executed trial met a boundary point, and the group sizes.
"""
import math

import numpy as np

MIN_COMPONENT = 10
MAX_TRIALS, SEED, RESIDUAL = 200, 2023, 2
EPSILON = float(np.spacing(1))
NOM = 1 - 0.99                       # sklearn's `1 - stop_probability`
KNIFE_EDGE = 1e-9


def components8(mask):
    """-> int array: for every masked pixel the raster index of the first pixel of its 8-connected component, -1 elsewhere."""
    h, w = mask.shape
    big = h * w
    lab = np.where(mask, np.arange(big, dtype=np.int64).reshape(h, w), big)
    while True:
        pad = np.full((h + 2, w + 2), big, np.int64)
        pad[1:-1, 1:-1] = lab
        new = lab
        for di in range(3):
            for dj in range(3):
                new = np.minimum(new, pad[di:di + h, dj:dj + w])
        new = np.where(mask, new, big)
        flat = np.append(new.reshape(-1), big)
        for _ in range(2):                   # pointer jumping
            flat = flat[flat]
        new = flat[:-1].reshape(h, w)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1)


def groups(prob, threshold):
    """Point sets of one map, each (x, y) in raster order: one per large component (its pixels plus all loose pixels), in
    raster order of the components' first pixels; all loose pixels alone when there is no large component."""
    prob = np.asarray(prob, dtype=np.float32)
    if prob.size == 0:
        return []
    mask = prob > np.float32(threshold)
    lab = components8(mask)
    roots, counts = np.unique(lab[mask], return_counts=True)
    large = roots[counts > MIN_COMPONENT]
    loose = mask & ~np.isin(lab, large)
    if len(large) == 0:
        return [np.where(loose)]
    return [np.where((lab == r) | loose) for r in large]


def subsets(n):
    """The 2-subsets of range(n) that sklearn.utils.random.sample_without_replacement(n, 2, random_state=rs) returns on
    successive calls with rs = RandomState(2023): a generator of (i1, i2)."""
    rs = np.random.RandomState(SEED)
    while True:
        if n < 200:                          # ratio 2 / n > 0.01: a permutation's head
            p = rs.permutation(n)
            yield int(p[0]), int(p[1])
        else:                                # tracking selection
            a = int(rs.randint(n))
            b = int(rs.randint(n))
            while b == a:
                b = int(rs.randint(n))
            yield a, b


def dynamic_max_trials(k, n):
    """-> (trials, value whose ceil it is); sklearn's _dynamic_max_trials with min_samples = 2, probability 0.99."""
    ratio = k / float(n)
    denom = max(EPSILON, 1 - ratio * ratio)
    if denom == 1:
        return math.inf, math.inf
    v = math.log(NOM) / math.log(denom)
    return abs(float(math.ceil(v))), v


class _Margin:
    def __init__(self):
        self.value = math.inf

    def see(self, distance):
        d = abs(float(distance))
        if d < self.value:
            self.value = d


def _trial_model(x, y, wgt, i1, i2, margin):
    """-> (inlier mask, R^2, boundary point met, model) of the line through points i1, i2."""
    x1, y1, x2, y2 = int(x[i1]), int(y[i1]), int(x[i2]), int(y[i2])
    dx, dy = x2 - x1, y2 - y1
    if dx != 0:
        r = (y - y1) * dx - dy * (x - x1)                   # int64, exact
        a, lim = np.abs(r), 2 * abs(dx)
        inl = a <= lim
        boundary = bool((a == lim).any())
        k = int(inl.sum())
        sy, syy, aa = int(y[inl].sum()), int((y[inl] * y[inl]).sum()), int((r[inl] * r[inl]).sum())
        b = k * syy - sy * sy
        if b == 0:
            r2 = 1.0 if aa == 0 else 0.0
        else:
            r2 = 1.0 - (float(aa) * float(k)) / (float(dx * dx) * float(b))
        return inl, r2, boundary, ("line", x1, y1, dx, dy)
    if y1 == y2:
        c = float(y1)
    else:
        w1, w2 = float(wgt[i1]), float(wgt[i2])
        c = (w1 * y1 + w2 * y2) / (w1 + w2)
    d = np.abs(y.astype(np.float64) - c)
    inl = d <= 2.0
    boundary = bool((d == 2.0).any())
    if y1 != y2:
        margin.see(np.abs(d - 2.0).min())
    k = int(inl.sum())
    sy, syy = int(y[inl].sum()), int((y[inl] * y[inl]).sum())
    b = k * syy - sy * sy
    res = (float(syy) - (2.0 * c) * float(sy)) + (float(k) * c) * c
    if b == 0:
        r2 = 1.0 if res == 0.0 else 0.0
    else:
        r2 = 1.0 - (res * float(k)) / float(b)
    return inl, r2, boundary, ("const", c)


def fit_group(prob, x, y, std_ratio, margin=None, report=None):
    """One group's points (raster order) -> [x_first, y_first, x_last, y_last, score] or None."""
    margin = margin or _Margin()
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    n = len(x)
    if len(np.unique(x)) <= 3:
        return None
    p32 = prob[x, y].astype(np.float32)
    wgt = (p32 * p32).astype(np.float64)                    # np.square of an fp32 map stays fp32
    best_k, best_r2, best_inl = 1, -math.inf, None
    max_trials, trials = MAX_TRIALS, 0
    draw = subsets(n)
    boundary_seen = False
    while trials < max_trials:
        trials += 1
        i1, i2 = next(draw)
        inl, r2, boundary, _ = _trial_model(x, y, wgt, i1, i2, margin)
        boundary_seen |= boundary
        k = int(inl.sum())
        if k < best_k:
            continue
        if k == best_k and r2 != best_r2 and best_inl is not None:
            margin.see(r2 - best_r2)
        if k == best_k and r2 < best_r2:
            continue
        best_k, best_r2, best_inl = k, r2, inl
        t, v = dynamic_max_trials(k, n)
        if v <= max_trials + 1:
            margin.see(min(v - (math.ceil(v) - 1), math.ceil(v) - v) if v <= max_trials else v - max_trials)
        max_trials = min(max_trials, t)
    if report is not None:
        report["boundary"] = report.get("boundary", False) or boundary_seen
        report.setdefault("group_sizes", []).append(n)
        report.setdefault("trials", []).append(trials)
    if best_inl is None:
        return None
    # final model: float64 closed-form weighted least squares over the best inliers
    xi, yi, wi = x[best_inl].astype(np.float64), y[best_inl].astype(np.float64), wgt[best_inl]
    sw = wi.sum()
    xm, ym = (wi * xi).sum() / sw, (wi * yi).sum() / sw
    sxx, sxy = (wi * (xi - xm) * (xi - xm)).sum(), (wi * (xi - xm) * (yi - ym)).sum()
    slope = sxy / sxx if sxx > 0 else 0.0
    icpt = ym - slope * xm
    margin.see(slope)
    if slope <= 0:
        return None
    res = np.abs(y.astype(np.float64) - (slope * x.astype(np.float64) + icpt))
    margin.see(np.abs(res - 1.0).min())
    near = res < 1
    xs, ys = x[near], y[near]
    if not (near.sum() > 5 and len(np.unique(xs)) > 3 and len(np.unique(ys)) > 3):
        return None
    top = prob[xs, ys].astype(np.float64)
    mean = top.sum() / len(top)
    std = math.sqrt(((top - mean) * (top - mean)).sum() / len(top))
    s = max(1.0 / slope, slope)
    score = (float(top.max()) - std * float(std_ratio)) - abs(s - 1.0) / 10.0
    return [int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]), score]


def segments(prob, threshold, std_ratio):
    """One map at one threshold -> (rows [[x_first, y_first, x_last, y_last, score], ...] in group order, report) with
    report = dict(margin, boundary, group_sizes, trials)."""
    prob = np.asarray(prob, dtype=np.float32)
    margin, report = _Margin(), dict(boundary=False, group_sizes=[], trials=[])
    rows = []
    for x, y in groups(prob, threshold):
        seg = fit_group(prob, x, y, std_ratio, margin, report)
        if seg is not None:
            rows.append(seg)
    report["margin"] = margin.value
    return rows, report


def matching_result(res_list, threshold, std_ratio):
    """generate_matching_result's row structure under the contract."""
    out = []
    for qid, rid, prob, _ in res_list:
        for seg in segments(prob, threshold, std_ratio)[0]:
            out.append([qid, rid, *seg])
    return out
