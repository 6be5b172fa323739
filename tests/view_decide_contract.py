"""Executable contract of vsc_view_decide_f64 (include/vsc_hip.h, csrc/view_decide.hip): the view decisions of
src/image_preprocess.py (``decide_views``) with every summation order, promotion and rounding written out, and the explicit region
stack of the kernel instead of recursion.  No np.mean / np.quantile / np.median anywhere: the only numpy used is elementwise
arithmetic (which rounds every element like the scalar operation) so that the orders below can run over many rows at once.

The orders are numpy's, checked against numpy 2.2.6 (tests/test_view_decide_cpu.py compares the bits on every case):
  a.mean(1)   per row numpy's pairwise sum (``pairwise``), then one division
  a.mean(0)   one add chain per column in row order from 0.0, then one division; a region ONE column wide is the exception:
              numpy drops that axis, the reduction becomes its inner loop and the column is summed pairwise
  a.mean()    the region flattened row-major, cut into chunks of 8192, pairwise inside a chunk, the chunk sums chained from 0.0
  quantile    pos = (N - 1) * 0.95, lo = floor(pos), t = pos - lo, A, B the order statistics lo, min(lo + 1, N - 1):
              A + (B - A) t below t = 0.5, else B - (B - A)(1 - t); A and B come from the (m + 1)-bin histogram of the counts
  median      the middle order statistic, or (a + b) / 2 of the two middle ones
  edges       a 0/1 float32 array: sums are integer counts, a mean is float32(count) / float32(size)
float32 where numpy 2 promotes a Python literal to the array's type: 0.125 + edge_p.mean(), 0.45 + edges.mean(),
edge_p.mean() < 0.0225, edge_at > 0.65."""
from __future__ import annotations

import math

import numpy as np

NUMPY_CHECKED = "2.2.6"
MIN_FRAMES, MIN_SIDE, MIN_VIEW, GAP = 5, 20, 80, 5
CHUNK = 8192            # elements of a flattened region per pairwise sum
STACK = 64              # pending regions the kernel holds (VSC_VIEW_DECIDE_STACK)
MAX_VIEWS = 64          # VSC_VIEW_DECIDE_MAX_VIEWS
F32 = np.float32


def pairwise(a):
    """numpy's pairwise sum over the last axis of ``a`` (float64 or float32), in the array's own type"""
    n = a.shape[-1]
    if n < 8:
        res = np.zeros(a.shape[:-1], a.dtype)
        for i in range(n):
            res = res + a[..., i]
        return res
    if n <= 128:
        r = [a[..., k] for k in range(8)]
        full = n - n % 8
        for i in range(8, full, 8):
            for k in range(8):
                r[k] = r[k] + a[..., i + k]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(full, n):
            res = res + a[..., i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[..., :n2]) + pairwise(a[..., n2:])


def flat_sum(a):
    """a.sum() of a 2-D float64 region: chunks of 8192 of the row-major order, pairwise inside, chained from 0.0"""
    flat = np.ascontiguousarray(a).reshape(-1)
    total = np.float64(0.0)
    whole = flat.size // CHUNK
    if whole:
        for s in pairwise(flat[:whole * CHUNK].reshape(whole, CHUNK)):
            total = total + s
    if flat.size % CHUNK:
        total = total + pairwise(flat[whole * CHUNK:])
    return total


def row_means(a):
    return pairwise(a) / a.shape[1]


def col_means(a):
    if a.shape[1] == 1:         # numpy drops the axis of one column: the reduction becomes the inner loop, a pairwise sum
        return pairwise(np.ascontiguousarray(a.T)) / a.shape[0]
    acc = np.zeros(a.shape[1], np.float64)
    for r in range(a.shape[0]):
        acc = acc + a[r]
    return acc / a.shape[0]


def mean1d(p):
    """p.mean() of a 1-D slice in p's own type; an empty slice gives NaN"""
    if p.size == 0:
        return p.dtype.type(np.nan)
    return p.dtype.type(pairwise(p) / p.dtype.type(p.size))


def median(p):
    n = p.size
    if n == 0:
        return np.float64(np.nan)
    order = sorted(p.tolist())
    if n % 2:
        return np.float64(order[n // 2])
    return (np.float64(order[n // 2 - 1]) + np.float64(order[n // 2])) / np.float64(2.0)


def quantile95(count, m):
    """np.quantile(count / m, 0.95) from the histogram of the counts"""
    hist = np.bincount(np.minimum(count.reshape(-1), m), minlength=m + 1)
    n = int(count.size)
    pos = np.float64(n - 1) * np.float64(0.95)
    lo = int(math.floor(pos))
    t = pos - np.float64(lo)
    hi = min(lo + 1, n - 1)

    def stat(k):
        seen = 0
        for c in range(m + 1):
            seen += int(hist[c])
            if seen > k:
                return np.float64(c) / np.float64(m)
        raise AssertionError

    a, b = stat(lo), stat(hi)
    d = b - a
    return a + d * t if t < 0.5 else b - d * (np.float64(1.0) - t)


def edge_maps(count, m, extra):
    """-> (q, mean, threshold, edges bool [h, w]) of a region's counts; ``extra`` is 0.35 (_borders) or 0.3 (_split)"""
    avg = count.astype(np.float64) / np.float64(m)
    q = quantile95(count, m)
    mean = flat_sum(avg) / np.float64(avg.size)
    floor = q if not (0.2 > q) else np.float64(0.2)
    cap = mean + np.float64(extra)
    threshold = cap if cap < floor else floor
    return q, mean, threshold, avg > threshold


def edge_means(edges):
    """-> (edges.mean(), edges.mean(1), edges.mean(0)) as float32"""
    h, w = edges.shape
    rows = edges.sum(1).astype(F32) / F32(w)
    cols = edges.sum(0).astype(F32) / F32(h)
    return F32(F32(int(edges.sum())) / F32(h * w)), rows, cols


def static_side(var_p, edge_p, edge_at) -> bool:
    level = median(var_p) + mean1d(var_p)
    calm = bool(mean1d(edge_p) < F32(0.0225))
    return bool((level < 75 and calm) or (level < 250 and calm and edge_at > F32(0.65)))


def trim(var_p, edge_p, size):
    bar = F32(0.125) + mean1d(edge_p)
    lines = [i for i in range(1, size - 1) if edge_p[i] > bar]
    first, end = 0, size
    for i in lines:
        if i - first < 5:
            continue
        extra = int(np.rint(np.float64(i - first) * np.float64(0.3)))
        if static_side(var_p[first:i - extra], edge_p[first:i - extra], edge_p[i]):
            first = i + 1
    for i in reversed(lines):
        if end - i < 5:
            continue
        extra = int(np.rint(np.float64(end - i) * np.float64(0.3)))
        if static_side(var_p[i + extra:end], edge_p[i + extra:end], edge_p[i]):
            end = i
    return first, end


def bands(p, size, start, min_size):
    half = GAP // 2
    pieces, inside = [], False
    for i in range(max(size - GAP, 0)):
        level = ((((p[i] + p[i + 1]) + p[i + 2]) + p[i + 3]) + p[i + 4]) / np.float64(GAP)
        if not inside and (level > 0.1 or i - start > 50):
            inside = True
        elif inside and level < 0.1:
            if i + half - start > min_size:
                pieces.append((start, i + half))
            inside = False
            start = i + half
    return pieces, start


def line_cuts(lines, size, min_size):
    """``lines`` descending"""
    pieces, end = [], size
    for i in lines:
        if end - i > min_size:
            pieces.append((i, end))
            end = i
    if pieces and end > min_size:
        pieces.append((0, end))
    return pieces


def split(var, count, m, min_size):
    h, w = var.shape
    rows, start = bands(row_means(var), h, 0, min_size)
    if rows or start != 0:
        if h - start > min_size:
            rows.append((start, h))
        if rows:
            return [(a, b, 0, w) for a, b in rows]
    cols, start = bands(col_means(var), w, start, min_size)
    if cols or start != 0:
        if w - start > min_size:
            cols.append((start, w))
        if cols:
            return [(0, h, a, b) for a, b in cols]
    _, _, _, edges = edge_maps(count, m, 0.3)
    e_all, e_rows, e_cols = edge_means(edges)
    level = F32(0.45) + e_all
    row_lines = [i for i in range(h - 1, -1, -1) if e_rows[i] > level]
    col_lines = [i for i in range(w - 1, -1, -1) if e_cols[i] > level]
    by_rows = lambda: [(a, b, 0, w) for a, b in line_cuts(row_lines, h, min_size)]     # noqa: E731
    by_cols = lambda: [(0, h, a, b) for a, b in line_cuts(col_lines, w, min_size)]     # noqa: E731
    for cut in ((by_cols, by_rows) if w > h else (by_rows, by_cols)):
        pieces = cut()
        if pieces:
            return pieces
    return None


def borders(var, count, m, trace=None):
    q, mean, threshold, edges = edge_maps(count, m, 0.35)
    e_all, e_rows, e_cols = edge_means(edges)
    h, w = var.shape
    v_rows, v_cols = row_means(var), col_means(var)
    if trace is not None:
        trace[:] = [q, mean, threshold, np.float64(e_all), v_rows[h // 2], v_cols[w // 2], np.float64(e_rows[h // 2]),
                    np.float64(e_cols[w // 2])]
    y0, y1 = trim(v_rows, e_rows, h)
    x0, x1 = trim(v_cols, e_cols, w)
    return y0, y1, x0, x1


def decide(var, count, m, n, max_views=MAX_VIEWS, trace=None):
    """-> (boxes [(y0, y1, x0, x1)], status): the views in the reference's order; status 1 (and no boxes) when the item needs more
    than ``max_views`` views or more than STACK pending regions.  ``trace``: a float64 [8] array to fill (left alone with n < 5)."""
    var = np.asarray(var, np.float64)
    count = np.asarray(count)
    h, w = var.shape
    if n < MIN_FRAMES:
        return [(0, h, 0, w)], 0
    stack, views, top = [(0, h, 0, w)], [], True
    with np.errstate(all="ignore"):
        while stack:
            box = stack.pop()
            y0, y1, x0, x1 = box
            b0, b1, a0, a1 = borders(var[y0:y1, x0:x1], count[y0:y1, x0:x1], m, trace if top else None)
            top = False
            cut = (y0 + b0, y0 + b1, x0 + a0, x0 + a1)
            pieces, leaf = None, box
            if min(b1 - b0, a1 - a0) >= MIN_SIDE:
                leaf = cut
                pieces = split(var[cut[0]:cut[1], cut[2]:cut[3]], count[cut[0]:cut[1], cut[2]:cut[3]], m, MIN_VIEW)
                if pieces is not None and len(pieces) == 1 and (pieces[0][1] - pieces[0][0], pieces[0][3] - pieces[0][2]) == (b1 - b0, a1 - a0):
                    pieces = None
            if pieces is None:
                if len(views) == max_views:
                    return [], 1
                views.append(leaf)
                continue
            if len(stack) + len(pieces) > STACK:
                return [], 1
            for p0, p1, q0, q1 in reversed(pieces):
                stack.append((cut[0] + p0, cut[0] + p1, cut[2] + q0, cut[2] + q1))
    return views, 0


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
