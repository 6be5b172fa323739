"""Executable statement of the DP and HV alignment contracts (include/vsc_hip.h, vsc_align_dp_f32 / vsc_align_hv_f32), written
the way the kernels compute them.  Test helper only -- it checks the contracts against the reference's fixture
(tests/golden/align_dp_hv.json) on the CPU and serves the GPU tests as the expected MaxSim; the project never runs it in
place of a kernel.  Plain Python over np.float32 scalars, so every add, multiply and comparison is the fp32 one the contract
names.

`dp_contract(..., wide=True)` is the same recurrence under numba's typing (the two half-weight candidates and the `min_sim`
comparison in float64), kept only so that the fixture can record per case whether that typing would change the boxes."""
import numpy as np

f32 = np.float32
NINF = f32(-np.inf)


def pairwise_f32(vals):
    """numpy's pairwise float32 sum of a sequence, restated: fewer than 8 elements in order; up to 128 in eight strided
    accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the remainder added in order; longer ones split at n // 2
    rounded down to a multiple of 8."""
    n = len(vals)
    if n < 8:
        res = f32(0.0)
        for v in vals:
            res = f32(res + v)
        return res
    if n <= 128:
        r = [f32(v) for v in vals[:8]]
        full = n - n % 8
        for i in range(8, full, 8):
            for k in range(8):
                r[k] = f32(r[k] + vals[i + k])
        res = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
        for i in range(full, n):
            res = f32(res + vals[i])
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return f32(pairwise_f32(vals[:n2]) + pairwise_f32(vals[n2:]))


def _maxsim(sb, box, bias):
    x1, y1, x2, y2 = box
    sub = sb[x1:x2, y1:y2]
    return f32(sub.max() - f32(bias)) if sub.size else NINF


def keep_ranges(path, diagonal_thres):
    """`cut_path` restated: the maximal runs of steps that keep the row (resp. the column) and cover more than
    `diagonal_thres` path cells are discarded; what lies between consecutive discarded ranges, from 0 and up to
    len(path), is kept.  A run of one kind followed at once by a run of the other overlaps it by one cell, which gives a
    range with start > end."""
    L = len(path)
    discard = []
    a = 0
    while a < L - 1:
        kind = 0 if path[a + 1][0] == path[a][0] else (1 if path[a + 1][1] == path[a][1] else 2)
        b = a + 1
        if kind == 2:
            a = b
            continue
        while b < L - 1 and (path[b + 1][kind] == path[b][kind]):
            b += 1
        if b + 1 - a > diagonal_thres:          # steps a .. b-1 -> cells a .. b
            discard.append((a, b + 1))
        a = b
    out, prev = [], 0
    for s, e in discard:
        out.append((prev, s))
        prev = e
    out.append((prev, L))
    return out


def dp_contract(m, bias, discontinue=3, min_sim=0.0, ave_sim=0.3, min_length=5, diagonal_thres=10, wide=False, stats=None):
    """-> (boxes, maxsim) of one [Q, R] fp32 matrix; every box found, in order (the kernel stores the first max_boxes)."""
    Q, R = m.shape
    if Q == 0 or R == 0:
        return [], []
    sb = (np.asarray(m, dtype=np.float32) + f32(bias)).astype(np.float32)
    sim = (sb + f32(1.0)).astype(np.float32)
    dp = sim.copy()
    acc = np.zeros((Q, R), np.int32)
    bt = -np.ones((Q, R), np.int8)
    half, min32 = f32(0.5), f32(min_sim)
    prevs = ((-1, -1), (-1, 0), (0, -1))
    for i in range(1, Q):
        for j in range(1, R):
            s = sim[i, j]
            if wide:
                c = [np.float64(f32(dp[i - 1, j - 1] + s)), np.float64(dp[i - 1, j]) + 0.5 * np.float64(s),
                     np.float64(dp[i, j - 1]) + 0.5 * np.float64(s)]
                unmatch = np.float64(s) < float(min_sim)
            else:
                c = [f32(dp[i - 1, j - 1] + s), f32(dp[i - 1, j] + f32(half * s)), f32(dp[i, j - 1] + f32(half * s))]
                unmatch = s < min32
            k = 0
            if c[1] > c[k]:
                k = 1
            if c[2] > c[k]:
                k = 2
            if unmatch:
                acc[i, j] = acc[i + prevs[k][0], j + prevs[k][1]] + 1
            if acc[i, j] <= discontinue:
                bt[i, j] = k
                dp[i, j] = f32(c[k])
    if stats is not None:
        stats.update(max_acc=int(acc.max()), rounds=0, stopped=False, crossed=0, mean_at_threshold=0, discarded=0)
    ave32 = f32(ave_sim)
    boxes = []
    for _ in range(100):
        flat = int(np.argmax(dp))                # the first maximum in row-major order
        i, j = divmod(flat, R)
        if dp[i, j] == NINF:
            if stats is not None:
                stats["stopped"] = True
            break
        walk = [(i, j)]
        while bt[i, j] != -1:
            di, dj = prevs[bt[i, j]]
            i, j = i + di, j + dj
            if dp[i, j] == NINF:
                break
            walk.append((i, j))
        path = walk[::-1]
        (r1, c1), (r2, c2) = path[0], path[-1]
        dp[r1:r2 + 1, c1:c2 + 1] = NINF
        ranges = keep_ranges(path, diagonal_thres)
        if stats is not None:
            stats["rounds"] += 1
            stats["crossed"] += sum(s > e for s, e in ranges)
            stats["discarded"] += len(ranges) - 1
        for s, e in ranges:
            if not e - s > min_length:
                continue
            sub = path[s:e]
            mean = f32(pairwise_f32([sim[p] for p in sub]) / f32(len(sub)))
            if stats is not None and mean == ave32:
                stats["mean_at_threshold"] += 1
            if mean > ave32 and sub[-1][0] - sub[0][0] > min_length and sub[-1][1] - sub[0][1] > min_length:
                boxes.append([int(sub[0][0]), int(sub[0][1]), int(sub[-1][0]), int(sub[-1][1])])
    return boxes, [_maxsim(sb, b, bias) for b in boxes]


def iou_int(a, b):
    """IoU of two inclusive boxes with "+1" integer areas and one float64 division (vta.py `iou` on integer corners)."""
    iw = max(min(a[2], b[2]) - max(a[0], b[0]) + 1, 0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]) + 1, 0)
    inter = iw * ih
    union = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    return float(inter) / float(union)


def hv_contract(m, bias, iou_thresh=0.9, min_sim=0.0, max_peaks=100, stats=None):
    """-> (boxes, maxsim) of one [Q, R] fp32 matrix."""
    Q, R = m.shape
    if Q == 0 or R == 0:
        return [], []
    sb = (np.asarray(m, dtype=np.float32) + f32(bias)).astype(np.float32)
    min32 = f32(min_sim)
    z = sb.copy()
    z[z < min32] = f32(0.0)
    peaks = []
    for sigma in range(-(Q - 1), R):
        a = max(-sigma, 0)
        e = min(max(R - sigma, 0), Q)
        vals = [z[q, q + sigma] for q in range(a, e)]
        if not any(v >= min32 for v in vals):
            continue
        peaks.append((sigma, a, e, pairwise_f32(vals)))
    order = sorted(range(len(peaks)), key=lambda p: -float(peaks[p][3]))      # stable: ties stay in ascending sigma
    if stats is not None:
        scores = [float(p[3]) for p in peaks]
        stats.update(peaks=len(peaks), ties=len(scores) - len(set(scores)), rejected=0)
    boxes = []
    for p in order[:max_peaks]:
        sigma, a, e, score = peaks[p]
        if score <= 0:
            continue
        box = [a, a + sigma, e - 1, e - 1 + sigma]
        worst = max([iou_int(box, g) for g in boxes], default=0.0)
        if worst > iou_thresh:
            if stats is not None:
                stats["rejected"] += 1
            continue
        boxes.append(box)
    return boxes, [_maxsim(sb, b, bias) for b in boxes]


class ContractModel:
    """The contract behind `forward_sim`: VCSL's model interface over dp_contract / hv_contract (the matrices arrive biased)."""

    def __init__(self, method, **params):
        self.fn = {"DP": dp_contract, "HV": hv_contract}[method]
        self.params = params

    def forward_sim(self, data):
        return [(key, self.fn(np.array(m, dtype=np.float32), 0.0, **self.params)[0]) for key, m in data]
