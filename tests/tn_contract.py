"""Executable statement of the TN contract (include/vsc_hip.h, vsc_tn_align_f32), written the way the kernel computes it:
top-K per row, predecessor bitmasks, Kahn ranks once per pair, rounds of layer-by-layer longest path.  Test helper
only -- it checks the contract against the reference's fixture on the CPU; the project never runs it in place of the
kernel.  Plain Python over np.float32 scalars, so every add and comparison is the fp32 / float64 one the contract names."""
import numpy as np

f32 = np.float32


def tn_contract(m, bias, tn_max_step=10, tn_top_k=5, max_path=10, min_sim=0.2, min_length=5, max_iou=0.3):
    Q, R = m.shape
    step = tn_max_step
    top = min(tn_top_k, R)
    if Q == 0 or top == 0:
        return [], []
    sims = (m + f32(bias)).astype(np.float32)
    # (A) top-K: descending value, ties to the lower column
    col = np.empty((Q, top), np.int64)
    val = np.empty((Q, top), np.float32)
    for q in range(Q):
        order = sorted(range(R), key=lambda c: (-sims[q, c], c))[:top]
        col[q], val[q] = order, sims[q, order]
    N = 1 + Q * top
    sink = N - 1

    def node(q, k):
        return 1 + q * top + k

    def bit(d, c):                         # predecessor bit of (q_j - d, c) in a node of row q_j: ascending = pred order
        return (step - 1 - d) * top + c

    minsim32 = f32(min_sim)
    # (B) predecessor masks
    pred = [0] * N
    for qi in range(Q):
        nxt = [None] * top                 # smallest intermediate column above col[qi, c]
        for d in range(1, step):
            qj = qi + d
            if qj >= Q:
                break
            valid = []
            for k in range(top):
                if not (val[qj, k] >= minsim32):
                    continue
                hit = False
                for c in range(top):
                    diff = col[qj, k] - col[qi, c]
                    if not (0 < diff < step):
                        continue
                    if nxt[c] is not None and nxt[c] < col[qj, k]:
                        continue
                    pred[node(qj, k)] |= 1 << bit(d, c)
                    hit = True
                if hit:
                    valid.append(col[qj, k])
            for x in valid:
                for c in range(top):
                    if x > col[qi, c] and (nxt[c] is None or x < nxt[c]):
                        nxt[c] = x
    qs, cs = col[Q - 1, top - 1], Q - 1

    def in_s(u):                          # sink edge condition of node u (node 0 = (-1, -1))
        qu, cu = (-1, -1) if u == 0 else ((u - 1) // top, col[(u - 1) // top, (u - 1) % top])
        return u != sink and cs > qu and qs > cu and cs - qu <= step and qs - cu <= step

    def in_r(u):                          # regular edge u -> sink
        if u == 0:
            return False
        qu, cu = (u - 1) // top, (u - 1) % top
        d = cs - qu
        return 0 < d < step and (pred[sink] >> bit(d, cu)) & 1

    s_only = [u for u in range(N) if in_s(u) and not in_r(u)]
    sink_preds = [u for u in range(1, N) if in_r(u)] + s_only

    def preds(v):
        if v == sink:
            return [(u, True) for u in sink_preds]
        qj = (v - 1) // top
        out = []
        for b in range(64):
            if (pred[v] >> b) & 1:
                d, c = step - 1 - b // top, b % top
                out.append((node(qj - d, c), False))
        return out

    def succs(u):
        out = []
        if u != 0:
            qi, c = (u - 1) // top, (u - 1) % top
            for d in range(1, step):
                for k in range(top):
                    if qi + d < Q and (pred[node(qi + d, k)] >> bit(d, c)) & 1:
                        out.append(node(qi + d, k))
        if u in s_only_set:
            out.append(sink)
        return out

    s_only_set = set(s_only)
    # (C) Kahn ranks
    indeg = [len(preds(v)) for v in range(N)]
    queue = [v for v in range(N) if indeg[v] == 0]
    i = 0
    while i < len(queue):
        for v in succs(queue[i]):
            indeg[v] -= 1
            if indeg[v] == 0:
                queue.append(v)
        i += 1
    assert len(queue) == N
    rank = [0] * N
    for i, v in enumerate(queue):
        rank[v] = i
    # (D) rounds
    zeroed = [0] * N
    boxes = []
    for _ in range(max_path + 1):
        dist = [f32(0)] * N
        back = list(range(N))
        for v in range(1, N):
            best, bu = None, v
            w = val[(v - 1) // top, (v - 1) % top]
            for u, is_sink in preds(v):
                if is_sink:
                    x = dist[u] + f32(0)
                else:
                    qj = (v - 1) // top
                    d, c = qj - (u - 1) // top, (u - 1) % top
                    x = dist[u] + (f32(0) if (zeroed[v] >> bit(d, c)) & 1 else w)
                if best is None or x > best:
                    best, bu = x, u
            if best is not None and best >= 0:
                dist[v], back[v] = best, bu
        end = min(range(N), key=lambda v: (-dist[v], rank[v]))
        path = [end]
        while back[path[-1]] != path[-1]:
            path.append(back[path[-1]])
        path.reverse()
        for u, v in zip(path, path[1:]):
            if v != sink:
                d, c = (v - 1) // top - (u - 1) // top, (u - 1) % top
                zeroed[v] |= 1 << bit(d, c)
        path = [v for v in path if v != 0 and v != sink]
        if not path:
            break
        score = f32(0)
        for v in path:
            score = f32(score + val[(v - 1) // top, (v - 1) % top])
        pq = [(v - 1) // top for v in path]
        pr = [int(col[(v - 1) // top, (v - 1) % top]) for v in path]
        box = [min(pq), min(pr), max(pq), max(pr)] if score > 0 else [0, 0, 0, 0]
        ave = ((box[3] - box[1]) + (box[2] - box[0])) / 2.0
        if score > 0:
            ok = (float(score) / ave if ave else float("inf")) > min_sim
        else:
            ok = False
        ok = ok and min(box[3] - box[1], box[2] - box[0]) > min_length
        if ok:
            best_iou = 0.0
            for g in boxes:
                iw = max(min(box[2], g[2]) - max(box[0], g[0]) + 1, 0)
                ih = max(min(box[3], g[3]) - max(box[1], g[1]) + 1, 0)
                inter = iw * ih
                ua = (box[2] - box[0] + 1) * (box[3] - box[1] + 1) + (g[2] - g[0] + 1) * (g[3] - g[1] + 1) - inter
                best_iou = max(best_iou, inter / ua)
            ok = best_iou < max_iou
        if ok:
            boxes.append(box)
    maxsim = [float(sims[b[0]:b[2], b[1]:b[3]].max() - f32(bias)) for b in boxes]
    return boxes, maxsim
