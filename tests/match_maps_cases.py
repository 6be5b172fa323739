"""Items for the vsc_match_maps_f32 tests: seeded random similarity matrices plus the planted cases the contract's corners need.
An item is (name, matrix float32 [q_rows, r_rows], frames per view).  Shared by the emulated CPU run and the GPU tests."""
import numpy as np

import match_maps_contract as C

FRAMES = (1, 3, 7, 8, 9, 10, 11, 40, 170)
VIEWS = (2, 3, 5)
EDGES = (31, 32, 33, 63, 64, 65)      # the 64 x 64 transpose tile's edges, and half of it
SENTINEL = np.float32(9.0e9)          # fills the gaps between packed items: a kernel that reads one shows it


def _rand(rs, q_rows, r_rows):
    return rs.uniform(-1.0, 1.0, (q_rows, r_rows)).astype(np.float32)


def _sum_sequential(a):
    s = a[0]
    for v in a[1:]:
        s = np.float32(s + v)
    return s


def summation_order_item(seed=5):
    """Two views of ten rows whose sets of row maxima differ, chosen so that ONLY the stated order of the fp32 sum makes view 1
    the winner: summed ascending one by one, or descending one by one, view 0 would tie or win.  The rows sit in shuffled
    order, so the kernel has to sort them as well."""
    rs = np.random.RandomState(seed)
    for _ in range(200000):
        a = np.sort(rs.uniform(0.3, 1.0, 10).astype(np.float32))
        b = a.copy()
        i, j = rs.choice(10, 2, replace=False)
        b[i] = np.nextafter(b[i], np.float32(2), dtype=np.float32)
        b[j] = np.nextafter(b[j], np.float32(-2), dtype=np.float32)
        b = np.sort(b)
        if not C.view_score(b) > C.view_score(a):
            continue
        if _sum_sequential(b) > _sum_sequential(a) or _sum_sequential(b[::-1]) > _sum_sequential(a[::-1]):
            continue
        r_rows = 12
        m = np.empty((20, r_rows), np.float32)
        for v, top in enumerate((a, b)):
            for k, row in enumerate(rs.permutation(10)):
                m[10 * v + row] = top[k] - rs.uniform(0.05, 0.2, r_rows).astype(np.float32)
                m[10 * v + row, rs.randint(r_rows)] = top[k]
        assert C.view_start(m, 10) == 10
        return "sum_order", m, 10
    raise AssertionError("no pair of views found whose order depends on the summation order")


def planted(resolution, seed=11):
    """The planted items for one canvas side R."""
    rs = np.random.RandomState(seed + resolution)
    R = resolution
    items = [("single_smaller", _rand(rs, max(R - 3, 1), max(R - 5, 1)), max(R - 3, 1)),
             ("single_taller", _rand(rs, R + 7, max(R - 2, 1)), R + 7),
             ("single_wider", _rand(rs, max(R - 2, 1), R + 9), max(R - 2, 1)),
             ("single_both", _rand(rs, R + 5, R + 6), R + 5),
             ("single_fewer_rows_than_frames", _rand(rs, 12, 17), 20),
             ("single_r1", _rand(rs, 5, 1), 5),
             ("multi_r1", _rand(rs, 12, 1), 4),
             ("empty_rows", np.zeros((0, 5), np.float32), 6),
             ("empty_columns", np.zeros((4, 0), np.float32), 4)]
    for frames in FRAMES:
        for views in VIEWS:
            items.append((f"multi_f{frames}_v{views}", _rand(rs, frames * views, int(rs.randint(1, 200))), frames))
    items.append(("multi_taller_and_wider", _rand(rs, 3 * 230, 241), 230))
    items.append(("all_negative", -rs.uniform(0.1, 1.0, (33, 21)).astype(np.float32), 11))
    view = _rand(rs, 12, 30)
    items.append(("identical_views", np.concatenate([view - np.float32(0.5), view, view, view - np.float32(0.25)]), 12))
    coarse = (rs.randint(-8, 9, (60, 9)) / 8.0).astype(np.float32)        # many equal maxima: ties inside and across views
    items.append(("coarse_ties", coarse, 12))
    items.append(summation_order_item())
    for h in EDGES:
        for w in EDGES:
            items.append((f"edge_{h}x{w}", _rand(rs, h, w), h))
    items.append(("edge_multi_65x33", _rand(rs, 3 * 65, 33), 65))
    return items


def pack(items, lead=7):
    """-> (flat float32, table int64 [n, 4]): the matrices back to back behind `lead` unused floats, with an unused float
    between neighbours where that makes the next offset odd -- so offsets are non-zero and mostly odd."""
    parts, table, off = [np.full(lead, SENTINEL, np.float32)], [], lead
    for _, m, frames in items:
        if off % 2 == 0:
            parts.append(np.full(1, SENTINEL, np.float32))
            off += 1
        table.append((off, m.shape[0], m.shape[1], frames))
        parts.append(np.ascontiguousarray(m, np.float32).reshape(-1))
        off += m.size
    return np.concatenate(parts), np.array(table, np.int64).reshape(-1, 4)
