"""Probability maps of the segment-extraction fixture (tests/golden/match_segments.json).

Every map is rebuilt from its recipe with `np.random.RandomState` and elementwise fp32 operations only, so any machine
reproduces the same bytes; each recorded case carries the SHA-256 of its map.  The maps are band maps in the style of
tests/test_matching.py::_probability_map: a faint background, copied segments as lines of high probability, and a few
isolated hits ("specks", the small components).  The fixture generator (tests/golden/gen_match_segments_golden.py), the
CPU suite and the GPU suite all build their inputs here.

Families:
  clean   thin lines (one pixel per query frame), zero background, no specks: most trials meet no boundary point
  thin    thin lines with at most one extra pixel beside the line, noise and specks
  thick   lines up to 3 pixels thick, noise and specks
  edge    degenerate shapes, an empty map, a map that is above the lowest threshold everywhere

A case is a dict: name, family, h, w, seed, noise, specks, thick, bands = [(q0, r0, frames, slope, level), ...] and
optionally rows = [(query frame, r0, points, level), ...] (runs of points that share one query frame) and fill.
"""
import hashlib

import numpy as np

# (threshold, std_ratio) of the three passes of infer_matching.py:289-291
PASSES = ((0.35, 0.5), (0.1, 1.25), (0.001, 2))
MAX_SIDE = 224


def matrix(case):
    """The fp32 [h, w] probability map of one case."""
    rs = np.random.RandomState(case["seed"])
    h, w = case["h"], case["w"]
    m = (rs.random_sample((h, w)) * case["noise"]).astype(np.float32)
    if case.get("fill") is not None:
        m = (np.float32(case["fill"]) * (1 + rs.random_sample((h, w)) / 2)).astype(np.float32)   # unequal weights everywhere
    thick = case["thick"]
    for q0, r0, n, slope, level in case["bands"]:
        for t in range(n):
            i, j = q0 + t, int(np.floor(r0 + slope * t + 0.5))
            if not (0 <= i < h and 0 <= j < w):
                continue
            m[i, j] = np.float32(level) - np.float32(0.002) * np.float32(t)
            if thick == 1 and t % 3 == 0 and j + 1 < w:
                m[i, j + 1] = np.float32(level) - np.float32(0.1)
            if thick >= 2:
                for d in range(1, thick):
                    if rs.random_sample() < 0.7:
                        jj = j + (d if d % 2 else -d)
                        if 0 <= jj < w:
                            m[i, jj] = np.float32(level) - np.float32(0.05 * d) - np.float32(rs.random_sample() * 0.05)
    for x, y0, n, level in case.get("rows", ()):              # n points sharing ONE query frame: trials with dx = 0
        for t in range(n):
            if 0 <= x < h and 0 <= y0 + t < w:
                m[x, y0 + t] = np.float32(level) - np.float32(0.002) * np.float32(t)
    if case["specks"] and h and w:
        at = np.stack([rs.randint(0, h, size=case["specks"]), rs.randint(0, w, size=case["specks"])], axis=1)
        m[at[:, 0], at[:, 1]] = np.float32(0.5) - np.float32(0.0005) * np.arange(case["specks"], dtype=np.float32)
    return np.ascontiguousarray(m, dtype=np.float32)


def digest(m):
    return hashlib.sha256(np.ascontiguousarray(m, dtype=np.float32).tobytes()).hexdigest()


def _case(name, family, h, w, seed, bands, noise=0.03, specks=12, thick=0, **extra):
    return dict(name=name, family=family, h=h, w=w, seed=seed, noise=noise, specks=specks, thick=thick,
                bands=[list(b) for b in bands], **extra)


def _bands(rs, h, w, count, slopes):
    """`count` bands that stay inside the map, apart from each other along the query axis."""
    out = []
    span = h // count
    for b in range(count):
        slope = slopes[(b + int(rs.randint(0, len(slopes)))) % len(slopes)]
        n = int(rs.randint(max(8, span // 2), max(9, span - 2)))
        n = min(n, int((w - 2) / abs(slope)) if slope else n)
        q0 = b * span + int(rs.randint(0, max(1, span - n)))
        reach = int(abs(slope) * n) + 1
        r_lo, r_hi = (0, max(1, w - reach)) if slope > 0 else (min(reach, w - 1), w)
        r0 = int(rs.randint(r_lo, max(r_lo + 1, r_hi)))
        out.append((q0, r0, n, slope, round(0.95 - 0.07 * b, 3)))
    return out


SLOPES = (1.0, 1.0, 0.5, 2.0, 1.25, 1.0, -1.0)


def cases():
    """The recorded cases, in fixture order (names are unique)."""
    out = []
    seed = 5000
    sizes = [(40, 50), (60, 80), (48, 48), (70, 40), (96, 130), (120, 90), (160, 160), (224, 224), (200, 224), (30, 160)]
    # clean thin lines: zero background, no specks
    for rep in range(20):
        seed += 1
        rs = np.random.RandomState(seed)
        h, w = sizes[rep % len(sizes)]
        out.append(_case(f"clean_{rep:02d}_{h}x{w}", "clean", h, w, seed, _bands(rs, h, w, 1 + rep % 3, SLOPES), noise=0.0, specks=0))
    # thin lines with an occasional second pixel, noise and specks
    for rep in range(22):
        seed += 1
        rs = np.random.RandomState(seed)
        h, w = sizes[(rep + 3) % len(sizes)]
        out.append(_case(f"thin_{rep:02d}_{h}x{w}", "thin", h, w, seed, _bands(rs, h, w, 1 + rep % 3, SLOPES), thick=rep % 2))
    # thick lines
    for rep in range(14):
        seed += 1
        rs = np.random.RandomState(seed)
        h, w = sizes[(rep + 5) % len(sizes)]
        out.append(_case(f"thick_{rep:02d}_{h}x{w}", "thick", h, w, seed, _bands(rs, h, w, 1 + rep % 2, SLOPES), thick=2 + rep % 2))
    # degenerate shapes and extremes
    seed += 1
    out += [
        _case("edge_empty", "edge", 64, 64, seed, [], noise=0.0, specks=0),
        _case("edge_all_above", "edge", 224, 224, seed + 1, [(20, 30, 150, 1.0, 0.9)], noise=0.0, specks=0, fill=0.002),
        _case("edge_all_above_small", "edge", 50, 40, seed + 2, [(5, 5, 30, 1.0, 0.9)], noise=0.0, specks=0, fill=0.01),
        _case("edge_1x1", "edge", 1, 1, seed + 3, [], specks=1),
        _case("edge_1x224", "edge", 1, 224, seed + 4, [(0, 0, 1, 1.0, 0.9)]),
        _case("edge_224x1", "edge", 224, 1, seed + 5, [(0, 0, 224, 0.0, 0.9)], specks=0),
        _case("edge_4x4", "edge", 4, 4, seed + 6, [(0, 0, 4, 1.0, 0.9)], specks=0),
        _case("edge_3x60", "edge", 3, 60, seed + 7, [(0, 5, 3, 1.0, 0.9)], specks=2),
        _case("edge_specks_only", "edge", 25, 25, seed + 8, []),
        _case("edge_constant_ref_frame", "edge", 60, 60, seed + 9, [(10, 20, 30, 0.0, 0.9)], specks=4),
        _case("edge_one_pixel_and_specks", "edge", 60, 60, seed + 10, [(30, 5, 1, 1.0, 0.9)], specks=30, noise=0.0),
        _case("edge_short", "edge", 40, 40, seed + 11, [(3, 3, 5, 1.0, 0.9), (20, 10, 7, 1.0, 0.8)], specks=3),
        _case("edge_full_diag_224", "edge", 224, 224, seed + 12, [(0, 0, 224, 1.0, 0.95)], specks=0, noise=0.0),
        _case("edge_many_specks", "edge", 120, 120, seed + 13, [(10, 12, 60, 1.0, 0.9)], specks=260),
        _case("edge_one_query_frame", "edge", 60, 80, seed + 14, [(5, 8, 30, 1.0, 0.9)], specks=6, rows=[(40, 10, 40, 0.8)]),
        _case("edge_query_frame_rows_only", "edge", 40, 60, seed + 15, [], specks=8, noise=0.0,
              rows=[(5, 3, 30, 0.9), (6, 4, 30, 0.85), (20, 10, 25, 0.8), (30, 0, 50, 0.7)]),
    ]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), "duplicate case names"
    return out


def by_name():
    return {c["name"]: c for c in cases()}
