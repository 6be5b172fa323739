"""Cases of the device view decisions (tests/view_decide_contract.py, csrc/view_decide.hip): the two maps of the 21 recipes of
tests/view_cases.py (the inputs of tests/golden/view_preprocess.json, through canny_cpu.frame_var / canny_cpu.canny_count), and
PLANTED maps built directly: moving panels are random variances of a few hundred to a few thousand (so every summation order
shows in the bits of the sums), static ground is below the band level of 0.1, panel outlines are edge lines on every sample, and
sparse random edges of 1..m samples fill the panels.

A case is a dict: name; var float64 [h, w]; count uint16 [h, w]; m Canny samples; n frames; max_views."""
import functools

import numpy as np

import canny_cpu
import view_cases
import view_decide_contract as C
from src.image_preprocess import canny_frames

EMULATED_MAX = 330          # the emulation runs one OS thread per GPU thread
WIDTHS = (1, 7, 8, 9, 128, 129, 257)


def planted(name, h, w, m=20, n=8, seed=0, panels=None, lines=True, density=0.03, max_views=C.MAX_VIEWS):
    rng = np.random.default_rng([seed, h, w, m])
    var = rng.uniform(0.0, 0.04, (h, w))
    count = np.zeros((h, w), np.uint16)
    for y0, y1, x0, x1 in ([(0, h, 0, w)] if panels is None else panels):
        ph, pw = y1 - y0, x1 - x0
        var[y0:y1, x0:x1] = rng.uniform(200.0, 4000.0, (ph, pw))
        count[y0:y1, x0:x1] = np.where(rng.random((ph, pw)) < density, rng.integers(1, m + 1, (ph, pw)), 0)
        if lines:
            count[y0, x0:x1] = count[y1 - 1, x0:x1] = m
            count[y0:y1, x0] = count[y0:y1, x1 - 1] = m
    return dict(name=name, var=var, count=count, m=m, n=n, max_views=max_views)


def _random(name, seed):
    """a random frame up to 330 on a side: a static margin on some sides, one to three panels stacked along one axis with static
    bands of 8-14 lines between them"""
    rng = np.random.default_rng([seed, 77])
    h, w = (int(v) for v in rng.integers(180, 331, 2))
    top, left = (int(v) for v in rng.integers(0, 25, 2) * rng.integers(0, 2, 2))
    bottom, right = (int(v) for v in rng.integers(0, 25, 2) * rng.integers(0, 2, 2))
    k = int(rng.integers(1, 4))
    vertical = bool(rng.integers(0, 2))
    lo, hi = (top, h - bottom) if vertical else (left, w - right)
    gaps = [int(g) for g in rng.integers(8, 15, k - 1)]
    each = (hi - lo - sum(gaps)) // k
    panels, at = [], lo
    for j in range(k):
        end = hi if j == k - 1 else at + each
        panels.append((at, end, left, w - right) if vertical else (top, h - bottom, at, end))
        at = end + (gaps[j] if j < k - 1 else 0)
    return planted(name, h, w, m=int(rng.integers(1, 21)), n=int(rng.integers(5, 60)), seed=seed, panels=panels,
                   lines=bool(rng.integers(0, 2)), density=float(rng.choice([0.0, 0.01, 0.05, 0.2])))


def _recipe(case):
    frames = view_cases.frames(case)
    idx = canny_frames(len(frames))
    return dict(name="recipe_" + case["name"], var=canny_cpu.frame_var(frames), count=canny_cpu.canny_count(frames, idx),
                m=len(idx), n=len(frames), max_views=C.MAX_VIEWS)


RECIPES = [c["name"] for c in view_cases.cases()]


def _planted_cases():
    c = {}
    for w in WIDTHS:
        c[f"width_{w}"] = lambda w=w: planted(f"width_{w}", 37, w, seed=w)
        c[f"height_{w}"] = lambda w=w: planted(f"height_{w}", w, 41, seed=100 + w, lines=False)
    c["pixels_8192"] = lambda: planted("pixels_8192", 64, 128, seed=1)
    c["pixels_8193"] = lambda: planted("pixels_8193", 3, 2731, seed=2)
    c["pixels_3x8192_5"] = lambda: planted("pixels_3x8192_5", 47, 523, seed=3)
    for m in (1, 7, 20):
        c[f"samples_{m}"] = lambda m=m: planted(f"samples_{m}", 150, 190, m=m, seed=10 + m, panels=[(18, 130, 0, 190)])
    c["frames_4"] = lambda: planted("frames_4", 150, 190, n=4, seed=20, panels=[(18, 130, 0, 190)])
    c["frames_5"] = lambda: planted("frames_5", 150, 190, n=5, seed=20, panels=[(18, 130, 0, 190)])
    grid = [(10, 160, 8, 158), (10, 160, 170, 322), (172, 320, 8, 158), (172, 320, 170, 322)]
    c["grid_2x2"] = lambda: planted("grid_2x2", 330, 330, seed=30, panels=grid)
    c["pip_in_grid"] = lambda: planted("pip_in_grid", 330, 330, seed=31, panels=[(10, 160, 8, 322), (200, 310, 60, 250)])
    stack3 = [(0, 100, 0, 150), (110, 205, 0, 150), (215, 320, 0, 150)]
    c["stack3"] = lambda: planted("stack3", 320, 150, seed=40, panels=stack3)
    c["over_max_views_2"] = lambda: planted("over_max_views_2", 320, 150, seed=40, panels=stack3, max_views=2)
    c["dense_edges"] = lambda: planted("dense_edges", 200, 240, seed=50, density=0.5, panels=[(0, 200, 25, 240)])
    c["all_static"] = lambda: planted("all_static", 120, 140, seed=51, panels=[])
    for s in range(8):
        c[f"random_{s}"] = lambda s=s: _random(f"random_{s}", s)
    c["letterbox_720p"] = lambda: planted("letterbox_720p", 720, 1280, seed=60, panels=[(90, 630, 0, 1280)])
    return c


PLANTED = _planted_cases()
ENGINEERED = ("over_max_views_2",)
LARGE = ("letterbox_720p",)


def names(large=True):
    """every case, recipes first; ``large=False``: without the ones too large for the emulation (above EMULATED_MAX on a side;
    the thin maps of 8193 and 3 x 8192 + 5 pixels stay)"""
    out = ["recipe_" + n for n in RECIPES] + list(PLANTED)
    return [n for n in out if large or n not in LARGE]


@functools.lru_cache(maxsize=None)
def get(name):
    if name.startswith("recipe_"):
        case = _recipe(next(c for c in view_cases.cases() if c["name"] == name[len("recipe_"):]))
    else:
        case = PLANTED[name]()
    case["var"].setflags(write=False)
    case["count"].setflags(write=False)
    assert case["name"] == name
    return case


@functools.lru_cache(maxsize=None)
def expected(name):
    """the contract's (boxes, status, trace float64 [8]); the trace starts as NaN with all bits set and stays so with n < 5"""
    case = get(name)
    trace = np.full(8, 0xFF, np.uint8).repeat(8).view(np.float64).copy()
    boxes, status = C.decide(case["var"], case["count"], case["m"], case["n"], case["max_views"], trace)
    trace.setflags(write=False)
    return boxes, status, trace


def batch(sel):
    """the maps of ``sel`` in one pair of flat arrays at odd element offsets, NaN / 0xFFFF between them -> (var, count, items
    int64 [n, 6])"""
    vars_, counts, items, voff, coff = [], [], [], 0, 0
    for k, name in enumerate(sel):
        case = get(name)
        h, w = case["var"].shape
        pad_v, pad_c = 1 + 2 * (k % 3), 3 + 2 * (k % 2)
        vars_ += [np.full(pad_v, np.nan), case["var"].reshape(-1)]
        counts += [np.full(pad_c, 0xFFFF, np.uint16), case["count"].reshape(-1)]
        items.append((voff + pad_v, coff + pad_c, h, w, case["m"], case["n"]))
        voff += pad_v + h * w
        coff += pad_c + h * w
    return np.concatenate(vars_), np.concatenate(counts), np.asarray(items, np.int64).reshape(-1, 6)
