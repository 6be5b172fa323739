"""Similarity matrices of the DP / HV alignment fixture (tests/golden/align_dp_hv.json).

Every matrix is rebuilt from its recipe with `np.random.RandomState` and elementwise fp32 operations only, so any machine
reproduces the same bytes; each recorded case carries the SHA-256 of its input.  The fixture generator
(tests/golden/gen_align_golden.py), the CPU tests and the GPU tests all build their inputs here.

A case is a dict: name, model ("DP" / "HV"), q, r, seed, bias, params (the model's parameters) and the recipe keys read by
`matrix`:
  noise   (lo, hi) of the uniform background, or const: one value everywhere
  paths   [(q0, r0, moves, level, jitter)]: cells planted along a walk; moves like "D20,V9,H11" (D: q+1 r+1, V: q+1, H: r+1)
  grid    True: every value rounded to a multiple of 2^-10 (all the sums of the contracts are exact there)
  exact   [(q0, r0, moves, threshold)]: cells whose (s + bias) + 1 equals float32(threshold) bit for bit (DP)
"""
import hashlib

import numpy as np

f32 = np.float32

# dp()'s own defaults with a usable diagonal_thres; DpVtaModel's defaults; the baseline's min_length; thresholds off the fp32 grid
DP_FUNC = dict(discontinue=3, min_sim=1.0, ave_sim=1.3, min_length=5, diagonal_thres=10)
DP_MODEL = dict(discontinue=3, min_sim=0.0, ave_sim=0.3, min_length=5, diagonal_thres=10)
DP_SSCD = dict(discontinue=3, min_sim=1.0, ave_sim=1.3, min_length=4, diagonal_thres=10)
DP_OFFGRID = dict(discontinue=2, min_sim=1.3, ave_sim=1.3, min_length=3, diagonal_thres=6)
DP_AVE03 = dict(discontinue=3, min_sim=0.0, ave_sim=0.3, min_length=5, diagonal_thres=10)
HV_MODEL = dict(iou_thresh=0.9, min_sim=0.0, max_peaks=100)

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (65, 63), (129, 40), (40, 129), (40, 120)]


def walk(q0, r0, moves):
    cells = [(q0, r0)]
    for tok in moves.split(","):
        if not tok:
            continue
        dq, dr = {"D": (1, 1), "V": (1, 0), "H": (0, 1)}[tok[0]]
        for _ in range(int(tok[1:])):
            q0, r0 = q0 + dq, r0 + dr
            cells.append((q0, r0))
    return cells


def matrix(case):
    """The unbiased fp32 [q, r] matrix of one case."""
    rs = np.random.RandomState(case["seed"])
    q, r, bias = case["q"], case["r"], case["bias"]
    if case.get("const") is not None:
        m = np.full((q, r), case["const"], dtype=np.float32)
    else:
        lo, hi = case["noise"]
        m = rs.uniform(lo, hi, size=(q, r)).astype(np.float32)
    for q0, r0, moves, level, jitter in case.get("paths", ()):
        for qi, ri in walk(q0, r0, moves):
            jit = f32(rs.uniform(-jitter, jitter)) if jitter else f32(0.0)
            if 0 <= qi < q and 0 <= ri < r:
                m[qi, ri] = f32(level) + jit
    if case.get("grid"):
        m = (np.round(m * f32(1024.0)) / f32(1024.0)).astype(np.float32)
    for q0, r0, moves, thr in case.get("exact", ()):
        s = f32(f32(f32(thr) - f32(1.0)) - f32(bias))
        assert f32(f32(s + f32(bias)) + f32(1.0)) == f32(thr), (case["name"], thr)
        for qi, ri in walk(q0, r0, moves):
            if 0 <= qi < q and 0 <= ri < r:
                m[qi, ri] = s
    return np.ascontiguousarray(m, dtype=np.float32)


def digest(m):
    return hashlib.sha256(np.ascontiguousarray(m, dtype=np.float32).tobytes()).hexdigest()


def _case(name, model, q, r, seed, bias, params, **recipe):
    return dict(name=name, model=model, q=q, r=r, seed=seed, bias=bias, params=dict(params), **recipe)


def dp_cases():
    out = []
    seed = 3000
    noise = {0.0: (-0.3, 0.35), 0.5: (-0.8, -0.15)}            # (s + bias) + 1 in [0.7, 1.35): mostly below min_sim = 1
    level = {0.0: 0.8, 0.5: 0.3}

    def add(name, q, r, bias, params, **recipe):
        nonlocal seed
        seed += 1
        grid = len(out) % 3 == 0                                # a third of the cases on the 2^-10 grid
        recipe.setdefault("noise", noise[bias])
        out.append(_case(name + ("_g" if grid else ""), "DP", q, r, seed, bias, params, grid=grid, **recipe))

    # the shapes of the issue: noise, and one diagonal through the matrix
    for i, (q, r) in enumerate(SHAPES):
        bias = 0.5 if i % 2 else 0.0
        add(f"shape_{q}x{r}", q, r, bias, DP_FUNC)
        n = min(q, r)
        add(f"shape_diag_{q}x{r}", q, r, bias, DP_SSCD if i % 2 else DP_FUNC,
            paths=[(max(0, (q - n) // 2), max(0, (r - n) // 2), f"D{n - 1}", level[bias], 0.05)])
    for bias in (0.0, 0.5):
        tag = "b05" if bias else "b0"
        lv = level[bias]
        # one, two and overlapping planted diagonals
        for rep in range(3):
            add(f"diag1_{tag}_{rep}", 40, 120, bias, DP_FUNC, paths=[(3 + rep, 20 + 7 * rep, "D25", lv, 0.05)])
            add(f"diag2_{tag}_{rep}", 60, 200, bias, DP_SSCD,
                paths=[(2 + rep, 10 + 3 * rep, "D20", lv, 0.05), (30, 120 - 5 * rep, "D25", lv, 0.05)])
            add(f"overlap_{tag}_{rep}", 50, 120, bias, DP_FUNC,
                paths=[(5, 20 + rep, "D30", lv, 0.05), (12, 27 + rep, "D30", lv, 0.05)])
        # a copy at half and double speed: runs of vertical / horizontal steps of diagonal_thres - 1, +0, +1 cells
        for rep, run in enumerate((8, 9, 10, 11)):
            add(f"vrun{run}_{tag}", 80, 120, bias, DP_FUNC, paths=[(2, 5, f"D12,V{run},D12,V{run},D12", lv, 0.05)])
            add(f"hrun{run}_{tag}", 50, 140, bias, DP_FUNC, paths=[(2, 5, f"D12,H{run},D12,H{run},D12", lv, 0.05)])
        add(f"half_{tag}", 70, 100, bias, DP_MODEL, paths=[(2, 4, ",".join(["D1,V1"] * 30), lv, 0.05)])
        add(f"double_{tag}", 50, 130, bias, DP_MODEL, paths=[(2, 4, ",".join(["D1,H1"] * 30), lv, 0.05)])
        # L-shaped paths: adjacent long vertical and horizontal runs (cut_path's crossed ranges)
        add(f"lshape_vh_{tag}", 80, 120, bias, DP_FUNC, paths=[(1, 2, "D10,V15,H15,D12", lv, 0.05)])
        add(f"lshape_hv_{tag}", 80, 120, bias, DP_FUNC, paths=[(1, 2, "D10,H14,V16,D12", lv, 0.05)])
        add(f"lshape_model_{tag}", 64, 64, bias, DP_MODEL, paths=[(0, 0, "D8,V20,H20,D10", lv, 0.05)])
    # entirely below min_sim: acc runs past 255 (an 8-bit counter must saturate, not wrap)
    out.append(_case("below_300x300", "DP", 300, 300, 11, 0.0, DP_FUNC, const=-0.5))
    out.append(_case("below_noise_300x300_g", "DP", 300, 300, 12, 0.0, DP_FUNC, noise=(-0.9, -0.1), grid=True))
    # all-equal matrices: the first-maximum rule everywhere
    for i, (q, r, const) in enumerate([(12, 12, 0.25), (20, 30, -0.5), (33, 9, 0.0), (7, 70, 0.5)]):
        out.append(_case(f"const_{i}", "DP", q, r, 20 + i, 0.0, DP_MODEL if i % 2 else DP_FUNC, const=const))
        out.append(_case(f"const_diag_{i}", "DP", q, r, 30 + i, 0.0, DP_SSCD, const=const,
                         paths=[(0, 0, f"D{min(q, r) - 1}", 0.8, 0.0)]))
    # masks to all -inf before round 100 / does not
    out.append(_case("mask_all_3x9", "DP", 3, 9, 41, 0.0, DP_FUNC, noise=(-0.3, 0.35)))
    out.append(_case("mask_all_6x6_g", "DP", 6, 6, 42, 0.0, DP_MODEL, noise=(-0.3, 0.35), grid=True))
    out.append(_case("mask_not_40x120", "DP", 40, 120, 43, 0.0, dict(DP_FUNC, min_sim=1.9, discontinue=0), noise=(-0.3, 0.35)))
    # many boxes (the GPU test stores two of them)
    out.append(_case("many_boxes", "DP", 100, 160, 44, 0.0, DP_SSCD, noise=(-0.3, 0.35),
                     paths=[(2 + 16 * k, 4 + 25 * k, "D12", 0.8, 0.05) for k in range(6)]))
    # thresholds that are no fp32 numbers, with cells / a sub-path mean exactly at float32(threshold)
    out.append(_case("minsim13_cells", "DP", 40, 60, 45, 0.0, DP_OFFGRID, paths=[(2, 3, "D30", 0.8, 0.05)],
                     exact=[(8, 9, "D5", 1.3), (20, 21, "D3", 1.3)], noise=(-0.3, 0.35)))
    out.append(_case("minsim13_b05", "DP", 40, 60, 46, 0.5, DP_OFFGRID, paths=[(2, 3, "D30", 0.3, 0.05)],
                     exact=[(8, 9, "D5", 1.3), (20, 21, "D3", 1.3)], noise=(-0.8, -0.15)))
    for i, (thr, params) in enumerate([(1.3, DP_OFFGRID), (0.3, DP_AVE03), (1.3, DP_FUNC)]):
        # the whole diagonal of a square matrix at float32(threshold), over a background far below it: the path is the diagonal
        out.append(_case(f"mean_at_{thr}_{i}", "DP", 32, 32, 50 + i, 0.0, params, noise=(-0.99, -0.95), exact=[(0, 0, "D31", thr)]))
        out.append(_case(f"mean_at_{thr}_{i}_64", "DP", 64, 64, 60 + i, 0.0, params, noise=(-0.99, -0.95), exact=[(0, 0, "D63", thr)]))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), "duplicate case names"
    return out


def hv_cases():
    out = []
    seed = 7000
    combos = [(ms, mp, it) for ms in (-1.0, 0.0, 0.2) for mp in (1, 3, 100) for it in (0.3, 0.9)]
    for ci, (min_sim, max_peaks, iou_thresh) in enumerate(combos):
        params = dict(iou_thresh=iou_thresh, min_sim=min_sim, max_peaks=max_peaks)
        tag = f"ms{min_sim}_mp{max_peaks}_iou{iou_thresh}"
        bias = 0.5 if ci % 2 else 0.0
        lo, hi = (-0.8, -0.15) if bias else (-0.3, 0.35)
        lv = 0.3 if bias else 0.8
        for k in range(7):
            seed += 1
            q, r = SHAPES[(ci * 7 + k) % len(SHAPES)]
            if k == 0:      # noise
                c = _case(f"noise_{tag}", "HV", q, r, seed, bias, params, noise=(lo, hi))
            elif k == 1:    # planted diagonals, neighbours of each other (boxes that overlap strongly)
                n = min(q, r)
                c = _case(f"diag_{tag}", "HV", q, r, seed, bias, params, noise=(lo, hi),
                          paths=[(0, 0, f"D{n - 1}", lv, 0.05), (0, 1, f"D{n - 1}", lv, 0.05), (1, 0, f"D{n - 1}", lv, 0.05)])
            elif k == 2:    # exact score ties between diagonals: a constant matrix
                c = _case(f"const_{tag}", "HV", q, r, seed, bias, params, const=0.25 - bias)
            elif k == 3:    # exact ties on the grid
                c = _case(f"grid_{tag}", "HV", q, r, seed, bias, params, noise=(lo, hi), grid=True,
                          paths=[(0, 2, f"D{min(q, r) - 1}", lv, 0.0)])
            elif k == 4:    # all negative
                c = _case(f"neg_{tag}", "HV", q, r, seed, bias, params, noise=(-0.9 - bias, -0.1 - bias))
            elif k == 5:    # the typical shape with two copies
                c = _case(f"typ_{tag}", "HV", 40, 120, seed, bias, params, noise=(lo, hi),
                          paths=[(3, 20, "D25", lv, 0.05), (10, 70, "D28", lv, 0.05)])
            else:           # the corner cells carry the largest values: one-cell diagonals first
                c = _case(f"corner_{tag}", "HV", q, r, seed, bias, params, noise=(lo, hi),
                          paths=[(q - 1, 0, "", 0.95 - bias, 0.0), (0, r - 1, "", 0.9 - bias, 0.0)])
            out.append(c)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), "duplicate case names"
    return out


def cases():
    """The recorded cases, in fixture order (names are unique)."""
    return dp_cases() + hv_cases()
