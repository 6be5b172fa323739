"""Similarity matrices of the temporal-network (TN) alignment fixture (tests/golden/tn_align.json).

Every matrix is rebuilt from its recipe with `np.random.RandomState` and elementwise fp32 operations only (no matmul, no
BLAS), so any machine reproduces the same bytes; each recorded case carries the SHA-256 of its input.  The fixture
generator (tests/golden/gen_tn_golden.py) and the GPU tests (tests/test_gpu_tn_align.py) both build their inputs here.

A case is a dict: name, q, r, seed, bias (0.5 = sscd_baseline's score-normalised branch on raw scores, 0.0 = its
normalised-feature branch on similarities in [-1, 1]), the TN parameters and the recipe keys read by `matrix`.
"""
import hashlib

import numpy as np

TN_SSCD = dict(tn_max_step=5, tn_top_k=5, max_path=10, min_sim=0.2, min_length=4, max_iou=0.3)     # sscd_baseline.py:118-136
TN_DEFAULT = dict(tn_max_step=10, tn_top_k=5, max_path=10, min_sim=0.2, min_length=5, max_iou=0.3)  # TnVtaModel defaults


def _noise(rs, q, r, bias):
    """Background scores: raw-score range around 0 for the biased branch, normalised similarities otherwise."""
    if bias:
        return (rs.uniform(-0.45, 0.05, size=(q, r))).astype(np.float32)
    return (rs.uniform(-0.3, 0.35, size=(q, r))).astype(np.float32)


def _plant(m, rs, q0, r0, length, stretch, level):
    """A copied segment: query frame q0 + i matches reference frame r0 + floor(i * stretch) (stretch < 1 repeats reference
    frames, > 1 skips them)."""
    q, r = m.shape
    for i in range(length):
        qi, ri = q0 + i, r0 + int(np.floor(i * stretch))
        if 0 <= qi < q and 0 <= ri < r:
            m[qi, ri] = np.float32(level) + np.float32(rs.uniform(-0.05, 0.05))


def matrix(case):
    """The unbiased fp32 [q, r] matrix of one case."""
    rs = np.random.RandomState(case["seed"])
    q, r, bias = case["q"], case["r"], case["bias"]
    m = _noise(rs, q, r, bias)
    level = 0.45 if bias else 0.8
    for seg in case.get("segments", ()):
        _plant(m, rs, *seg, level=level)
    if case.get("quant"):                     # exact ties everywhere: values on a grid of 1/quant
        m = (np.round(m * np.float32(case["quant"])) / np.float32(case["quant"])).astype(np.float32)
    for src, dst in case.get("dup_rows", ()):
        m[dst] = m[src]
    for src, dst in case.get("dup_cols", ()):
        m[:, dst] = m[:, src]
    if case.get("const") is not None:         # every value equal: ties in top-K order, among predecessors, at the maximum
        m[:] = np.float32(case["const"])
        for seg in case.get("segments", ()):
            for i in range(seg[2]):
                qi, ri = seg[0] + i, seg[1] + int(np.floor(i * seg[3]))
                if 0 <= qi < q and 0 <= ri < r:
                    m[qi, ri] = np.float32(level)
    return np.ascontiguousarray(m, dtype=np.float32)


def digest(m):
    return hashlib.sha256(np.ascontiguousarray(m, dtype=np.float32).tobytes()).hexdigest()


def _case(name, q, r, seed, bias, params=TN_SSCD, **recipe):
    return dict(name=name, q=q, r=r, seed=seed, bias=bias, params=dict(params), **recipe)


def cases():
    """The recorded cases, in fixture order (names are unique)."""
    out = []
    seed = 1000
    for bias in (0.5, 0.0):
        tag = "b05" if bias else "b0"
        # one planted diagonal copy
        for i, (q, r) in enumerate([(30, 60), (60, 180), (40, 40), (80, 120), (25, 300), (50, 90)]):
            for rep in range(3):
                seed += 1
                rs = np.random.RandomState(seed)
                ln = int(rs.randint(q // 3, q))
                q0 = int(rs.randint(0, q - ln + 1))
                r0 = int(rs.randint(0, max(1, r - ln)))
                out.append(_case(f"diag1_{tag}_{q}x{r}_{rep}", q, r, seed, bias, segments=[(q0, r0, ln, 1.0)]))
        # two copies, and two overlapping copies
        for rep in range(6):
            seed += 1
            out.append(_case(f"diag2_{tag}_{rep}", 60, 200, seed, bias,
                             segments=[(2 + rep, 10 + 3 * rep, 20, 1.0), (30, 120 - 5 * rep, 25, 1.0)]))
            out.append(_case(f"overlap_{tag}_{rep}", 50, 120, seed + 5000, bias,
                             segments=[(5, 20 + rep, 30, 1.0), (12, 27 + rep, 30, 1.0)]))
        # time-stretched copies: repeated (stretch < 1) and skipped (stretch > 1) reference frames
        for rep, stretch in enumerate([0.5, 0.75, 1.5, 2.0, 3.0, 0.34, 1.25, 4.0]):
            seed += 1
            out.append(_case(f"stretch_{tag}_{rep}", 60, 240, seed, bias, segments=[(5, 12, 40, stretch)]))
        # exact ties: quantised values (ties in top-K order, among predecessors, at the maximum)
        for rep, quant in enumerate([4, 8, 16, 2, 32, 8]):
            seed += 1
            out.append(_case(f"quant_{tag}_{rep}", 40, 80, seed, bias, quant=quant, segments=[(3, 9, 25, 1.0)]))
        # duplicated rows and columns (identical frames)
        for rep in range(5):
            seed += 1
            out.append(_case(f"dup_{tag}_{rep}", 40, 90, seed, bias, segments=[(4, 10, 30, 1.0)],
                             dup_rows=[(10, 11), (10, 12), (20, 21)], dup_cols=[(15 + rep, 16 + rep), (40, 41), (40, 42)]))
        # constant matrices with a planted diagonal: every top-K / predecessor / maximum is a tie
        for rep, (q, r, const) in enumerate([(20, 30, 0.3), (12, 12, 0.25), (30, 10, 0.3), (15, 40, -0.1)]):
            seed += 1
            out.append(_case(f"const_{tag}_{rep}", q, r, seed, bias, const=const,
                             segments=[(2, 3, 8, 1.0)]))
        # edge shapes
        seed += 1
        out += [_case(f"q1_{tag}", 1, 50, seed, bias),
                _case(f"r1_{tag}", 30, 1, seed + 1, bias),
                _case(f"rltk_{tag}", 30, 3, seed + 2, bias, segments=[(0, 0, 3, 1.0)]),
                _case(f"r4_{tag}", 25, 4, seed + 3, bias, segments=[(2, 0, 4, 1.0)]),
                _case(f"qlestep_{tag}", 5, 5, seed + 4, bias, segments=[(0, 0, 5, 1.0)]),
                _case(f"qlestep2_{tag}", 4, 40, seed + 5, bias, segments=[(0, 0, 4, 1.0)]),
                _case(f"q2_{tag}", 2, 3, seed + 6, bias),
                _case(f"q1r1_{tag}", 1, 1, seed + 7, bias),
                _case(f"lastnode_{tag}", 30, 30, seed + 8, bias, segments=[(0, 0, 30, 1.0)]),
                _case(f"lastnode2_{tag}", 20, 60, seed + 9, bias, segments=[(5, 45, 15, 1.0)])]
        seed += 10
        # TnVtaModel defaults: step 10, min_length 5
        for rep, (q, r, stretch) in enumerate([(60, 180, 1.0), (80, 200, 2.0), (50, 100, 0.5), (120, 600, 1.0),
                                               (40, 80, 3.0)]):
            seed += 1
            out.append(_case(f"tnvta_{tag}_{rep}", q, r, seed, bias, params=TN_DEFAULT,
                             segments=[(3, 7, q // 2, stretch), (q // 2 + 5, r // 2, q // 3, 1.0)]))
        for rep in range(3):
            seed += 1
            out.append(_case(f"tnvta_quant_{tag}_{rep}", 40, 90, seed, bias, params=TN_DEFAULT, quant=8,
                             segments=[(2, 5, 30, 1.0)]))
    # pure noise, other parameter sets
    for rep in range(6):
        seed += 1
        out.append(_case(f"noise_{rep}", 30 + 10 * rep, 60 + 20 * rep, seed, 0.5 if rep % 2 else 0.0))
    for rep, p in enumerate([dict(tn_max_step=3, tn_top_k=3, max_path=5, min_sim=0.1, min_length=2, max_iou=0.5),
                             dict(tn_max_step=2, tn_top_k=8, max_path=4, min_sim=0.3, min_length=1, max_iou=0.1),
                             dict(tn_max_step=6, tn_top_k=9, max_path=12, min_sim=0.15, min_length=3, max_iou=0.3),
                             dict(tn_max_step=1, tn_top_k=5, max_path=2, min_sim=0.2, min_length=0, max_iou=0.3),
                             dict(tn_max_step=17, tn_top_k=4, max_path=3, min_sim=0.2, min_length=5, max_iou=0.6),
                             dict(tn_max_step=5, tn_top_k=1, max_path=10, min_sim=0.0, min_length=4, max_iou=0.3)]):
        seed += 1
        out.append(_case(f"params_{rep}", 50, 120, seed, 0.5, params=p, segments=[(4, 8, 30, 1.0), (20, 70, 20, 2.0)]))
    # a few large pairs
    out.append(_case("large_300x1200", 300, 1200, 77, 0.5, segments=[(10, 100, 200, 1.0), (40, 700, 120, 0.5)]))
    out.append(_case("large_1000x4000", 1000, 4000, 78, 0.0, segments=[(50, 300, 600, 1.0), (700, 3000, 250, 2.0)]))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), "duplicate case names"
    return out


def by_name():
    return {c["name"]: c for c in cases()}
