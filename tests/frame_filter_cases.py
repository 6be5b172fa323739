"""Seeded cases of the near-duplicate frame filter (tests/frame_filter_contract.py, csrc/frame_filter.hip).  The matrices are PLANTED,
not products of descriptors, so they are asymmetric: a kernel that reads column i where row i is meant, or takes mean(1) for
mean(0), fails on them (test_frame_filter_cpu.py checks that the transposed matrix gives another answer).

A case is a dict: name; s float32 [L, L]; thr (compared as float32); tie_free -- the contract's means are pairwise distinct, so the
host path (greedy_select) has a defined answer and must give the contract's.  Tied cases are compared with the contract only."""
import functools

import numpy as np

import frame_filter_contract as C

THR = 0.975                                           # FRAME_THRESHOLD of src/query_postprocess.py
SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 300)
# more than one bit word per lane's worth of columns beyond 1 024, and -- with 1 088 and 1 089 -- the two sides of the size at which
# the adjacency bits leave LDS for the scratch (8 L (1 + ceil(L / 64)) <= VSC_FRAME_FILTER_LDS_BYTES holds up to 1 088)
BIG_SIZES = (1088, 1089, 1100)
EMULATED_MAX = 300                                    # the emulation runs one OS thread per GPU thread
ONE = np.float32(1)
ABOVE, BELOW = np.nextafter(np.float32(THR), ONE), np.nextafter(np.float32(THR), np.float32(0))
DIAGS = np.array([ONE, np.nextafter(ONE, np.float32(0)), np.nextafter(ONE, np.float32(2))], np.float32)   # 1.0, 1 - ulp, 1 + ulp


def _planted(rng, L):
    """random asymmetric background below the threshold, the three diagonals in turn, then near-duplicates: one-sided and two-sided
    pairs at 0.99, exactly at the threshold (stays), one ulp above (goes) and one ulp below, and chains a~b, b~c without a~c"""
    s = rng.uniform(-0.2, 0.9, (L, L)).astype(np.float32)
    d = np.arange(L)
    s[d, d] = DIAGS[d % 3]
    if L < 2:
        return s
    values = np.array([0.99, np.float32(THR), ABOVE, BELOW, 0.99, ABOVE], np.float32)
    for k in range(max(L // 3, 1)):
        i, j = rng.choice(L, 2, replace=False)
        s[i, j] = values[k % len(values)]
        if k % 2:
            s[j, i] = values[(k // 2) % len(values)]
    for _ in range(L // 8):
        if L >= 3:
            a, b, c = rng.choice(L, 3, replace=False)
            s[a, b] = s[b, a] = s[b, c] = s[c, b] = np.float32(0.99)
            s[a, c] = s[c, a] = np.float32(0.3)
    return s


def tie_free(name, L, seed, thr=THR, make=_planted):
    """the first seed from `seed` on whose matrix has pairwise distinct means (in practice: the first)"""
    for bump in range(64):
        s = make(np.random.default_rng([seed + 1000 * bump, L]), L)
        if len(np.unique(C.means(s))) == L:
            return dict(name=name, s=s, thr=thr, tie_free=True)
    raise AssertionError(f"{name}: no tie-free matrix in 64 seeds")


def _tie_columns(s, j1, j2, k1, k2):
    """make column j2 of v = column j1 of v, bit for bit: the two diagonal entries involved become k / 1024, which 1 + x and
    (1 + x) - 1 carry exactly"""
    s[j1, j1] = ONE + np.float32(k1 / 1024)
    s[j2, j1] = np.float32(k2 / 1024)
    s[:, j2] = s[:, j1]
    s[j1, j2] = np.float32(k1 / 1024)                 # v[j1][j2] = v[j1][j1]
    s[j2, j2] = ONE + np.float32(k2 / 1024)           # v[j2][j2] = v[j2][j1]


def tied_columns(name, L, seed):
    """the planted matrix with L // 4 disjoint pairs of duplicated columns: equal means two by two"""
    rng = np.random.default_rng([seed, L, 7])
    s = _planted(rng, L)
    cols = rng.permutation(L)[: 2 * (L // 4)]
    for j1, j2 in cols.reshape(-1, 2):
        _tie_columns(s, j1, j2, int(rng.integers(-50, 50)), int(rng.integers(-50, 50)))
    m = C.bits(C.means(s))
    assert L < 4 or all(m[a] == m[b] for a, b in cols.reshape(-1, 2)), name
    return dict(name=name, s=s, thr=THR, tie_free=L < 4)


def tied_rule_decides(name, L, seed):
    """Tied pairs (j1, j2) whose ORDER decides what is kept.  Threshold 0.02, background below it.  v[j1][j1] = v[j1][j2] = 30 / 1024
    is above it: j1, when visited, removes itself and j2.  Row j2 is above it at one ordinary frame d only.  j2 before j1 (the
    contract, when j2 > j1): d goes.  j1 before j2: j2 is never visited and d stays."""
    rng = np.random.default_rng([seed, L, 11])
    s = rng.uniform(-0.9, -0.1, (L, L)).astype(np.float32)
    d = np.arange(L)
    s[d, d] = ONE
    cols = rng.permutation(L)[: 3 * (L // 6)].reshape(-1, 3)
    for j1, j2, dd in cols:
        _tie_columns(s, j1, j2, 30, -10)
    for j1, j2, dd in cols:
        s[j2, dd] = np.float32(0.5)
    m = C.bits(C.means(s))
    assert all(m[a] == m[b] for a, b, _ in cols), name
    return dict(name=name, s=s, thr=0.02, tie_free=False)


def constant(name, L, c):
    """every similarity the same value: with c = 0.5 or 1.0 every partial sum is exact, so all L means are bit-equal"""
    return dict(name=name, s=np.full((L, L), c, np.float32), thr=THR, tie_free=L < 2)


def _none_above(rng, L):
    s = rng.uniform(-0.2, 0.9, (L, L)).astype(np.float32)
    s[np.arange(L), np.arange(L)] = ONE
    return s


def _all_above(rng, L):
    s = rng.uniform(0.98, 0.999, (L, L)).astype(np.float32)
    s[np.arange(L), np.arange(L)] = ONE
    return s


def _negative_thr(rng, L):
    """threshold -0.05: a frame with diagonal 1.0 (v = 0) removes ITSELF when visited; every second frame has diagonal 0.9 (v = -0.1)
    and does not"""
    s = rng.uniform(-0.9, 0.0, (L, L)).astype(np.float32)
    s[rng.random((L, L)) < 0.9] -= np.float32(0.2)
    d = np.arange(L)
    s[d, d] = np.where(d % 2 == 0, ONE, np.float32(0.9))
    return s


def _zero_thr_diag(rng, L):
    """threshold 0.0 against v[i][i] = 0, -2^-24, +2^-23: only the frames with diagonal 1 + ulp remove themselves"""
    s = rng.uniform(-0.9, -0.1, (L, L)).astype(np.float32)
    d = np.arange(L)
    s[d, d] = DIAGS[d % 3]
    for _ in range(L // 5):
        i, j = rng.choice(L, 2, replace=False)
        s[i, j] = np.float32(0.25)
    return s


def _freeze(case):
    case["s"].setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for L in SIZES + BIG_SIZES:
        out.append(tie_free(f"planted_{L}", L, seed=1))
    for L in (2, 63, 64, 65, 129, 256, 300, 1100):
        out.append(tied_columns(f"tied_columns_{L}", L, seed=2))
    for L in (6, 65, 257):
        out.append(tied_rule_decides(f"tied_rule_{L}", L, seed=3))
    out.append(constant("constant_half_2", 2, 0.5))
    out.append(constant("constant_half_128", 128, 0.5))
    out.append(constant("constant_half_300", 300, 0.5))
    out.append(constant("constant_one_65", 65, 1.0))
    out.append(constant("constant_one_300", 300, 1.0))
    out.append(tie_free("none_above_65", 65, seed=4, make=_none_above))
    out.append(tie_free("all_above_129", 129, seed=5, make=_all_above))
    out.append(tie_free("negative_thr_64", 64, seed=6, thr=-0.05, make=_negative_thr))
    out.append(tie_free("negative_thr_257", 257, seed=6, thr=-0.05, make=_negative_thr))
    out.append(tie_free("zero_thr_diag_63", 63, seed=7, thr=0.0, make=_zero_thr_diag))
    return tuple(_freeze(c) for c in out)


def names(max_rows=None):
    return [c["name"] for c in cases() if max_rows is None or len(c["s"]) <= max_rows]


def get(name):
    return next(c for c in cases() if c["name"] == name)


def batch(case_names, seed=0):
    """The cases' matrices in ONE flat buffer at element offsets that are no multiples of 64 (odd gaps of NaN between them)
    -> (flat float32, items int64 [n, 2] = (element offset, rows)).  All cases of a batch share one threshold."""
    rng = np.random.default_rng([seed, len(case_names)])
    parts, items, at = [], [], 0
    for name in case_names:
        gap = int(rng.integers(1, 32)) * 2 + 1
        parts.append(np.full(gap, np.nan, np.float32))
        at += gap
        s = get(name)["s"]
        items.append((at, len(s)))
        parts.append(s.reshape(-1))
        at += s.size
    parts.append(np.full(5, np.nan, np.float32))
    return np.concatenate(parts), np.asarray(items, np.int64).reshape(-1, 2)


def default_thr_names(max_rows=None):
    """the cases at the default threshold, in an order that mixes sizes (empty ones included)"""
    sel = [n for n in names(max_rows) if get(n)["thr"] == THR]
    return sel[1::2] + sel[0::2]


def many_small(n=131, seed=9):
    """more items than one launch holds (VSC_FRAME_FILTER_CHUNK = 128): planted matrices of 0 .. 6 rows
    -> (flat, items, [matrix per item])"""
    rng = np.random.default_rng([seed, n])
    mats = [_planted(rng, int(rng.integers(0, 7))) for _ in range(n)]
    parts, items, at = [], [], 0
    for s in mats:
        parts.append(np.full(3, np.nan, np.float32))
        at += 3
        items.append((at, len(s)))
        parts.append(s.reshape(-1))
        at += s.size
    return np.concatenate(parts), np.asarray(items, np.int64).reshape(-1, 2), mats
