"""Operands shared by tests/test_score_norm_emulated.py (the kernels compiled for the CPU) and tests/test_gpu_score_norm.py (the
device): the shapes at which the kernels take another path -- one row, fewer columns than a wave, the 64-column workgroup edge,
the 64-row tile edge, padded strides, every summation form of the bias -- generated from seeds."""
import numpy as np

TILE = 64       # VSC_COLUMN_VAR_TILE

# (n, d, ld): the small shapes, then the edges of the row tile
VAR_SHAPES = [(1, 1, 1), (2, 3, 3), (7, 64, 64), (513, 65, 65), (4099, 130, 136),
              (TILE - 1, 5, 8), (TILE, 5, 5), (TILE + 1, 5, 5), (2 * TILE, 66, 66), (2 * TILE + 1, 3, 3)]
VAR_SHAPE_LARGE = (20000, 512, 512)

ROWS_D = [2, 5, 64, 65, 129, 512, 513]
NKS = [1, 2, 7, 8, 9, 10, 16, 17]


def offset_rows(n, d, ld=None, seed=0):
    """[n, ld] float32 whose first d columns have their mean at ten standard deviations (any other summation order shows in the
    last bits of the sum and of the centred squares) and whose padding is NaN -- a kernel that read it would show it."""
    rs = np.random.RandomState(seed + 31 * n + d)
    ld = d if ld is None else ld
    x = np.full((n, ld), np.nan, np.float32)
    scale = rs.uniform(0.01, 1.0, d)
    x[:, :d] = (rs.standard_normal((n, d)) * scale + 10.0 * scale * rs.choice([-1.0, 1.0], d)).astype(np.float32)
    return x


def drops(d):
    return sorted({c for c in (-1, 0, 63, 64, d - 1) if c < d})


def descriptor_rows(d, ldx, seed=0):
    """six rows [6, ldx]: random rows of different scale, a zero row (row 2) and a row of 1e-30 (row 4: every square underflows to
    zero, the row must come back unchanged); NaN padding."""
    rs = np.random.RandomState(seed + d)
    x = np.full((6, ldx), np.nan, np.float32)
    x[:, :d] = (rs.standard_normal((6, d)) * np.array([1.0, 1e-3, 0.0, 37.0, 0.0, 1.0])[:, None]).astype(np.float32)
    x[4, :d] = np.float32(1e-30)
    return x


def topk_scores(nq, nk, ldk, seed=0):
    """[nq, ldk] descending-looking scores near 1 (the sums round at every step); NaN padding; and a gate with every third row set"""
    rs = np.random.RandomState(seed + 7 * nk)
    s = np.full((nq, ldk), np.nan, np.float32)
    s[:, :nk] = -np.sort(-(rs.standard_normal((nq, nk)) * 0.05 + 0.9).astype(np.float32), axis=1)
    gate = (np.arange(nq) % 3 == 1).astype(np.uint8)
    return s, gate
