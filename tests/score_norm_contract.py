"""Executable contract of the device score normalisation (include/vsc_hip.h: vsc_column_var_f32, vsc_score_norm_rows_f32,
vsc_score_norm_bias_f32).  Plain numpy, every rounding written out in the order the kernels keep: the descriptors of the device
path are the BYTES the numpy path writes, so "close" is not a result here -- compare `bits()`.

What each function pins down, and what it is checked against (tests/test_score_norm_cpu.py):
  column_var    == x.var(axis=0) of a C-contiguous float32 [n, d] array
  bias          == -beta * sims[:, :nk].mean(axis=1)
  rows          == np.concatenate([normalize(np.delete(x, drop, axis=1)), last], axis=1)
  l2_normalize  == l2_normalize_kernel (csrc/elementwise.hip) -- checkable on the device only (tests/test_gpu_score_norm.py)
"""
import numpy as np

F32, F64 = np.float32, np.float64
MAX_NK = 128          # numpy's pairwise block: a longer row sum recurses, the contract ends here
WAVE = 64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def column_sum_chain(rows_iter, first):
    """((v0 + v1) + v2) + ... over float32 rows, ascending."""
    acc = first.astype(F32, copy=True)
    for v in rows_iter:
        acc = acc + v
    return acc


def column_var(x):
    """numpy's var(axis=0) of a C-contiguous float32 [n, d] array: one chain per column over the rows in ascending order."""
    x = np.asarray(x, F32)
    n = x.shape[0]
    if x.ndim != 2 or n < 1:
        raise ValueError("column_var: at least one row")
    s = column_sum_chain((x[r] for r in range(1, n)), x[0])
    mean = (s.astype(F64) / F64(n)).astype(F32)

    def sq(r):
        dl = x[r] - mean              # fl(x - mean)
        return dl * dl                # fl(. * .): a separate rounding, no fused multiply-add

    acc = column_sum_chain((sq(r) for r in range(1, n)), sq(0))
    return (acc.astype(F64) / F64(n)).astype(F32)


def low_variance_dim(x):
    """np.argmin on the host: the first minimum wins, NaN as numpy treats it."""
    return int(np.argmin(column_var(x)))


def row_sum(a, nk):
    """numpy's pairwise sum of a[:, :nk] along the row, 1 <= nk <= 128."""
    if not 1 <= nk <= MAX_NK:
        raise ValueError(f"row_sum: nk {nk} outside [1, {MAX_NK}]")
    a = np.asarray(a, F32)
    if nk < 8:
        res = a[:, 0].copy()
        for i in range(1, nk):
            res = res + a[:, i]
        return res
    r = [a[:, j].copy() for j in range(8)]
    i = 8
    while i < nk - nk % 8:
        for j in range(8):
            r[j] = r[j] + a[:, i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(i, nk):
        res = res + a[:, i]
    return res


def row_mean(a, nk):
    return (row_sum(a, nk).astype(F64) / F64(nk)).astype(F32)


def bias(topk, nk, beta, gate=None):
    """fl32((float)(-beta) * mean); a gated row is exactly -100.0f."""
    out = F32(-beta) * row_mean(topk, nk)
    assert out.dtype == F32
    if gate is not None:
        out = np.where(np.asarray(gate) != 0, F32(-100.0), out)
    return out


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding: the product of two float32 is exact in float64; the float64 sum is rounded to odd (so the
    second rounding, to float32, cannot land on the wrong side of a tie) from its two-sum error."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    t = p + c
    bb = t - p
    e = (p - (t - bb)) + (c - bb)
    even = (t.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(t)
    t = np.where(fix, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
    return t.astype(F32)


def l2_normalize(x):
    """l2_normalize_kernel on the rows of a contiguous float32 [n, w] array: lane l sums the squares of columns l, l + 64, ... as
    fmaf(x, x, ss); xor butterfly 32 ... 1; nrm = sqrtf(ss); a row with nrm == 0 stays as it is, otherwise x / nrm."""
    x = np.asarray(x, F32)
    n, w = x.shape
    ss = np.zeros((n, WAVE), F32)
    for k in range(0, w, WAVE):
        chunk = x[:, k:k + WAVE]
        m = chunk.shape[1]
        ss[:, :m] = fma32(chunk, chunk, ss[:, :m])
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[:, lanes ^ o]
    nrm = np.sqrt(ss[:, :1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(nrm == 0, x, x / nrm).astype(F32)


def rows(x, drop=-1, normalize=True, append=0, last=None, normalize_fn=l2_normalize):
    """out[:, c'] over the logical columns c' = c - (c > drop) of the columns c != drop, normalised as a narrowed contiguous row,
    then the appended column: 0 none, 1 the constant 1.0f, 2 last[row]."""
    x = np.asarray(x, F32)
    n, d = x.shape
    if not -1 <= drop < d or append not in (0, 1, 2):
        raise ValueError("rows: drop in [-1, d), append in {0, 1, 2}")
    w = d - (drop >= 0)
    narrowed = np.empty((n, w), F32)
    for c in range(d):
        if c != drop:
            narrowed[:, c - (drop >= 0 and c > drop)] = x[:, c]
    if normalize:
        narrowed = np.asarray(normalize_fn(narrowed), F32)
    if append == 0:
        return narrowed
    out = np.empty((n, w + 1), F32)
    out[:, :w] = narrowed
    out[:, w] = F32(1.0) if append == 1 else np.asarray(last, F32).reshape(n)
    return out
