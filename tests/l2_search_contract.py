"""Executable contract of the exact L2 search (include/vsc_hip.h, above vsc_l2_augment_f32; csrc/l2_search.hip).

  dist(q, r)   c_d of c_0 = +0.0f, t_j = q_j - r_j (one float32 rounding), c_{j+1} = fmaf(t_j, t_j, c_j), j ascending
  knn          the k smallest distances over all rows, ascending, equal distances by ascending id; a NaN or infinite distance is
               never reported; unused slots (FLT_MAX, -1)
  range_search every pair with dist < radius, strict, query-major, ascending id

and the arithmetic the device's SELECTION rests on: the expanded score of the inner-product sweep on augmented operands, the bound
`slack` on |expanded + dist|, and the certificate rule.  The fmaf chains run in tests/l2_search_contract.c (Python 3.10 has no
math.fma, and a float64 emulation double-rounds), compiled here with the host compiler and bound with ctypes.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
FLT_MAX = np.finfo(np.float32).max
MAX_K = 1024


def _load():
    global _lib
    if _lib is None:
        cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("clang")
        assert cc, "the L2 contract needs a host C compiler"
        out = os.path.join(tempfile.mkdtemp(prefix="l2_contract_"), "libl2_contract.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(_HERE, "l2_search_contract.c"), "-o", out, "-lm"])
        _lib = ctypes.CDLL(out)
    return _lib


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def dist_matrix(q, r):
    q, r = _f32(q), _f32(r)
    assert q.ndim == r.ndim == 2 and q.shape[1] == r.shape[1]
    out = np.empty((q.shape[0], r.shape[0]), np.float32)
    _load().l2c_dist_matrix(_p(q), ctypes.c_int64(q.shape[0]), _p(r), ctypes.c_int64(r.shape[0]), ctypes.c_int(q.shape[1]), _p(out))
    return out


def norms(x):
    x = _f32(x)
    out = np.empty(x.shape[0], np.float32)
    _load().l2c_norms(_p(x), ctypes.c_int64(x.shape[0]), ctypes.c_int(x.shape[1]), _p(out))
    return out


def expanded_matrix(q, r):
    """the sweep's score of every pair: ~ -dist, by the fp32 fmaf chain over the d + 2 augmented terms"""
    q, r = _f32(q), _f32(r)
    qn, rn = norms(q), norms(r)
    out = np.empty((q.shape[0], r.shape[0]), np.float32)
    _load().l2c_expanded_matrix(_p(q), _p(qn), ctypes.c_int64(q.shape[0]), _p(r), _p(rn), ctypes.c_int64(r.shape[0]), ctypes.c_int(q.shape[1]),
                                _p(out))
    return out


def knn_from(dist, k, ref_id_offset=0):
    """top-k of a distance matrix by the contract's order"""
    nq, nr = dist.shape
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        ok = np.flatnonzero(np.isfinite(dist[i]))
        order = ok[np.lexsort((ok, dist[i, ok].view(np.uint32)))][:k]        # distances are >= +0: the bit order is the float order
        D[i, :len(order)] = dist[i, order]
        I[i, :len(order)] = order + ref_id_offset
    return D, I


def knn(q, r, k, ref_id_offset=0):
    return knn_from(dist_matrix(q, r), k, ref_id_offset)


def range_from(dist, radius, ref_id_offset=0):
    hit = np.isfinite(dist) & (dist < np.float32(radius))
    lims = np.zeros(dist.shape[0] + 1, np.int64)
    np.cumsum(hit.sum(1), out=lims[1:])
    rows, ids = np.nonzero(hit)                                              # row-major: query-major, ascending id
    return lims, dist[rows, ids], ids.astype(np.int64) + ref_id_offset


def range_search(q, r, radius, ref_id_offset=0):
    return range_from(dist_matrix(q, r), radius, ref_id_offset)


def probe_size(k, nr):
    """ranks of the first probe"""
    return int(min(max(k + 8, 2 * k), MAX_K, nr))


def wide_probe_size(k, nr):
    """ranks of the one wider probe of the rows the first cannot certify; 0: there is none (it would hold the whole bank, which
    the direct path answers without a bound)"""
    kk = probe_size(k, nr)
    wide = min(max(4 * kk, 256), MAX_K)
    return wide if kk < wide < nr else 0


def slack(d, qn2, rmax2):
    """The device's bound on |expanded score + chain distance| over a bank whose largest computed |r|^2 is rmax2, for a query of computed
    |q|^2 = qn2 (csrc/l2_search.hip l2_slack): (3d + 8) (2^-24 (|q| + max|r|)^2 1.01 + 2^-126); inf where there is none."""
    qn2, rmax2 = float(qn2), float(rmax2)
    if not (0.0 <= qn2 <= float(FLT_MAX) and 0.0 <= rmax2 <= float(FLT_MAX)):
        return float("inf")
    S = (np.sqrt(qn2) + np.sqrt(rmax2)) ** 2
    if not S < 1.0e38:
        return float("inf")
    terms = 3.0 * d + 8.0
    return float(terms * 2.0 ** -24 * S * 1.01 + terms * 2.0 ** -126)


def certified(q, r, k, kk=None, slack_scale=1.0):
    """-> bool [nq]: the rows whose probe of kk ranks (default: the first probe's) is certified, by the reference arithmetic alone:
    the kk best expanded scores (descending, lower id first) are the probe, D_k the k-th smallest chain distance inside it, and the
    row is certified when D_k < -s'_kk - slack strictly (in float64, as the device compares), or when the probe holds the whole
    bank.  slack_scale: the margin of a statement about the device, whose norms are summed in another order."""
    q, r = _f32(q), _f32(r)
    nr, d = r.shape
    kk = probe_size(k, nr) if kk is None else kk
    if kk >= nr:
        return np.ones(q.shape[0], bool)
    e, dist = expanded_matrix(q, r), dist_matrix(q, r)
    qn, rmax = norms(q), norms(r).max()
    out = np.zeros(q.shape[0], bool)
    for i in range(q.shape[0]):
        probe = np.lexsort((np.arange(nr), -e[i].astype(np.float64)))[:kk]
        dk = np.sort(dist[i, probe][np.isfinite(dist[i, probe])])
        s = slack(d, qn[i], rmax) * slack_scale
        out[i] = len(dk) >= k and np.isfinite(e[i, probe[-1]]) and np.isfinite(s) and float(dk[k - 1]) < -float(e[i, probe[-1]]) - s
    return out


def far_cluster(seed=5, nr=300, nq=6, d=16, norm=200.0, spread=1e-2):
    """the case the host form's heuristic probe cannot see: a tight cluster far from the origin, queries from the same cluster"""
    rng = np.random.RandomState(seed)
    centre = rng.randn(d)
    centre *= norm / np.linalg.norm(centre)
    r = (centre + spread * rng.randn(nr, d)).astype(np.float32)
    q = (centre + spread * rng.randn(nq, d)).astype(np.float32)
    return q, r


def middle_cluster(seed=9, nr=4000, nq=12, d=2, norm=1.5, spread=1e-2):
    """between the two: a cluster whose expanded-form rounding exceeds the gap between the 5th and the 13th neighbour and, for most
    rows, stays below the gap to the 256th -- the first probe cannot certify, the wider one can"""
    return far_cluster(seed, nr, nq, d, norm, spread)


def path_bounds(q, r, k):
    """What the reference arithmetic says about the device's path report, with a factor 2 of margin on slack either way (the device
    sums its norms in another order): -> (most rows the first probe can certify, fewest it must, fewest the wider probe must)."""
    wide = wide_probe_size(k, len(r))
    first_hi, first_lo = certified(q, r, k, slack_scale=0.5), certified(q, r, k, slack_scale=2.0)
    wide_sure = certified(q, r, k, kk=wide, slack_scale=2.0) & ~first_hi if wide else np.zeros(len(q), bool)
    return int(first_hi.sum()), int(first_lo.sum()), int(wide_sure.sum())


def unit(seed, n, d):
    x = np.random.RandomState(seed).randn(n, d)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def flat_l2_data():
    """the data of tests/test_gpu_knn.py::test_flat_l2_index"""
    rng = np.random.RandomState(3)
    r = (rng.randn(500, 24) * 3).astype(np.float32)
    q = (rng.randn(17, 24) * 3).astype(np.float32)
    q[5] = r[77]
    return q, r
