"""Executable statement of the two selection contracts of include/vsc_hip.h (vsc_global_topk_f32, vsc_pair_first_hits) in
numpy.  Test helper only: the GPU tests compare the kernels with it bit for bit, the CPU tests compare it with what the host
path of vsc/index.py produces; the project never runs it in place of the kernels."""
import numpy as np


def global_topk(scores, ids, want, rows=None, row_stride=None):
    """-> (rows, ids, scores) of the min(want, valid) best entries, best first, equal scores in input order.
    scores / ids: flat, or one [nq, k] probe (then the row of an entry is its first index unless `rows` is given);
    row_stride: the row of flat entry p is p // row_stride."""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    assert scores.shape == ids.shape
    if rows is None:
        stride = row_stride if row_stride is not None else (scores.shape[1] if scores.ndim == 2 else 1)
        rows = np.arange(scores.size, dtype=np.int64) // max(int(stride), 1)
    rows = np.asarray(rows, np.int64).reshape(-1)
    scores, ids = scores.reshape(-1), ids.reshape(-1)
    valid = np.flatnonzero(ids >= 0)                      # padding is no candidate
    # a stable descending sort by VALUE: -0.0 == +0.0 compare equal, so input order decides between them
    order = valid[np.argsort(-scores[valid], kind="stable")][: max(int(want), 0)]
    return rows[order], ids[order], scores[order]


def pair_first_hits(rows, ids, q_video, r_video, n_r_videos, limit=None):
    """-> ascending positions of the first hit of every distinct (q video, r video) pair of a best-first list, cut to `limit`."""
    rows, ids = np.asarray(rows, np.int64), np.asarray(ids, np.int64)
    if len(rows) == 0:
        return np.zeros(0, np.int64)
    key = np.asarray(q_video, np.int64)[rows] * np.int64(n_r_videos) + np.asarray(r_video, np.int64)[ids]
    _, first = np.unique(key, return_index=True)
    first.sort()
    return first[: None if limit is None or limit < 0 else int(limit)].astype(np.int64)


def bits(x):
    """float32 array -> its uint32 bit patterns (scores are compared exactly)"""
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
