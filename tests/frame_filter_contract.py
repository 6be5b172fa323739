"""Executable contract of the near-duplicate frame filter (vsc_frame_filter_f32 in include/vsc_hip.h; the host path is
src/query_postprocess.py: greedy_select / select_frames, the reference infer/extract_query_feats.py:190-199), in numpy with every
operation written out.

Input: one video's float32 matrix s [L, L] as vsc_pair_similarity_f32 wrote it, and the threshold as a float32.
  v[i][j] = s[i][j] for i != j; v[i][i] = s[i][i] - 1.0f (a float32 subtraction: the host path subtracts np.eye(L, float32)).
  mean[j] = (((v[0][j] + v[1][j]) + v[2][j]) + ...) / (float)L: one float32 add chain per column, rows ascending, then one IEEE
    float32 division.  The chain STARTS from v[0][j]; numpy's reduction starts from +0.0.  The two differ only where every addend
    is -0.0 (sum -0.0 against +0.0), and no column is like that: it holds v[j][j] = s[j][j] - 1.0f, which is never -0.0.  numpy
    divides the float32 sums in float64 and rounds to float32, which for float32 operands and L < 2^24 is the float32 division
    (test_frame_filter_cpu.py holds both facts against sim.mean(0)).
  visit order: mean descending, EQUAL means in descending index: mean.argsort(kind="stable")[::-1].  -0.0 equals +0.0.  The host
    path's argsort() is numpy's unstable sort: among equal means its order depends on the numpy build, so the two agree exactly where
    a video's means are pairwise distinct.  NaN is outside the contract.
  greedy pass: removed = {}; for i in visit order, unless i is removed: every j with v[i][j] > thr (ROW i, float32 compare, j = i
    included) becomes removed.  kept = the indices not removed, ascending."""
import numpy as np


def diagonal_removed(s):
    """v of the contract"""
    s = np.asarray(s, np.float32)
    v = s.copy()
    d = np.arange(len(s))
    v[d, d] = s[d, d] - np.float32(1.0)
    return v


def means(s):
    """float32 [L]: the explicit chain and one float32 division"""
    v = diagonal_removed(s)
    L = len(v)
    if L == 0:
        return np.zeros(0, np.float32)
    acc = v[0].copy()
    for i in range(1, L):
        acc = acc + v[i]                       # float32 + float32, element-wise: one rounding per row
    assert acc.dtype == np.float32
    return acc / np.float32(L)


def order(mean):
    """int64 [L]: descending mean, equal means in descending index"""
    return np.asarray(mean).argsort(kind="stable")[::-1]


def keep(s, thr):
    """-> (kept indices ascending int64, mean float32 [L], visit order int64 [L])"""
    v = diagonal_removed(s)
    m = means(s)
    o = order(m)
    thr = np.float32(thr)
    removed = np.zeros(len(v), bool)
    for i in o:
        if removed[i]:
            continue
        removed |= v[i] > thr
    return np.nonzero(~removed)[0], m, o


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
