"""Matching-track segment AP on the HIP path (reference: VSC22-Matching-Track-1st/infer/vsc/metrics.py:120-383, ``match_metric``).

The reference walks the predictions in score order and, for each, rebuilds and re-sorts every interval list of its video pair.
Here the host only packs: pair ids are factorised (pairs that have ground truth first, in order of first appearance -- the
insertion order of the reference's dict), the predictions get their rank in the stable descending sort by score, and two CSR
tables list each pair's ranks and ground truths.  ``vsc_segment_metric_deltas_f64`` (one wave per pair) writes every prediction's
{dI_q, dI_r, dT_q, dT_r} at its rank, ``vsc_segment_metric_scan_f64`` sums them strictly in rank order and returns the running
values at the end of every tie group, and a second scan gives the two ground-truth totals (include/vsc_hip.h states the
contract, tests/segment_metric_contract.py is its executable form).  Only ``[n_groups][4]`` and ``[2]`` come back; the divisions,
square roots and the AP sum are done here in Python floats, exactly as the reference does them, so ``.ap`` and the curve are the
reference's bit for bit.

Refused with ``ValueError`` before any device work: non-finite scores or timestamps, and any box with ``end < start`` -- the
reference sorts intervals as (start, end) tuples and sums ``end - start`` over whatever its merge leaves, so its answer for an
inverted box depends on which neighbours the sort happens to put next to it; there is nothing to reproduce.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np


class Packed(NamedTuple):
    pred_boxes: np.ndarray      # [P][4] float64, rank order
    pred_ptr: np.ndarray        # [n_pairs + 1] int64
    pred_rank: np.ndarray       # [P] int64: each pair's ranks, ascending
    gt_boxes: np.ndarray        # [G][4] float64, grouped by pair in file order
    gt_ptr: np.ndarray          # [n_pairs + 1] int64
    n_pairs: int
    n_gt_pairs: int             # pairs 0 .. n_gt_pairs - 1 have ground truth
    group_ends: np.ndarray      # [n_groups] int64: rank of the last prediction of every run of == scores
    group_scores: np.ndarray    # [n_groups] float64: the score of the run's first prediction (what itertools.groupby reports)


def _boxes(matches, what: str) -> np.ndarray:
    b = np.array([(m.query_start, m.query_end, m.ref_start, m.ref_end) for m in matches], dtype=np.float64).reshape(-1, 4)
    if not np.isfinite(b).all():
        raise ValueError(f"{what}: non-finite timestamps")
    if (b[:, 1] < b[:, 0]).any() or (b[:, 3] < b[:, 2]).any():
        bad = int(np.nonzero((b[:, 1] < b[:, 0]) | (b[:, 3] < b[:, 2]))[0][0])
        raise ValueError(f"{what}: row {bad} has end < start ({b[bad].tolist()})")
    return b


def _csr(pair: np.ndarray, n_pairs: int):
    """stable grouping of positions by pair id: (positions grouped, ptr)"""
    ptr = np.zeros(n_pairs + 1, np.int64)
    np.cumsum(np.bincount(pair, minlength=n_pairs), out=ptr[1:])
    return np.argsort(pair, kind="stable").astype(np.int64), ptr


def pack(gts, predictions) -> Packed:
    """Lists of ``vsc.metrics.Match`` -> the operands of the two device entries (numpy, host)."""
    gt_boxes, pred_boxes = _boxes(gts, "ground truth"), _boxes(predictions, "predictions")
    scores = np.array([m.score for m in predictions], dtype=np.float64)
    if not np.isfinite(scores).all():
        raise ValueError("predictions: non-finite scores")
    pair_of: dict = {}
    gt_pair = np.array([pair_of.setdefault((m.query_id, m.ref_id), len(pair_of)) for m in gts], dtype=np.int64)
    n_gt_pairs = len(pair_of)
    pred_pair = np.array([pair_of.setdefault((m.query_id, m.ref_id), len(pair_of)) for m in predictions], dtype=np.int64)
    n_pairs = len(pair_of)
    order = np.argsort(-scores, kind="stable")             # sorted(predictions, key=score, reverse=True): ties keep file order
    s = scores[order]
    pred_rank, pred_ptr = _csr(pred_pair[order], n_pairs)
    gt_order, gt_ptr = _csr(gt_pair, n_pairs)
    ends = np.nonzero(np.r_[s[1:] != s[:-1], True])[0].astype(np.int64) if len(s) else np.zeros(0, np.int64)
    starts = np.r_[0, ends[:-1] + 1].astype(np.int64) if len(s) else ends
    return Packed(np.ascontiguousarray(pred_boxes[order]), pred_ptr, pred_rank, np.ascontiguousarray(gt_boxes[gt_order]), gt_ptr, n_pairs,
                  n_gt_pairs, ends, s[starts])


def finish(groups, totals, group_scores):
    """metrics.py:338-383 on the running sums: groups [n_groups][4] = {I_q, I_r, T_q, T_r} at the end of every tie group, totals
    [2] = the ground-truth lengths.  -> (ap, precisions, recalls, scores) in Python floats; ZeroDivisionError where the
    reference raises it (no ground-truth length, or no covered length at a group)."""
    gq, gr = float(totals[0]), float(totals[1])
    recall = metric = 0.0
    precisions, recalls, scores = [], [], []
    for (iq, ir, tq, tr), score in zip(np.asarray(groups, dtype=np.float64).reshape(-1, 4).tolist(), np.asarray(group_scores).tolist()):
        new_recall = math.sqrt((iq / gq) * (ir / gr))
        precision = math.sqrt((iq / tq) * (ir / tr))
        delta_recall = new_recall - recall
        metric += precision * delta_recall
        recall = new_recall
        if delta_recall > 0:
            recalls.append(recall)
            precisions.append(precision)
            scores.append(score)
    return metric, precisions, recalls, scores


class HipSegmentMetric:
    """The device handle (vsc_segment_metric_*): owns the scratch, bound to the stream that is current when it is made."""

    def __init__(self):
        from vsc_hip import _lib
        self._lib = _lib.require_device()
        handle = ctypes.c_void_p()
        _lib.check(self._lib.vsc_segment_metric_create(_lib.current_stream(), ctypes.byref(handle)))
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vsc_segment_metric_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def deltas(self, pred_boxes, pred_ptr, pred_rank, gt_boxes, gt_ptr, deltas=None, gt_len=None):
        """device tensors in, (deltas [P][4], gt_len [n_pairs][2]) float64 device tensors out (enqueued on the handle's stream)"""
        import torch

        from vsc_hip import _lib
        n_preds, n_gts, n_pairs = pred_boxes.shape[0], gt_boxes.shape[0], pred_ptr.shape[0] - 1
        assert pred_boxes.dtype == gt_boxes.dtype == torch.float64 and pred_ptr.dtype == pred_rank.dtype == gt_ptr.dtype == torch.int64
        assert gt_ptr.shape[0] == n_pairs + 1 and pred_rank.shape[0] == n_preds
        if deltas is None:
            deltas = torch.empty((n_preds, 4), dtype=torch.float64, device=pred_boxes.device)
        if gt_len is None:
            gt_len = torch.empty((n_pairs, 2), dtype=torch.float64, device=pred_boxes.device)
        _lib.check(self._lib.vsc_segment_metric_deltas_f64(self._h, _lib.ptr(pred_boxes), _lib.ptr(pred_ptr), _lib.ptr(pred_rank), n_preds,
                                                           _lib.ptr(gt_boxes), _lib.ptr(gt_ptr), n_gts, n_pairs, _lib.ptr(deltas), _lib.ptr(gt_len)))
        return deltas, gt_len

    def scan(self, rows, ends, out=None):
        """rows [n][cols] float64, ends [n_ends] int64 ascending (device) -> out [n_ends][cols]: np.cumsum(rows, 0)[ends], left to right"""
        import torch

        from vsc_hip import _lib
        assert rows.dtype == torch.float64 and ends.dtype == torch.int64 and rows.dim() == 2
        if out is None:
            out = torch.empty((ends.shape[0], rows.shape[1]), dtype=torch.float64, device=rows.device)
        _lib.check(self._lib.vsc_segment_metric_scan_f64(self._h, _lib.ptr(rows), rows.shape[0], rows.shape[1], _lib.ptr(ends), ends.shape[0],
                                                         _lib.ptr(out)))
        return out


def segment_ap(gts, predictions):
    """``match_metric`` of the reference on lists of ``vsc.metrics.Match``: -> (ap, precisions, recalls, scores).  Needs a device."""
    import torch

    from vsc_hip import _lib
    _lib.require_device()
    k = pack(gts, predictions)
    if not len(predictions):
        return 0.0, [], [], []
    up = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    with HipSegmentMetric() as h:
        d, gt_len = h.deltas(up(k.pred_boxes), up(k.pred_ptr), up(k.pred_rank), up(k.gt_boxes), up(k.gt_ptr))
        groups = h.scan(d, up(k.group_ends))
        totals = None
        if k.n_gt_pairs:
            totals = h.scan(gt_len[:k.n_gt_pairs], up(np.array([k.n_gt_pairs - 1], np.int64)))
        groups = groups.cpu().numpy()
        totals = totals.cpu().numpy()[0] if totals is not None else (0.0, 0.0)
    return finish(groups, totals, k.group_scores)
