"""Descriptor-track micro-AP on the HIP path (reference: VSC22-Descriptor-Track-1st/infer/vsc/metrics.py:423-494,
``average_precision`` -- the number the reference logs as "Candidate uAP").

The host interns the video ids -- the only dictionary left here -- and packs every pair into a 64-bit key; one buffer goes up.
``vsc_uap_rank_f64`` orders the predictions (stable, descending), counts what the reference refuses and joins the ranked
predictions against the ground truth; ``vsc_uap_curve_f64`` scans, writes the curve at the correct predictions and returns the two
sums in numpy's summation order (include/vsc_hip.h states the contract, tests/uap_contract.py is its executable form).  What comes
back is sums, counts and status (64 bytes) and the written columns of the curve.  ``max(0.0, .)``, the rescale by predicted / actual positives and the division by
the number of ground-truth pairs are done here in Python floats, as the reference does them, so ``.ap``, ``.simple_ap`` and the
curve are the reference's bit for bit (tests/golden/uap_device.json).

Raises what the reference raises: AssertionError("Duplicates detected in ground truth" / "... in predictions"),
ValueError("Scores must be finite."), and KeyError for an empty ground truth or no predictions (the reference's data frames have
no columns then; recorded in tests/golden/uap_device.json).
"""
from __future__ import annotations

import numpy as np


def intern_pairs(ground_truth, predictions):
    """-> (pred_keys uint64 [n], gt_keys uint64 [g], key_bits): the pair (q, r) as q_index << ref_bits | r_index over the ids of
    both lists; ref_bits is 32 unless both index ranges are small, in which case the key sorts run fewer digit passes"""
    q_of: dict = {}
    r_of: dict = {}
    pq = np.fromiter((q_of.setdefault(p.query_id, len(q_of)) for p in predictions), np.uint64, len(predictions))
    pr = np.fromiter((r_of.setdefault(p.ref_id, len(r_of)) for p in predictions), np.uint64, len(predictions))
    gq = np.fromiter((q_of.setdefault(p.query_id, len(q_of)) for p in ground_truth), np.uint64, len(ground_truth))
    gr = np.fromiter((r_of.setdefault(p.ref_id, len(r_of)) for p in ground_truth), np.uint64, len(ground_truth))
    if len(q_of) >= 1 << 32 or len(r_of) >= 1 << 32:
        raise ValueError("more than 2^32 distinct video ids")
    ref_bits = max(1, (len(r_of) - 1).bit_length())
    key_bits = ref_bits + max(1, (len(q_of) - 1).bit_length())
    sh = np.uint64(ref_bits)
    return (pq << sh) | pr, (gq << sh) | gr, key_bits


class HipUap:
    """The device handle (vsc_uap_*): bound to the stream that is current when it is made (or to `stream`); owns no device memory."""

    def __init__(self, lib=None, stream=None):
        import ctypes

        from vsc_hip import _lib
        self._lib = lib or _lib.require_device()
        handle = ctypes.c_void_p()
        _lib.check(self._lib.vsc_uap_create(stream if stream is not None else _lib.current_stream(), ctypes.byref(handle)))
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vsc_uap_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def rank(self, scores, pred_keys, n, gt_keys, g, key_bits, perm, ranked, correct, status):
        """device pointers (ints or c_void_p) in and out; enqueues on the handle's stream"""
        from vsc_hip import _lib
        _lib.check(self._lib.vsc_uap_rank_f64(self._h, scores, pred_keys, n, gt_keys, g, key_bits, perm, ranked, correct, status))

    def curve(self, ranked, correct, n, n_gt, sums, counts, curve):
        from vsc_hip import _lib
        _lib.check(self._lib.vsc_uap_curve_f64(self._h, ranked, correct, n, n_gt, sums, counts, curve))


def uap_device(scores, pred_keys, gt_keys, key_bits, lib=None):
    """The two entries on arrays: -> (sums float64 [2], counts int64 [2], status int64 [4], curve float64 [3][n_pos]).  One
    upload, two calls on the current stream, and the download in two pieces: the 64 bytes of sums, counts and status, which say how
    many columns of the curve were written, then those columns.  n >= 1, g >= 1."""
    import torch

    from vsc_hip import _lib
    lib = lib or _lib.require_device()
    n, g = len(scores), len(gt_keys)
    assert n >= 1 and g >= 1 and len(pred_keys) == n
    up = np.empty(2 * n + g, np.uint64)
    up[:n] = np.ascontiguousarray(scores, np.float64).view(np.uint64)
    up[n:2 * n] = pred_keys
    up[2 * n:] = gt_keys
    dev = torch.from_numpy(up.view(np.int64)).cuda()
    # outputs, 8-byte words: sums [2], counts [2], status [4], curve [3][n], perm [n], ranked [n], correct (bytes) [n]
    out = torch.empty(8 + 5 * n + (n + 7) // 8, dtype=torch.int64, device=dev.device)
    base, w = out.data_ptr(), 8
    sums, counts, status, curve = base, base + 2 * w, base + 4 * w, base + 8 * w
    perm, ranked, correct = curve + 3 * n * w, curve + 4 * n * w, curve + 5 * n * w
    with HipUap(lib) as h:
        h.rank(dev.data_ptr(), dev.data_ptr() + n * w, n, dev.data_ptr() + 2 * n * w, g, key_bits, perm, ranked, correct, status)
        h.curve(ranked, correct, n, g, sums, counts, curve)
    head = out[:8].cpu().numpy()                     # (synchronises the stream)
    n_pos = int(head[2])
    rows = out[8:8 + 3 * n].view(3, n)[:, :n_pos].contiguous().cpu().numpy().view(np.float64) if n_pos else np.zeros((3, 0))
    return head[:2].view(np.float64).copy(), head[2:4].copy(), head[4:8].copy(), rows


def check_status(status, n: int, g: int) -> None:
    """Raises what the reference raises, in its order: status = {non-finite scores, duplicate predictions, duplicate ground-truth
    pairs, ...} as vsc_uap_rank_f64 counts them, n predictions, g ground-truth pairs."""
    if status[2]:
        raise AssertionError("Duplicates detected in ground truth")
    if status[1]:
        raise AssertionError("Duplicates detected in predictions")
    if not g:
        raise KeyError("empty ground truth: the reference's ground-truth frame has no query_id / ref_id columns")
    if not n:
        raise KeyError("no predictions: the reference's prediction frame has no score column")
    if status[0]:
        raise ValueError("Scores must be finite.")


def average_precision_hip(ground_truth, predictions):
    """``vsc.metrics.average_precision`` with the sort, the join, the scans and the sums on the device."""
    from vsc.metrics import AveragePrecision, PrecisionRecallCurve
    from vsc_hip import _lib
    lib = _lib.require_device()
    ground_truth, predictions = list(ground_truth), list(predictions)
    pred_keys, gt_keys, key_bits = intern_pairs(ground_truth, predictions)
    scores = np.fromiter((p.score for p in predictions), np.float64, len(predictions))
    n, g = len(predictions), len(ground_truth)
    if n and g:
        sums, counts, status, curve = uap_device(scores, pred_keys, gt_keys, key_bits, lib)
    else:       # nothing to launch: the duplicate checks come first in the reference, so they are made here
        status = [0, n - len(np.unique(pred_keys)), g - len(np.unique(gt_keys)), 0]
    check_status(status, n, g)
    n_pos = int(counts[0])
    ap = max(0.0, float(sums[0])) * (n_pos / g)
    simple = float(sums[1]) / g
    return AveragePrecision(ap=float(ap), simple_ap=float(simple),
                            pr_curve=PrecisionRecallCurve(curve[0].copy(), curve[1].copy(), curve[2].copy()))
