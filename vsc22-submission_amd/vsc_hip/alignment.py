"""Temporal alignment on the HIP path: VCSL's `TnVtaModel`, `DpVtaModel` and `HvVtaModel` (infer/vcsl/vta.py:244-363 / :153-241 /
:366-426, the model classes :476-539) without the VCSL package; `build_alignment` stands where `build_vta_model` stands (:542-552).
`DpAlignment` and `HvAlignment` have TnAlignment's three entry points and run `vsc_align_dp_f32` / `vsc_align_hv_f32`.

`TnAlignment.forward_sim([(key, matrix), ...])` is VCSL's model interface, so an instance plugs into the `model=` seam of
`vsc.baseline.localization.VCSLLocalization`; `TnAlignment.align(flat, pairs, bias)` takes the device tensor of one
`ops.pair_similarity` launch as it is, so the matrices never leave the device.  Both run `vsc_tn_align_f32` (one wave per
pair, all pairs in one launch); its header comment states the contract, including the one deliberate difference from the
reference: ties in a row's top-K go to the lower column (numpy's default argsort leaves their order unspecified).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

# limits of the kernel (include/vsc_hip.h, vsc_tn_align_f32)
MAX_TOP_K = 16
MASK_BITS = 64          # (max_step - 1) * top_k
MAX_PATH = 4095
MAX_Q_ROWS = 1 << 16
MAX_R_ROWS = 1 << 24


def check_params(tn_max_step: int, tn_top_k: int, max_path: int, min_length: int) -> None:
    """Raise ValueError for TN parameters outside what the kernel holds."""
    if tn_max_step < 1:
        raise ValueError(f"tn_max_step {tn_max_step} < 1")
    if not 1 <= tn_top_k <= MAX_TOP_K:
        raise ValueError(f"tn_top_k {tn_top_k} outside [1, {MAX_TOP_K}]")
    if (tn_max_step - 1) * tn_top_k > MASK_BITS:
        raise ValueError(f"(tn_max_step - 1) * tn_top_k = {(tn_max_step - 1) * tn_top_k} exceeds the {MASK_BITS} "
                         f"predecessor bits of a graph node")
    if not 0 <= max_path <= MAX_PATH:
        raise ValueError(f"max_path {max_path} outside [0, {MAX_PATH}]")
    if min_length < 0:
        raise ValueError(f"min_length {min_length} < 0")


def check_shape(q_rows: int, r_rows: int) -> None:
    if not (0 <= q_rows <= MAX_Q_ROWS and 0 <= r_rows <= MAX_R_ROWS):
        raise ValueError(f"{q_rows} x {r_rows} similarity matrix outside the kernel's {MAX_Q_ROWS} x {MAX_R_ROWS}")


class TnAlignment:
    """VCSL's TN model (TnVtaModel's parameters and defaults) on the HIP path."""

    def __init__(self, tn_max_step: int = 10, tn_top_k: int = 5, max_path: int = 10, min_sim: float = 0.2,
                 min_length: int = 5, max_iou: float = 0.3):
        check_params(tn_max_step, tn_top_k, max_path, min_length)
        self.tn_max_step, self.tn_top_k, self.max_path = int(tn_max_step), int(tn_top_k), int(max_path)
        self.min_sim, self.min_length, self.max_iou = float(min_sim), int(min_length), float(max_iou)

    def align(self, flat, pairs, bias: float = 0.0):
        """Device path: flat fp32 device tensor, pairs int64 [n, 3] (element offset, q_rows, r_rows) on the host, every
        element used as s + bias.  -> (boxes int32 [n, max_path + 1, 4], counts int32 [n], maxsim float32
        [n, max_path + 1]) on the device (ops.tn_align)."""
        from vsc_hip import ops
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
        for _, q, r in pairs:
            check_shape(int(q), int(r))
        return ops.tn_align(flat, pairs, bias, self.tn_max_step, self.tn_top_k, self.max_path, self.min_sim,
                            self.min_length, self.max_iou)

    def align_pair_similarity(self, flat, offsets, pairs4, bias: float = 0.0):
        """`ops.pair_similarity`'s (flat, offsets) and its int64 [n, 4] pair table (q_row0, q_rows, r_row0, r_rows)."""
        pairs4 = np.asarray(pairs4, dtype=np.int64).reshape(-1, 4)
        table = np.stack([np.asarray(offsets, dtype=np.int64)[:len(pairs4)], pairs4[:, 1], pairs4[:, 3]], axis=1)
        return self.align(flat, table, bias)

    def forward_sim(self, data: Sequence[Tuple[str, np.ndarray]]) -> List[Tuple[str, List[List[int]]]]:
        """VCSL's interface: [(key, [q, r] similarity matrix), ...] -> [(key, [[x1, y1, x2, y2], ...]), ...]."""
        import torch

        from vsc_hip import _lib
        data = list(data)
        if not data:
            return []
        _lib.require_device()
        mats = [np.ascontiguousarray(m, dtype=np.float32) for _, m in data]
        for m in mats:
            if m.ndim != 2:
                raise ValueError(f"similarity matrix of shape {m.shape}: two dimensions expected")
        sizes = np.array([m.size for m in mats], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        table = np.stack([offsets, [m.shape[0] for m in mats], [m.shape[1] for m in mats]], axis=1).astype(np.int64)
        dev = torch.device("cuda", torch.cuda.current_device())
        flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).to(dev)
        boxes, counts, _ = self.align(flat, table, 0.0)
        boxes, counts = boxes.cpu().numpy(), counts.cpu().numpy()
        return [(key, boxes[i, :counts[i]].tolist()) for i, (key, _) in enumerate(data)]


# limits of vsc_align_dp_f32 / vsc_align_hv_f32 (include/vsc_hip.h)
MAX_ALIGN_DIM = 1 << 16
MAX_ALIGN_CELLS = 1 << 26
MAX_DISCONTINUE = 254
MAX_BOXES = 4096


def check_align_shape(q_rows: int, r_rows: int) -> None:
    if not (0 <= q_rows <= MAX_ALIGN_DIM and 0 <= r_rows <= MAX_ALIGN_DIM):
        raise ValueError(f"{q_rows} x {r_rows} similarity matrix outside the kernel's {MAX_ALIGN_DIM} rows and columns")
    if q_rows * r_rows > MAX_ALIGN_CELLS:
        raise ValueError(f"{q_rows} x {r_rows} similarity matrix outside the kernel's {MAX_ALIGN_CELLS} cells")


class _BoxAlignment:
    """What DpAlignment and HvAlignment share: TnAlignment's `align_pair_similarity` and `forward_sim` over their own `align`."""

    max_boxes: int

    def _table(self, pairs):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
        for _, q, r in pairs:
            check_align_shape(int(q), int(r))
        return pairs

    align_pair_similarity = TnAlignment.align_pair_similarity

    def forward_sim(self, data: Sequence[Tuple[str, np.ndarray]]) -> List[Tuple[str, List[List[int]]]]:
        """VCSL's interface: [(key, [q, r] similarity matrix), ...] -> [(key, [[x1, y1, x2, y2], ...]), ...].  Raises if a pair
        has more boxes than the `max_boxes` slots hold (the reference returns them all)."""
        import torch

        from vsc_hip import _lib
        data = list(data)
        if not data:
            return []
        _lib.require_device()
        mats = [np.ascontiguousarray(m, dtype=np.float32) for _, m in data]
        for m in mats:
            if m.ndim != 2:
                raise ValueError(f"similarity matrix of shape {m.shape}: two dimensions expected")
        sizes = np.array([m.size for m in mats], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        table = np.stack([offsets, [m.shape[0] for m in mats], [m.shape[1] for m in mats]], axis=1).astype(np.int64)
        dev = torch.device("cuda", torch.cuda.current_device())
        flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])).to(dev)
        boxes, counts, _ = self.align(flat, table, 0.0)
        boxes, counts = boxes.cpu().numpy(), counts.cpu().numpy()
        check_counts(counts, self.max_boxes, [key for key, _ in data])
        return [(key, boxes[i, :counts[i]].tolist()) for i, (key, _) in enumerate(data)]


def check_counts(counts, max_boxes: int, keys) -> None:
    """Raise if a pair found more boxes than were stored."""
    over = [i for i in range(len(counts)) if counts[i] > max_boxes]
    if over:
        i = over[0]
        raise RuntimeError(f"pair {keys[i]!r} has {int(counts[i])} boxes, {max_boxes} slots (max_boxes); {len(over)} such pairs")


class DpAlignment(_BoxAlignment):
    """VCSL's DP model (DpVtaModel's parameters and defaults) on the HIP path.  `max_iou` and `sum_sim` are accepted and unused,
    as in the reference; `max_boxes` is this class's own: the box slots per pair (the reference's list is unbounded)."""

    def __init__(self, discontinue: int = 3, min_sim: float = 0.0, min_length: int = 5, max_iou: float = 0.3, sum_sim: float = 8,
                 ave_sim: float = 0.3, diagonal_thres: int = 10, max_boxes: int = 100, handle=None):
        if not 0 <= discontinue <= MAX_DISCONTINUE:
            raise ValueError(f"discontinue {discontinue} outside [0, {MAX_DISCONTINUE}]")
        if min_length < 0:
            raise ValueError(f"min_length {min_length} < 0")
        if diagonal_thres < 0:
            raise ValueError(f"diagonal_thres {diagonal_thres} < 0")
        if not 1 <= max_boxes <= MAX_BOXES:
            raise ValueError(f"max_boxes {max_boxes} outside [1, {MAX_BOXES}]")
        self.discontinue, self.min_sim, self.min_length = int(discontinue), float(min_sim), int(min_length)
        self.max_iou, self.sum_sim = max_iou, sum_sim
        self.ave_sim, self.diagonal_thres, self.max_boxes = float(ave_sim), int(diagonal_thres), int(max_boxes)
        self.handle = handle

    def align(self, flat, pairs, bias: float = 0.0):
        """Device path, as TnAlignment.align -> (boxes int32 [n, max_boxes, 4], counts int32 [n] = boxes FOUND, maxsim float32
        [n, max_boxes]) on the device (ops.dp_align)."""
        from vsc_hip import ops
        return ops.dp_align(flat, self._table(pairs), bias, self.discontinue, self.min_sim, self.ave_sim, self.min_length,
                            self.diagonal_thres, self.max_boxes, handle=self.handle)


class HvAlignment(_BoxAlignment):
    """VCSL's HV model (HvVtaModel's parameters and defaults) on the HIP path.  `min_bins` and `min_peaks` are accepted and
    unused, as in the reference."""

    def __init__(self, iou_thresh: float = 0.9, min_sim: float = 0.0, min_bins: int = 1, max_peaks: int = 100, min_peaks: int = 10,
                 handle=None):
        if not 1 <= max_peaks <= MAX_BOXES:
            raise ValueError(f"max_peaks {max_peaks} outside [1, {MAX_BOXES}]")
        self.iou_thresh, self.min_sim, self.max_peaks = float(iou_thresh), float(min_sim), int(max_peaks)
        self.min_bins, self.min_peaks = min_bins, min_peaks
        self.max_boxes = self.max_peaks
        self.handle = handle

    def align(self, flat, pairs, bias: float = 0.0):
        """Device path, as TnAlignment.align -> (boxes int32 [n, max_peaks, 4], counts int32 [n], maxsim float32 [n, max_peaks])
        on the device (ops.hv_align)."""
        from vsc_hip import ops
        return ops.hv_align(flat, self._table(pairs), bias, self.min_sim, self.iou_thresh, self.max_peaks, handle=self.handle)


def build_alignment(method: str = "DTW", **config):
    """`build_vta_model` (infer/vcsl/vta.py:542-552) for the models that exist on the device.  `concurrency` and `version` are
    the reference's process-pool arguments and are dropped."""
    config.pop("concurrency", None)
    config.pop("version", None)
    if method == "TN":
        return TnAlignment(**config)
    if method == "DP":
        return DpAlignment(**config)
    if method == "HV":
        return HvAlignment(**config)
    if method == "DTW":
        raise NotImplementedError("DTW rests on tslearn.metrics.dtw_path_from_metric; tslearn is not part of this project, so "
                                  "the model has no device counterpart: use TN, DP or HV")
    raise ValueError(f"Unknown method {method}")
