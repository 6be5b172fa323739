"""Temporal-network (TN) alignment on the HIP path: VCSL's `TnVtaModel` (infer/vcsl/vta.py:244-363, 499-518) without the
VCSL package.

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
