"""csrc/segment_metric.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads and the wave intrinsics, the handle's allocations
filled with 0xFF when fresh) and must equal the executable contract (tests/segment_metric_contract.py) bit for bit: the sorted
inserts over chunks of 64, the fusing of components, the considered flags, the summation order, the scan's tiles and its walk over
`ends`, the refusals.  The GPU suite (tests/test_gpu_segment_metric.py) checks the same on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import segment_metric_cases as cases  # noqa: E402
import segment_metric_contract as C  # noqa: E402

P = ctypes.c_void_p


class Emulated:
    def __init__(self, lib):
        self.lib = lib
        self.handle = P()
        assert lib.vsc_segment_metric_create(None, ctypes.byref(self.handle)) == 0

    def close(self):
        self.lib.vsc_segment_metric_destroy(self.handle)

    def deltas(self, k):
        n_preds, n_gts = len(k["pred_boxes"]), len(k["gt_boxes"])
        out, gt_len = np.full((n_preds, 4), np.nan), np.full((k["n_pairs"], 2), np.nan)
        rc = self.lib.vsc_segment_metric_deltas_f64(self.handle, k["pred_boxes"].ctypes.data, k["pred_ptr"].ctypes.data, k["pred_rank"].ctypes.data,
                                                    n_preds, k["gt_boxes"].ctypes.data, k["gt_ptr"].ctypes.data, n_gts, k["n_pairs"],
                                                    out.ctypes.data, gt_len.ctypes.data)
        return rc, out, gt_len

    def scan(self, rows, ends, cols=None):
        rows, ends = np.ascontiguousarray(rows, np.float64), np.ascontiguousarray(ends, np.int64)
        cols = rows.shape[1] if cols is None else cols
        out = np.full((len(ends), max(cols, 1)), np.nan)
        rc = self.lib.vsc_segment_metric_scan_f64(self.handle, rows.ctypes.data, len(rows), cols, ends.ctypes.data, len(ends), out.ctypes.data)
        return rc, out


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    emu = Emulated(hip_emu_build.build_shared(tmp_path_factory, "segment_metric", hip_emu_build.source("segment_metric")))
    yield emu
    emu.close()


@pytest.mark.parametrize("name", [c[0] for c in cases.cases() if c[2]])
def test_emulated_kernels_equal_contract(emulated, name):
    """every case with predictions, the lists of 130 predictions and 65 ground truths included; one handle for all of them, so its
    scratch is reused at every size"""
    gts, preds = next(c[1:] for c in cases.cases() if c[0] == name)
    k = C.pack(gts, preds)
    rc, d, gt_len = emulated.deltas(k)
    assert rc == 0
    want_d, want_len = C.deltas(k["pred_boxes"], k["pred_ptr"], k["pred_rank"], k["gt_boxes"], k["gt_ptr"], k["n_pairs"])
    assert np.array_equal(C.bits(gt_len), C.bits(want_len))
    assert np.array_equal(C.bits(d), C.bits(want_d)), np.nonzero((C.bits(d) != C.bits(want_d)).any(1))[0][:10]
    rc, groups = emulated.scan(d, k["group_ends"])
    assert rc == 0 and np.array_equal(C.bits(groups), C.bits(C.scan(want_d, k["group_ends"])))
    if k["n_gt_pairs"]:
        rc, totals = emulated.scan(gt_len[:k["n_gt_pairs"]], [k["n_gt_pairs"] - 1])
        assert rc == 0 and np.array_equal(C.bits(totals), C.bits(C.scan(want_len[:k["n_gt_pairs"]], [k["n_gt_pairs"] - 1])))


@pytest.mark.parametrize("n,cols", [(1, 1), (511, 3), (512, 8), (513, 4), (1500, 4)])
def test_emulated_scan_tiles_and_ends(emulated, n, cols):
    """rows around the tile of 512 and over several tiles; ends: every row (more than 256 in a tile), a sparse set, repeated ends,
    the last row alone"""
    rs = np.random.RandomState(n)
    rows = rs.uniform(-1, 1, (n, cols)) * 10.0 ** rs.randint(-8, 8, (n, cols))
    for ends in (np.arange(n), np.unique(rs.randint(0, n, max(n // 7, 1))), np.sort(np.r_[rs.randint(0, n, 5), rs.randint(0, n, 5)].repeat(2)), [n - 1]):
        rc, out = emulated.scan(rows, ends)
        assert rc == 0 and np.array_equal(C.bits(out), C.bits(C.scan(rows, ends))), (n, cols, len(ends))


def test_emulated_refusals_and_empty_calls(emulated):
    k = C.pack(*cases.cases()[4][1:])
    rows, ends = np.ones((4, 2)), [3]
    assert emulated.scan(rows, ends, cols=0)[0] != 0 and emulated.scan(np.ones((4, 9)), ends)[0] != 0
    lib, h = emulated.lib, emulated.handle
    assert lib.vsc_segment_metric_scan_f64(h, rows.ctypes.data, -1, 2, None, 1, None) != 0
    assert lib.vsc_segment_metric_scan_f64(h, None, 0, 2, None, 0, None) == 0                 # n = 0: nothing launched
    assert lib.vsc_segment_metric_deltas_f64(h, None, None, None, -1, None, None, 0, 1, None, None) != 0
    assert lib.vsc_segment_metric_deltas_f64(h, None, None, None, 0, None, None, -1, 1, None, None) != 0
    assert lib.vsc_segment_metric_deltas_f64(h, None, None, None, 0, None, None, 0, -1, None, None) != 0
    assert lib.vsc_segment_metric_deltas_f64(h, None, None, None, 0, None, None, 5, 3, None, None) == 0    # n_preds = 0: nothing launched
    assert lib.vsc_segment_metric_deltas_f64(None, None, None, None, 0, None, None, 5, 3, None, None) != 0
    rc, d, gt_len = emulated.deltas(k)                                                          # and the handle still works
    assert rc == 0 and np.array_equal(C.bits(d), C.bits(C.deltas(k["pred_boxes"], k["pred_ptr"], k["pred_rank"], k["gt_boxes"], k["gt_ptr"], k["n_pairs"])[0]))
