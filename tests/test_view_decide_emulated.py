"""csrc/view_decide.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads and the wave intrinsics, LDS filled with a pattern
before every launch) with -ffp-contract=off, and must equal the executable contract (tests/view_decide_contract.py) exactly: boxes,
counts, status and the bits of the trace -- every case up to 330 pixels on a side (and the two thin maps around the 8192-element boundary),
single and batched at odd offsets, more items than one launch holds, outputs between 0xFF guard bands with the -1 tails intact, a
NULL trace, the refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import view_decide_cases as cases  # noqa: E402
import view_decide_contract as C  # noqa: E402
from hip_emu_build import guarded, guards_intact  # noqa: E402     (8 elements of 0xFF bytes on both sides)

P = ctypes.c_void_p
SMALL = cases.names(large=False)


class Emulated:
    def __init__(self, lib):
        self.lib = lib
        self.handle = P()
        assert lib.vsc_view_decide_create(None, ctypes.byref(self.handle)) == 0

    def close(self):
        self.lib.vsc_view_decide_destroy(self.handle)

    def run(self, var, count, items, max_views=C.MAX_VIEWS, trace=True):
        """-> (rc, boxes [n, max_views, 4], counts, status, trace [n, 8]); the trace is NULL with trace=False"""
        var = np.ascontiguousarray(var, np.float64).reshape(-1)
        count = np.ascontiguousarray(count, np.uint16).reshape(-1)
        items = np.ascontiguousarray(items, np.int64).reshape(-1, 6)
        n = len(items)
        bufs = [guarded(n * max_views * 4, np.int32), guarded(n, np.int32), guarded(n, np.int32), guarded(n * 8, np.float64)]
        ptrs = [v.ctypes.data for _, v in bufs]
        if not trace:
            ptrs[3] = None
        rc = self.lib.vsc_view_decide_f64(self.handle, var.ctypes.data, var.size, count.ctypes.data, count.size, items.ctypes.data, n,
                                          max_views, *ptrs)
        assert all(guards_intact(b) for b, _ in bufs)
        return rc, bufs[0][1].reshape(n, max_views, 4), bufs[1][1], bufs[2][1], bufs[3][1].reshape(n, 8)


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    emu = Emulated(hip_emu_build.build_shared(tmp_path_factory, "view_decide", hip_emu_build.source("view_decide")))
    yield emu
    emu.close()


def assert_item(name, boxes, count, status, trace):
    """one item's outputs against the contract; trace None: not compared"""
    want_boxes, want_status, want_trace = cases.expected(name)
    assert status == want_status, (name, status)
    assert count == len(want_boxes), (name, count, want_boxes)
    assert boxes[:count].tolist() == [list(b) for b in want_boxes], (name, boxes[:count].tolist(), want_boxes)
    assert (boxes[count:] == -1).all(), (name, "the tail is not -1")
    if trace is not None:
        assert np.array_equal(C.bits(trace), C.bits(want_trace)), (name, "trace bits", trace, want_trace)


def one_item(case):
    h, w = case["var"].shape
    return [(0, 0, h, w, case["m"], case["n"])]


@pytest.mark.parametrize("name", SMALL)
def test_emulated_kernel_equals_contract(emulated, name):
    case = cases.get(name)
    rc, boxes, counts, status, trace = emulated.run(case["var"], case["count"], one_item(case), case["max_views"])
    assert rc == 0
    assert_item(name, boxes[0], int(counts[0]), int(status[0]), trace[0])


def test_emulated_null_trace_writes_nowhere_else(emulated):
    for name in ("recipe_stack2_vertical", "grid_2x2", "over_max_views_2"):
        case = cases.get(name)
        rc, boxes, counts, status, trace = emulated.run(case["var"], case["count"], one_item(case), case["max_views"], trace=False)
        assert rc == 0
        assert_item(name, boxes[0], int(counts[0]), int(status[0]), None)
        assert (trace.view(np.uint8) == 0xFF).all(), "a NULL output was written somewhere else"


BATCH = ["recipe_stack3_horizontal", "width_1", "frames_4", "grid_2x2", "pixels_8193", "recipe_edge_lines_3_vertical", "height_7",
         "random_0", "frames_5", "recipe_height_scan_leaves_start", "samples_1", "width_129"]


def test_emulated_batch_of_mixed_sizes_at_odd_offsets(emulated):
    var, count, items = cases.batch(BATCH)
    assert any(int(v) % 2 for v in items[:, 0]) and any(int(v) % 2 for v in items[:, 1])
    rc, boxes, counts, status, trace = emulated.run(var, count, items)
    assert rc == 0
    for k, name in enumerate(BATCH):
        assert_item(name, boxes[k], int(counts[k]), int(status[k]), trace[k])


def test_emulated_smaller_max_views(emulated):
    """max_views = 3 holds the three views of stack3 exactly; 2 does not (the engineered case)"""
    case = cases.get("stack3")
    rc, boxes, counts, status, _ = emulated.run(case["var"], case["count"], one_item(case), 3)
    assert rc == 0 and status[0] == 0 and boxes[0].tolist() == [list(b) for b in cases.expected("stack3")[0]]
    rc, boxes, counts, status, _ = emulated.run(case["var"], case["count"], one_item(case), 2)
    assert rc == 0 and status[0] == 1 and counts[0] == 0 and (boxes == -1).all()


def test_emulated_more_items_than_one_launch(emulated):
    sel = (["width_7", "frames_4", "height_9", "width_8"] * 17)[:67]
    var, count, items = cases.batch(sel)
    rc, boxes, counts, status, trace = emulated.run(var, count, items, 5)
    assert rc == 0
    for k, name in enumerate(sel):
        assert_item(name, boxes[k], int(counts[k]), int(status[k]), trace[k])


def test_emulated_refusals_write_nothing(emulated):
    lib, h = emulated.lib, emulated.handle
    case = cases.get("width_9")
    var, count = np.ascontiguousarray(case["var"].reshape(-1)), np.ascontiguousarray(case["count"].reshape(-1))
    hh, ww = case["var"].shape
    good = [0, 0, hh, ww, 20, 8]
    a = lambda x: x.ctypes.data     # noqa: E731
    bufs = [guarded(2 * 64 * 4, np.int32), guarded(2, np.int32), guarded(2, np.int32), guarded(16, np.float64)]
    out = [a(v) for _, v in bufs]

    def call(handle, v, vlen, c, clen, items, n, max_views, *o):
        table = np.asarray(items, np.int64) if items is not None else None
        return lib.vsc_view_decide_f64(handle, v, vlen, c, clen, a(table) if table is not None else None, n, max_views, *o)

    ok = (h, a(var), var.size, a(count), count.size)
    assert call(None, *ok[1:], good, 1, 64, *out) != 0                                        # no handle
    for bad in ([0, 0, 0, ww, 20, 8], [0, 0, hh, 0, 20, 8], [0, 0, 4097, 1, 20, 8], [0, 0, 1, 4097, 20, 8], [0, 0, -1, ww, 20, 8]):
        assert call(*ok, bad, 1, 64, *out) != 0                                               # sides outside 1..4096
    for m in (0, 256, -1):
        assert call(*ok, [0, 0, hh, ww, m, 8], 1, 64, *out) != 0                              # samples outside 1..255
    assert call(*ok, [0, 0, hh, ww, 20, -1], 1, 64, *out) != 0                                # negative frames
    for max_views in (0, 65, -1):
        assert call(*ok, good, 1, max_views, *out) != 0
    assert call(*ok, [1, 0, hh, ww, 20, 8], 1, 64, *out) != 0                                 # the variances run past var_len
    assert call(*ok, [0, 1, hh, ww, 20, 8], 1, 64, *out) != 0                                 # the counts run past count_len
    assert call(*ok, [var.size + 1, 0, 1, 1, 20, 8], 1, 64, *out) != 0 and call(*ok, [-1, 0, 1, 1, 20, 8], 1, 64, *out) != 0
    assert call(*ok, [0, -1, 1, 1, 20, 8], 1, 64, *out) != 0
    assert call(h, a(var), var.size - 1, a(count), count.size, good, 1, 64, *out) != 0
    assert call(h, a(var), var.size, a(count), count.size - 1, good, 1, 64, *out) != 0
    assert call(h, a(var), -1, a(count), count.size, good, 1, 64, *out) != 0 and call(*ok, good, -1, 64, *out) != 0
    assert call(*ok, None, 1, 64, *out) != 0                                                  # no item table
    assert call(h, None, var.size, a(count), count.size, good, 1, 64, *out) != 0              # no variances
    assert call(h, a(var), var.size, None, count.size, good, 1, 64, *out) != 0                # no counts
    for k in range(3):
        o = list(out)
        o[k] = None
        assert call(*ok, good, 1, 64, *o) != 0                                                # no boxes / counts / status
    assert call(*ok, good + [0, 0, 4097, ww, 20, 8], 2, 64, *out) != 0                        # a bad item after a good one: nothing launched
    assert all((b.view(np.uint8) == 0xFF).all() for b, _ in bufs), "a refused call wrote"
    assert call(h, None, 0, None, 0, None, 0, 64, None, None, None, None) == 0                # no items: nothing launched
    assert lib.vsc_view_decide_create(None, None) != 0
    rc, boxes, counts, status, trace = emulated.run(case["var"], case["count"], one_item(case))   # and the entry still works
    assert rc == 0
    assert_item("width_9", boxes[0], int(counts[0]), int(status[0]), trace[0])
