"""csrc/match_maps.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads and the wave intrinsics) and must equal the executable
contract (tests/match_maps_contract.py) bit for bit.  This checks the kernels' logic -- the sorted top-ten in the lanes, the summation
order, the choice among the waves, the tile walk of both slices, the launcher's chunks and refusals; the GPU suite
(tests/test_gpu_match_maps.py) checks the same on the device on every planted item."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import match_maps_cases as cases  # noqa: E402
import match_maps_contract as C  # noqa: E402


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    return hip_emu_build.build_shared(tmp_path_factory, "match_maps", hip_emu_build.source("match_maps")).vsc_match_maps_f32


def _run(fn, flat, table, resolution, with_transpose):
    n, slices = len(table), 2 if with_transpose else 1
    table = np.ascontiguousarray(table, np.int64)
    starts = np.full(max(n, 1), -7, np.int32)
    out = np.full((max(n, 1) * slices, resolution, resolution, 3), np.nan, np.float32)
    rc = fn(flat.ctypes.data, flat.size, table.ctypes.data, n, resolution, int(with_transpose), starts.ctypes.data, out.ctypes.data, None)
    return rc, starts[:n], out[:n * slices]


def _affordable(items, most_rows, edges):
    """Multi-view items of up to `most_rows` rows (every row costs a dozen barrier rounds of 64 OS threads), every other
    single-view item, and the tile-edge items named in `edges` (None: all of them)."""
    keep = []
    for it in items:
        name, m, frames = it
        if name.startswith("edge_"):
            if edges is None or name in edges:
                keep.append(it)
        elif m.shape[0] <= frames or m.shape[0] <= most_rows:
            keep.append(it)
    return keep


@pytest.mark.parametrize("resolution,with_transpose,most_rows", [(8, 1, 60), (70, 1, 36), (70, 0, 36)])
def test_emulated_kernels_equal_contract(emulated, resolution, with_transpose, most_rows):
    """R = 8: one tile per slice, every planted item of up to 60 rows (frames 1 .. 11 with 2, 3 and 5 views, the ties, the
    summation order, r_rows = 1, empty items).  R = 70: four tiles per slice with ragged edges, fewer items."""
    edges = None if resolution == 8 else ("edge_33x65", "edge_65x33", "edge_64x64", "edge_63x31", "edge_multi_65x33")
    items = _affordable(cases.planted(resolution), most_rows, edges)
    assert len(items) >= 20 and any(it[1].shape[0] > it[2] for it in items)
    flat, table = cases.pack(items)
    rc, starts, out = _run(emulated, flat, table, resolution, with_transpose)
    assert rc == 0
    want_starts, want = C.match_maps(flat, table, resolution, with_transpose)
    assert np.array_equal(starts, want_starts), [(it[0], a, b) for it, a, b in zip(items, starts, want_starts) if a != b]
    slices = 1 + with_transpose
    for p, it in enumerate(items):
        assert np.array_equal(C.bits(out[p * slices:(p + 1) * slices]), C.bits(want[p * slices:(p + 1) * slices])), it[0]


def test_emulated_launcher_chunks_and_refusals(emulated):
    """More items than one launch carries (128), and what the entry refuses."""
    rs = np.random.RandomState(3)
    items = [(f"i{k}", rs.uniform(-1, 1, ((1 + (k % 8 == 7)) * (1 + k % 3), 1 + k % 5)).astype(np.float32), 1 + k % 3) for k in range(131)]
    flat, table = cases.pack(items)
    rc, starts, out = _run(emulated, flat, table, 4, 0)
    want_starts, want = C.match_maps(flat, table, 4, 0)
    assert rc == 0 and np.array_equal(starts, want_starts) and np.array_equal(C.bits(out), C.bits(want))
    flat = np.zeros(100, np.float32)
    for bad in ([(0, 10, 3, 4)], [(50, 10, 6, 10)], [(0, 10, 3, 0)], [(0, 8, 0, 4)], [(-1, 2, 2, 2)]):
        assert _run(emulated, flat, np.array(bad, np.int64), 8, 0)[0] != 0, bad
    assert _run(emulated, flat, np.array([(0, 2, 2, 2)], np.int64), 0, 0)[0] != 0
    assert _run(emulated, flat, np.array([(0, 2, 2, 2)], np.int64), 1025, 0)[0] != 0
    assert _run(emulated, flat, np.array([(0, 2, 2, 2)], np.int64), 8, 2)[0] != 0
    rc, starts, out = _run(emulated, flat, np.zeros((0, 4), np.int64), 8, 1)
    assert rc == 0 and starts.shape == (0,)
