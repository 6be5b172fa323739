"""csrc/match_segments.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads and the wave intrinsics) and must equal the executable
contract (tests/seg_contract.py) on small fixture maps.  This checks the kernel's logic phase by phase -- the label sweeps, the size
counters, the ranking, the point lookup, the MT19937 subset stream, the trial loop and the final fit; the GPU suite
(tests/test_gpu_match_segments.py) checks the same on the device for every fixture entry."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import seg_cases  # noqa: E402
import seg_contract  # noqa: E402

# One small map per phase variant, so the run stays under a minute (every workgroup is 512 OS threads): a group below 200 points
# (permutation head), groups above it (tracking selection), several large components, dx = 0 trials, degenerate shapes.
CASES = ["clean_00_40x50", "thick_05_40x50", "edge_empty", "edge_1x1", "edge_4x4", "edge_specks_only", "edge_query_frame_rows_only",
         "edge_all_above_small"]


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    lib = hip_emu_build.build_shared(tmp_path_factory, "match_segments", hip_emu_build.source("match_segments"))
    return lib.vsc_match_segments_f32


def _run(fn, m, slots=8):
    thr = np.array([p[0] for p in seg_cases.PASSES], np.float32)
    ratio = np.array([p[1] for p in seg_cases.PASSES], np.float64)
    items = np.array([[0, m.shape[0], m.shape[1]]], np.int64)
    flat = np.ascontiguousarray(m.reshape(-1)) if m.size else np.zeros(1, np.float32)
    seg, sc, cnt = np.zeros((3, slots, 4), np.int32), np.zeros((3, slots), np.float64), np.full(3, -1, np.int32)
    assert fn(flat.ctypes.data, m.size, items.ctypes.data, 1, thr.ctypes.data, ratio.ctypes.data, 3, slots, seg.ctypes.data,
              sc.ctypes.data, cnt.ctypes.data, None) == 0
    return seg, sc, cnt


@pytest.mark.parametrize("name", CASES)
def test_emulated_kernel_equals_contract(emulated, name):
    m = seg_cases.matrix(seg_cases.by_name()[name])
    seg, sc, cnt = _run(emulated, m)
    for t, (thr, ratio) in enumerate(seg_cases.PASSES):
        want, report = seg_contract.segments(m, thr, ratio)
        if report["margin"] < seg_contract.KNIFE_EDGE:
            continue
        got = [[*(int(v) for v in seg[t, k]), float(sc[t, k])] for k in range(int(cnt[t]))]
        assert int(cnt[t]) == len(want) and [g[:4] for g in got] == [w[:4] for w in want], (name, thr, got, want)
        assert np.allclose([g[4] for g in got], [w[4] for w in want], rtol=0, atol=1e-9), (name, thr, got, want)


def test_emulated_kernel_reports_uncapped_counts(emulated):
    m = np.zeros((60, 80), np.float32)
    for b, (q0, r0) in enumerate([(1, 2), (20, 40), (40, 5)]):
        for t in range(15):
            m[q0 + t, r0 + t] = 0.9 - 0.05 * b - 0.002 * t
    want, _ = seg_contract.segments(m, 0.35, 0.5)
    assert len(want) == 3
    seg, sc, cnt = _run(emulated, m, slots=1)
    assert int(cnt[0]) == 3 and [int(v) for v in seg[0, 0]] == want[0][:4]
