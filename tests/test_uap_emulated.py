"""csrc/uap.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads and the wave intrinsics, one scratch buffer per
slot, filled with 0xFF when fresh) with -ffp-contract=off, and must equal the executable contract (tests/uap_contract.py) on uint64
views: the sort key, the stable ranking over tiles, the skipped digit passes, the duplicate counts, the join, the two scans, where the
curve is written, the reversed group terms, the walk through numpy's summation tree, the refusals.  Every case up to 2 500 predictions;
the GPU suite (tests/test_gpu_uap.py) checks the same, and the larger cases, on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import uap_cases as cases  # noqa: E402
import uap_contract as C  # noqa: E402
from hip_emu_build import guarded, guards_intact  # noqa: E402     (guards of 8 elements of 0xFF bytes; as floats NaN)

P = ctypes.c_void_p


class Emulated:
    def __init__(self, lib):
        self.lib = lib
        self.handle = P()
        assert lib.vsc_uap_create(None, ctypes.byref(self.handle)) == 0

    def close(self):
        self.lib.vsc_uap_destroy(self.handle)

    def rank(self, scores, pred_keys, gt_keys, key_bits):
        n, g = len(scores), len(gt_keys)
        scores, pred_keys, gt_keys = (np.ascontiguousarray(a, t) for a, t in ((scores, np.float64), (pred_keys, np.uint64), (gt_keys, np.uint64)))
        bufs = [guarded(n, np.int64), guarded(n, np.float64), guarded(n, np.uint8), guarded(4, np.int64)]
        rc = self.lib.vsc_uap_rank_f64(self.handle, scores.ctypes.data, pred_keys.ctypes.data, n, gt_keys.ctypes.data, g, key_bits,
                                       *(v.ctypes.data for _, v in bufs))
        assert all(guards_intact(b) for b, _ in bufs)
        return (rc, *(v for _, v in bufs))

    def curve(self, ranked, correct, n_gt):
        n = len(ranked)
        ranked, correct = np.ascontiguousarray(ranked, np.float64), np.ascontiguousarray(correct, np.uint8)
        bufs = [guarded(2, np.float64), guarded(2, np.int64), guarded(3 * n, np.float64)]
        rc = self.lib.vsc_uap_curve_f64(self.handle, ranked.ctypes.data, correct.ctypes.data, n, n_gt, *(v.ctypes.data for _, v in bufs))
        assert all(guards_intact(b) for b, _ in bufs)
        return rc, bufs[0][1], bufs[1][1], bufs[2][1].reshape(3, n)


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    emu = Emulated(hip_emu_build.build_shared(tmp_path_factory, "uap", hip_emu_build.source("uap")))
    yield emu
    emu.close()


def check_case(emulated, case):
    pk, gk = cases.keys(case)
    n, g = len(pk), len(gk)
    rc, perm, ranked, correct, status = emulated.rank(case["scores"], pk, gk, case["key_bits"])
    assert rc == 0
    want = C.rank(case["scores"], pk, gk, case["key_bits"])
    assert np.array_equal(status, want[3]), (status, want[3])
    assert np.array_equal(perm, want[0]), np.nonzero(perm != want[0])[0][:10]
    assert np.array_equal(C.bits(ranked), C.bits(want[1])) and np.array_equal(correct, want[2])
    if g == 0:
        return
    rc, sums, counts, curve = emulated.curve(ranked, correct, g)
    assert rc == 0
    wsums, wcounts, wcurve = C.curve(want[1], want[2], g)
    n_pos = int(wcounts[0])
    assert np.array_equal(counts, wcounts), (counts, wcounts)
    assert np.array_equal(C.bits(sums), C.bits(wsums)), (sums, wsums)
    assert np.array_equal(C.bits(curve[:, :n_pos]), C.bits(wcurve))
    assert (curve[:, n_pos:].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "columns beyond n_pos were written"


@pytest.mark.parametrize("name", [c for c in cases.names(cases.EMULATED_MAX) if cases.get(c)["scores"].size])
def test_emulated_entries_equal_contract(emulated, name):
    """every case with predictions up to 2 500, the refused ones included: their status counts what is wrong and the call completes"""
    check_case(emulated, cases.get(name))


def test_emulated_status_of_the_refusals(emulated):
    for name, slot in (("refuse_nan", 0), ("refuse_inf", 0), ("refuse_duplicate_prediction", 1), ("refuse_duplicate_ground_truth", 2)):
        case = cases.get(name)
        pk, gk = cases.keys(case)
        rc, _, _, _, status = emulated.rank(case["scores"], pk, gk, case["key_bits"])
        assert rc == 0 and status[slot] == 1 and status[[s for s in range(3) if s != slot]].tolist() == [0, 0], (name, status)


def test_emulated_group_counts_cross_the_tree_thresholds(emulated):
    """the number of tie groups crosses 7 / 8, 128 / 129 and the chunk of 8192 independently of n: scores with exactly G groups"""
    rs = np.random.RandomState(5)
    for n, groups in ((40, 7), (40, 8), (300, 128), (300, 129), (300, 137), (2400, 1025)):
        s = np.sort(np.r_[np.arange(groups), rs.randint(0, groups, n - groups)])[::-1].astype(np.float32).astype(np.float64) * 0.25 - 9.0
        correct = (rs.rand(n) < 0.3).astype(np.uint8)
        rc, sums, counts, curve = emulated.curve(s, correct, int(correct.sum()) + 3)
        wsums, wcounts, wcurve = C.curve(s, correct, int(correct.sum()) + 3)
        assert rc == 0 and wcounts[1] == groups and np.array_equal(counts, wcounts)
        assert np.array_equal(C.bits(sums), C.bits(wsums)) and np.array_equal(C.bits(curve[:, :wcounts[0]]), C.bits(wcurve))


def test_emulated_long_sum_crosses_numpy_chunks(emulated):
    """9 000 rows, all distinct: both sums run over more than one chunk of 8192 (one tile pass more than the cases above; the
    ranking is not repeated here)"""
    rs = np.random.RandomState(6)
    n = 9000
    s = (np.arange(n, 0, -1) * 1e-3).astype(np.float32).astype(np.float64)
    correct = (rs.rand(n) < 0.2).astype(np.uint8)
    rc, sums, counts, curve = emulated.curve(s, correct, int(correct.sum()))
    wsums, wcounts, wcurve = C.curve(s, correct, int(correct.sum()))
    assert rc == 0 and wcounts[1] == n and np.array_equal(counts, wcounts)
    assert np.array_equal(C.bits(sums), C.bits(wsums)) and np.array_equal(C.bits(curve[:, :wcounts[0]]), C.bits(wcurve))


def test_emulated_refusals_and_empty_calls(emulated):
    lib, h = emulated.lib, emulated.handle
    s, k, out = np.ones(4), np.arange(4, dtype=np.uint64), np.zeros(16, np.int64)
    a = lambda x: x.ctypes.data     # noqa: E731
    rank = lambda n, g, bits, *p: lib.vsc_uap_rank_f64(h, a(s), a(k), n, a(k), g, bits, *p)     # noqa: E731
    good = (a(out), a(s.copy()), a(out), a(out))
    assert rank(-1, 4, 20, *good) != 0 and rank(4, -1, 20, *good) != 0
    assert rank(4, 4, 0, *good) != 0 and rank(4, 4, 65, *good) != 0
    assert rank(1 << 31, 4, 20, *good) != 0
    assert rank(4, 4, 20, None, good[1], good[2], good[3]) != 0 and rank(4, 4, 20, good[0], good[1], good[2], None) != 0
    assert lib.vsc_uap_rank_f64(h, a(s), a(k), 4, None, 2, 20, *good) != 0                     # g > 0 without keys
    assert lib.vsc_uap_rank_f64(None, a(s), a(k), 4, a(k), 4, 20, *good) != 0                  # no handle
    assert lib.vsc_uap_rank_f64(h, None, None, 0, None, 0, 20, None, None, None, None) == 0    # n = 0: nothing launched
    ones = np.ones(4, np.uint8)
    curve = lambda n, n_gt, *p: lib.vsc_uap_curve_f64(h, a(s), a(ones), n, n_gt, *p)     # noqa: E731
    cgood = (a(np.zeros(2)), a(out), a(np.zeros(12)))
    assert curve(-1, 3, *cgood) != 0 and curve(4, 0, *cgood) != 0 and curve(4, 3, None, cgood[1], cgood[2]) != 0
    assert lib.vsc_uap_curve_f64(None, a(s), a(ones), 4, 3, *cgood) != 0                       # no handle
    assert lib.vsc_uap_curve_f64(h, None, None, 0, 3, None, None, None) == 0                   # n = 0: nothing launched
    assert lib.vsc_uap_create(None, None) != 0
    check_case(emulated, cases.get("n129_ties"))                                               # and the entries still work


def test_emulated_scratch_is_reused_across_sizes(emulated):
    """growing and shrinking sizes back to back on the same grow-only slots: a smaller call after a larger one finds the larger
    call's leftovers in every buffer and must not read them; the slots grow only when a call needs more"""
    order = ["n257_ties", "n9_distinct", "n2049_ties", "n128_distinct", "n1000_ties", "n1_distinct", "n2500_distinct", "n7_ties"]
    check_case(emulated, cases.get("n2500_ties"))
    before = emulated.lib.emu_scratch_allocs()
    for name in order:
        check_case(emulated, cases.get(name))
    assert emulated.lib.emu_scratch_allocs() == before, "a call no larger than an earlier one grew the scratch"


def test_emulated_grown_sort_tile(emulated, tmp_path_factory):
    """built with VSC_SORT_MAX_TILES = 1: the 2 500 predictions take one tile of 2 560, ten rounds of one workgroup, where the plain
    build takes two tiles of 2 048 in each of its 8 + 3 digit passes over them"""
    grown = Emulated(hip_emu_build.build_shared(tmp_path_factory, "uap_grown", hip_emu_build.source("uap"), ["-DVSC_SORT_MAX_TILES=1"]))
    blocks = []
    for emu in (emulated, grown):
        before = emu.lib.emu_blocks()
        check_case(emu, cases.get("n2500_ties"))
        blocks.append(emu.lib.emu_blocks() - before)
    grown.close()
    assert blocks[0] - blocks[1] == (8 + 3) * 2 * (2 - 1), blocks      # (histogram, scatter) x one tile fewer
