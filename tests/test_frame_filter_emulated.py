"""csrc/frame_filter.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads and the wave intrinsics, LDS filled with a pattern
before every launch, the scratch slot filled with 0xFF when fresh) with -ffp-contract=off, and must equal the executable contract
(tests/frame_filter_contract.py): kept rows, counts, the bits of the means, the visit order -- every case up to 300 rows, single and
batched at odd offsets, more items than one launch holds, outputs between 0xFF guard bands with the -1 tails intact, the refusals.
A second build with the LDS budget lowered to 2 KiB sends every matrix of 86 rows and more through the scratch path, which on the
device begins at 1 089 rows (tests/test_gpu_frame_filter.py runs those)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_filter_cases as cases  # noqa: E402
import frame_filter_contract as C  # noqa: E402
import hip_emu_build  # noqa: E402
from hip_emu_build import guarded, guards_intact  # noqa: E402     (guards of 8 elements of 0xFF bytes: -1 as int32, NaN as float32)

P = ctypes.c_void_p
SMALL = cases.names(cases.EMULATED_MAX)


class Emulated:
    def __init__(self, lib):
        self.lib = lib
        self.handle = P()
        assert lib.vsc_frame_filter_create(None, ctypes.byref(self.handle)) == 0

    def close(self):
        self.lib.vsc_frame_filter_destroy(self.handle)

    def run(self, flat, items, thr, optional=True):
        """-> (rc, kept, counts, means, order); the optional outputs are NULL with optional=False"""
        flat = np.ascontiguousarray(flat, np.float32)
        items = np.ascontiguousarray(items, np.int64).reshape(-1, 2)
        n, total = len(items), int(items[:, 1].sum())
        bufs = [guarded(total, np.int32), guarded(n, np.int32), guarded(total, np.float32), guarded(total, np.int32)]
        ptrs = [v.ctypes.data for _, v in bufs]
        if not optional:
            ptrs[2] = ptrs[3] = None
        rc = self.lib.vsc_frame_filter_f32(self.handle, flat.ctypes.data, flat.size, items.ctypes.data, n, thr, *ptrs)
        assert all(guards_intact(b) for b, _ in bufs)
        return (rc, *(v for _, v in bufs))


def build(tmp_path_factory, tag, defines=()):
    return Emulated(hip_emu_build.build_shared(tmp_path_factory, "frame_filter_" + tag, hip_emu_build.source("frame_filter"), defines))


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    emu = build(tmp_path_factory, "lds")
    yield emu
    emu.close()


@pytest.fixture(scope="module")
def emulated_scratch(tmp_path_factory):
    """LDS budget 2 KiB: 8 L (1 + ceil(L / 64)) exceeds it from L = 86 on, so every matrix of 86 rows and more keeps its
    adjacency bits in the scratch"""
    emu = build(tmp_path_factory, "scratch", ["-DFF_EMU_LDS_BYTES=2048"])
    yield emu
    emu.close()


def assert_item(name, s, thr, kept, count, means=None, order=None):
    want_kept, want_mean, want_order = C.keep(s, thr)
    L = len(s)
    assert count == len(want_kept), (name, count, len(want_kept))
    assert kept[:count].tolist() == want_kept.tolist(), (name, "kept rows")
    assert (kept[count:] == -1).all(), (name, "the tail is not -1")
    if means is not None:
        assert np.array_equal(means.view(np.uint32), C.bits(want_mean)), (name, "mean bits", np.nonzero(means.view(np.uint32) != C.bits(want_mean))[0][:8])
        assert order.tolist() == want_order.tolist(), (name, "visit order")
    assert len(kept) == L


def check_case(emu, name):
    case = cases.get(name)
    s, L = case["s"], len(case["s"])
    rc, kept, counts, means, order = emu.run(s.reshape(-1), [(0, L)], case["thr"])
    assert rc == 0
    assert_item(name, s, case["thr"], kept, int(counts[0]), means, order)
    rc, kept2, counts2, means2, order2 = emu.run(s.reshape(-1), [(0, L)], case["thr"], optional=False)
    assert rc == 0 and np.array_equal(kept2, kept) and np.array_equal(counts2, counts)
    assert (means2.view(np.uint32) == 0xFFFFFFFF).all() and (order2 == -1).all(), "a NULL output was written somewhere else"


@pytest.mark.parametrize("name", SMALL)
def test_emulated_kernel_equals_contract(emulated, name):
    check_case(emulated, name)


@pytest.mark.parametrize("name", [n for n in SMALL if len(cases.get(n)["s"]) >= 63])
def test_emulated_scratch_path_equals_contract(emulated_scratch, name):
    """the same source with the adjacency bits in the scratch (0xFF when fresh, larger leftovers afterwards)"""
    before = emulated_scratch.lib.emu_scratch_bytes(-1)
    check_case(emulated_scratch, name)
    L = len(cases.get(name)["s"])
    if 8 * L * (1 + (L + 63) // 64) > 2048:
        assert emulated_scratch.lib.emu_scratch_bytes(-1) >= max(before, 8 * L * ((L + 63) // 64))
    else:
        assert emulated_scratch.lib.emu_scratch_bytes(-1) == before


def check_batch(emu, flat, items, mats, thr):
    rc, kept, counts, means, order = emu.run(flat, items, thr)
    assert rc == 0
    at = 0
    for k, s in enumerate(mats):
        L = len(s)
        assert_item(f"item {k}", s, thr, kept[at:at + L], int(counts[k]), means[at:at + L], order[at:at + L])
        at += L
    assert at == len(kept)


def test_emulated_batch_of_mixed_sizes_at_odd_offsets(emulated, emulated_scratch):
    """every case at the default threshold in one call, empty items among them, matrices at element offsets that are no multiples of
    64 with NaN between them; in the low-budget build LDS and scratch items share the launch and the scratch slices do not overlap"""
    sel = cases.default_thr_names(cases.EMULATED_MAX)
    flat, items = cases.batch(sel)
    mats = [cases.get(n)["s"] for n in sel]
    check_batch(emulated, flat, items, mats, cases.THR)
    check_batch(emulated_scratch, flat, items, mats, cases.THR)


def test_emulated_more_items_than_one_launch(emulated):
    flat, items, mats = cases.many_small()
    check_batch(emulated, flat, items, mats, cases.THR)


def test_emulated_refusals_write_nothing(emulated):
    lib, h = emulated.lib, emulated.handle
    s = cases.get("planted_65")["s"]
    flat = np.ascontiguousarray(s.reshape(-1))
    a = lambda x: x.ctypes.data     # noqa: E731
    bufs = [guarded(65, np.int32), guarded(1, np.int32), guarded(65, np.float32), guarded(65, np.int32)]
    out = [a(v) for _, v in bufs]
    call = lambda hh, f, flen, it, n, thr, *o: lib.vsc_frame_filter_f32(hh, f, flen, a(np.asarray(it, np.int64)) if it is not None else None, n, thr, *o)     # noqa: E731
    assert call(None, a(flat), flat.size, [0, 65], 1, 0.975, *out) != 0                       # no handle
    assert call(h, a(flat), flat.size, [0, 4097], 1, 0.975, *out) != 0                        # above the row limit
    assert call(h, a(flat), flat.size, [1, 65], 1, 0.975, *out) != 0                          # runs past sims_len
    assert call(h, a(flat), flat.size, [flat.size + 1, 0], 1, 0.975, *out) != 0               # starts past sims_len
    assert call(h, a(flat), flat.size, [-1, 3], 1, 0.975, *out) != 0 and call(h, a(flat), flat.size, [0, -3], 1, 0.975, *out) != 0
    assert call(h, a(flat), flat.size, [0, 65], -1, 0.975, *out) != 0 and call(h, a(flat), -1, [0, 0], 1, 0.975, *out) != 0
    assert call(h, a(flat), flat.size, None, 1, 0.975, *out) != 0                             # no item table
    assert call(h, None, flat.size, [0, 65], 1, 0.975, *out) != 0                             # no similarities
    assert call(h, a(flat), flat.size, [0, 65], 1, 0.975, None, *out[1:]) != 0                # no kept
    assert call(h, a(flat), flat.size, [0, 65], 1, 0.975, out[0], None, *out[2:]) != 0        # no counts
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(h, a(flat), flat.size, [0, 65], 1, bad, *out) != 0
    assert call(h, a(flat), flat.size, [0, 65, 0, 4097], 2, 0.975, *out) != 0                 # a bad item after a good one: nothing launched
    assert all((b.view(np.uint8) == 0xFF).all() for b, _ in bufs), "a refused call wrote"
    assert call(h, None, 0, None, 0, 0.975, None, None, None, None) == 0                      # no items: nothing launched
    assert call(h, None, 0, [0, 0], 1, 0.975, None, out[1], None, None) == 0 and bufs[1][1][0] == 0   # one empty video: count 0
    assert lib.vsc_frame_filter_create(None, None) != 0
    check_case(emulated, "planted_65")                                                        # and the entry still works
