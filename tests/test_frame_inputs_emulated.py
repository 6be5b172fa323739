"""csrc/frame_inputs.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads, LDS filled with a pattern before every launch, the
scratch slot filled with 0xFF when fresh) plus tests/hip_emu/frame_inputs.h (the coefficient cache on the host) and must equal
the executable contract (tests/frame_inputs_contract.py) bit for bit on every case of tests/frame_inputs_cases.py small enough for
one OS thread per lane: outputs between 0xFF guard bands at odd byte addresses, all targets of a case in one call, the refusals.
A second build with the LDS budget lowered to 8 bytes sends every target through the two-pass path, which on the device begins
where one output row's vertical support no longer fits 160 KiB (tests/test_gpu_frame_inputs.py runs that shape); a third with
4 KiB splits the fused targets into bands of a few rows fed by one staged source row at a time."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_inputs_cases as cases  # noqa: E402
import hip_emu_build  # noqa: E402

P = ctypes.c_void_p
GUARD = 13          # bytes of 0xFF on both sides of every buffer: odd, so that inputs and outputs start at odd addresses
SMALL = cases.names()


def guarded(nbytes, fill=0xFF):
    return hip_emu_build.guarded(nbytes, np.uint8, GUARD, fill)


def guards_intact(buf):
    return hip_emu_build.guards_intact(buf, GUARD)


class Emulated:
    def __init__(self, lib):
        self.lib = lib
        self.handle = P()
        assert lib.vsc_frame_inputs_create(None, ctypes.byref(self.handle)) == 0

    def close(self):
        self.lib.vsc_frame_inputs_destroy(self.handle)

    def run(self, frames, targets, handle="own", fill=0xFF):
        """-> (rc, [output per target]); the frames sit between guard bands too, at an odd address"""
        frames = np.asarray(frames, np.uint8)
        n, h, w = frames.shape[:3]
        fbuf, fview = guarded(frames.size)
        fview[:] = frames.reshape(-1)
        t = np.ascontiguousarray(np.asarray(targets, np.int32).reshape(-1, 10))
        bufs = [guarded(n * int(r[8]) * int(r[9]) * 3, fill) for r in t]
        ptrs = (P * max(len(t), 1))(*[v.ctypes.data for _, v in bufs])
        rc = self.lib.vsc_frame_inputs_u8(self.handle if handle == "own" else handle, fview.ctypes.data, n, h, w, t.ctypes.data, len(t), ptrs)
        assert guards_intact(fbuf) and all(guards_intact(b) for b, _ in bufs), "a guard band was written"
        return rc, [v.reshape(n, int(r[8]), int(r[9]), 3) for (_, v), r in zip(bufs, t)]


def build(tmp_path_factory, tag, defines=()):
    return Emulated(hip_emu_build.build_shared(tmp_path_factory, "frame_inputs_" + tag, hip_emu_build.source("frame_inputs"), defines))


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    emu = build(tmp_path_factory, "lds")
    yield emu
    emu.close()


@pytest.fixture(scope="module")
def emulated_two_pass(tmp_path_factory):
    """LDS budget 8 bytes: no band of any target fits, every target takes the two launches over the scratch"""
    emu = build(tmp_path_factory, "two_pass", ["-DFI_EMU_LDS_BYTES=8"])
    yield emu
    emu.close()


def check_case(emu, name):
    c = cases.get(name)
    rc, outs = emu.run(c["frames"], c["targets"])
    assert rc == 0
    for t, (got, want) in enumerate(zip(outs, cases.contract(name))):
        assert got.shape == want.shape
        assert np.array_equal(got, want), (name, t, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def vertical_first(target):
    return target[1] - target[0] > 100 * (target[3] - target[2]) and target[4] < target[1] - target[0]


@pytest.mark.parametrize("name", SMALL)
def test_emulated_kernel_equals_contract(emulated, name):
    """all targets of the case in one call; one launch per fused target, two per vertical-first one"""
    before = emulated.lib.emu_launches()
    check_case(emulated, name)
    targets = cases.get(name)["targets"]
    assert emulated.lib.emu_launches() - before == sum(2 if vertical_first(t) else 1 for t in targets)


@pytest.mark.parametrize("name", SMALL)
def test_emulated_two_pass_path_equals_contract(emulated_two_pass, name):
    before = emulated_two_pass.lib.emu_launches()
    check_case(emulated_two_pass, name)
    assert emulated_two_pass.lib.emu_launches() - before == 2 * len(cases.get(name)["targets"])
    assert emulated_two_pass.lib.emu_scratch_bytes(-1) > 0


@pytest.fixture(scope="module")
def emulated_bands(tmp_path_factory):
    """LDS budget 4 KiB: the targets that still fit do so with one staged source row at a time and bands of a few output rows"""
    emu = build(tmp_path_factory, "bands", ["-DFI_EMU_LDS_BYTES=4096"])
    yield emu
    emu.close()


@pytest.mark.parametrize("name", SMALL)
def test_emulated_small_bands_equal_contract(emulated_bands, name):
    check_case(emulated_bands, name)


def test_emulated_band_count_does_not_divide_the_rows(emulated_bands):
    """64 x 48 -> a 23 x 19 window under 4 KiB: one fused launch whose 23 output rows (a prime) split into several bands per frame"""
    lib = emulated_bands.lib
    launches, blocks = lib.emu_launches(), lib.emu_blocks()
    check_case(emulated_bands, "64x48_rect_window")
    assert lib.emu_launches() - launches == 1
    bands = (lib.emu_blocks() - blocks) // 2
    assert bands > 1 and (lib.emu_blocks() - blocks) % 2 == 0 and 23 % bands != 0, bands


def test_emulated_tables_are_built_once(emulated):
    check_case(emulated, "64x48_rect_window")
    tables = emulated.lib.emu_coeff_tables()
    check_case(emulated, "64x48_rect_window")
    assert emulated.lib.emu_coeff_tables() == tables


def test_emulated_refusals_write_nothing(emulated, emulated_two_pass):
    for emu in (emulated, emulated_two_pass):
        frames = cases.get("37x53_sq17_sq24_clip24")["frames"]
        good = (0, 37, 0, 53, 17, 17, 0, 0, 17, 17)

        def refused(targets, handle="own", fr=frames):
            rc, outs = emu.run(fr, targets, handle=handle, fill=0x5A)
            assert rc != 0, targets
            assert all((o == 0x5A).all() for o in outs), "a refused call wrote"

        refused([good], handle=None)                                            # no handle
        for box in ((-1, 37, 0, 53), (0, 38, 0, 53), (0, 37, -1, 53), (0, 37, 0, 54), (5, 5, 0, 53), (0, 37, 9, 9), (6, 5, 0, 53)):
            refused([box + good[4:]])                                           # a box outside the frame, or empty
        for oh, ow in ((0, 17), (17, 0), (4097, 17), (17, 4097), (-1, 17)):
            refused([(0, 37, 0, 53, oh, ow, 0, 0, 1, 1)])                       # output sides outside 1 .. 4096
        for win in ((-1, 0, 17, 17), (0, -1, 17, 17), (1, 0, 17, 17), (0, 1, 17, 17), (0, 0, 18, 17), (0, 0, 17, 18), (16, 16, 2, 1)):
            refused([good[:6] + win])                                           # a window outside the output
        refused([good, (0, 38, 0, 53) + good[4:]])                              # a bad target after a good one: nothing launched
        lib, h = emu.lib, emu.handle
        t = np.asarray([good], np.int32)
        out = np.full(2 * 17 * 17 * 3, 0x5A, np.uint8)
        ptrs = (P * 1)(out.ctypes.data)
        f = np.ascontiguousarray(frames)
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, -1, 37, 53, t.ctypes.data, 1, ptrs) != 0          # n below 0
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, 2, 37, 53, t.ctypes.data, 1, (P * 1)(None)) != 0  # a null output
        assert lib.vsc_frame_inputs_u8(h, None, 2, 37, 53, t.ctypes.data, 1, ptrs) != 0                    # no frames
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, 2, 37, 53, None, 1, ptrs) != 0                    # no target table
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, 2, 37, 53, t.ctypes.data, 1, None) != 0           # no output table
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, 2, 0, 53, t.ctypes.data, 1, ptrs) != 0
        assert (out == 0x5A).all(), "a refused call wrote"
        launches = lib.emu_launches()
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, 0, 37, 53, t.ctypes.data, 1, ptrs) == 0           # no frames: nothing launched
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, 2, 37, 53, None, 0, None) == 0                    # no targets
        empty = np.asarray([good[:8] + (0, 17)], np.int32)
        assert lib.vsc_frame_inputs_u8(h, f.ctypes.data, 2, 37, 53, empty.ctypes.data, 1, (P * 1)(None)) == 0   # an empty window needs no output
        assert lib.emu_launches() == launches and (out == 0x5A).all()
        assert lib.vsc_frame_inputs_create(None, None) != 0
        check_case(emu, "37x53_sq17_sq24_clip24")                               # and the entry still works
