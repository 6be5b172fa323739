"""csrc/score_norm.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads and the wave intrinsics), its own C entry points
included, with -ffp-contract=off, and must equal the executable contract
(tests/score_norm_contract.py) bit for bit: the staging of row tiles and which rows and columns are read, the order of the chains,
the logical column index of the narrowed row, the lane sums and the butterfly, the three summation forms of the bias, the refusals.
The GPU suite (tests/test_gpu_score_norm.py) checks the same on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import score_norm_cases as cases  # noqa: E402
import score_norm_contract as C  # noqa: E402

P = ctypes.c_void_p
GUARD = 8       # floats of 0xFF bytes (NaN) before and behind every output, which is filled with them too


class Emulated:
    def __init__(self, lib):
        self.lib = lib
        self.handle = P()
        assert lib.vsc_score_norm_create(None, ctypes.byref(self.handle)) == 0

    def close(self):
        self.lib.vsc_score_norm_destroy(self.handle)

    @staticmethod
    def guarded(count):
        return hip_emu_build.guarded(count, np.float32, GUARD)

    @staticmethod
    def guards_intact(buf):
        return hip_emu_build.guards_intact(buf, GUARD)

    def column_var(self, x, n, d, ld):
        buf, out = self.guarded(d)
        rc = self.lib.vsc_column_var_f32(self.handle, x.ctypes.data, n, d, ld, out.ctypes.data)
        assert self.guards_intact(buf)
        return rc, out

    def rows(self, x, n, d, ldx, drop, normalize, append, last, ldo):
        wo = d - (drop >= 0) + (append != 0)
        buf, out = self.guarded(max(n, 1) * ldo)
        rc = self.lib.vsc_score_norm_rows_f32(self.handle, x.ctypes.data, n, d, ldx, drop, normalize, append,
                                              None if last is None else last.ctypes.data, out.ctypes.data, ldo)
        assert self.guards_intact(buf)
        out = out.reshape(max(n, 1), ldo)
        return rc, out[:n, :wo], out[:n, wo:]

    def bias(self, topk, nq, ldk, nk, beta, gate):
        buf, out = self.guarded(nq)
        rc = self.lib.vsc_score_norm_bias_f32(self.handle, topk.ctypes.data, nq, ldk, nk, np.float32(-beta),
                                              None if gate is None else gate.ctypes.data, out.ctypes.data)
        assert self.guards_intact(buf)
        return rc, out


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    emu = Emulated(hip_emu_build.build_shared(tmp_path_factory, "score_norm", hip_emu_build.source("score_norm")))
    yield emu
    emu.close()


@pytest.mark.parametrize("n,d,ld", cases.VAR_SHAPES)
def test_emulated_column_var_equals_contract(emulated, n, d, ld):
    x = cases.offset_rows(n, d, ld)
    rc, var = emulated.column_var(x, n, d, ld)
    want = C.column_var(x[:, :d])
    assert rc == 0 and np.array_equal(C.bits(var), C.bits(want)), np.nonzero(C.bits(var) != C.bits(want))[0][:10]
    assert np.array_equal(C.bits(want), C.bits(np.ascontiguousarray(x[:, :d]).var(axis=0)))


def test_emulated_column_var_first_minimum_and_refusals(emulated):
    x = cases.offset_rows(200, 70)
    x[:, 66] = x[:, 3]                                   # two identical columns: the same bits, argmin is the first
    x[:, [3, 66]] *= np.float32(1e-3)
    rc, var = emulated.column_var(x, 200, 70, 70)
    assert rc == 0 and C.bits(var)[3] == C.bits(var)[66] and int(np.argmin(var)) == 3 == C.low_variance_dim(x)
    lib, h, out = emulated.lib, emulated.handle, np.zeros(4, np.float32)
    assert lib.vsc_column_var_f32(h, x.ctypes.data, 0, 70, 70, out.ctypes.data) != 0     # no rows
    assert lib.vsc_column_var_f32(h, x.ctypes.data, 200, 0, 70, out.ctypes.data) != 0
    assert lib.vsc_column_var_f32(h, x.ctypes.data, 200, 70, 69, out.ctypes.data) != 0    # stride below the width
    assert lib.vsc_column_var_f32(h, None, 200, 70, 70, out.ctypes.data) != 0
    assert lib.vsc_column_var_f32(h, x.ctypes.data, 200, 70, 70, None) != 0
    assert lib.vsc_column_var_f32(None, x.ctypes.data, 200, 70, 70, out.ctypes.data) != 0    # no handle


@pytest.mark.parametrize("d", cases.ROWS_D)
def test_emulated_rows_equal_contract(emulated, d):
    """every drop, append mode and normalize flag at this width; padded strides whose padding stays NaN; the zero row and the row
    whose squares underflow come back unchanged"""
    ldx = d + 3
    x = cases.descriptor_rows(d, ldx)
    n = len(x)
    last = np.arange(n, dtype=np.float32) * np.float32(-0.37) - np.float32(100.0)
    for drop in cases.drops(d):
        for append in (0, 1, 2):
            for normalize in (0, 1):
                wo = d - (drop >= 0) + (append != 0)
                if wo == 0:
                    continue
                rc, out, pad = emulated.rows(x, n, d, ldx, drop, normalize, append, last, wo + 2)
                want = C.rows(x[:, :d], drop, bool(normalize), append, last)
                assert rc == 0 and np.array_equal(C.bits(out), C.bits(want)), (d, drop, append, normalize)
                assert np.isnan(pad).all()
                for r in (2, 4):
                    assert np.array_equal(C.bits(out[r, :wo - (append != 0)]), C.bits(np.delete(x[r, :d], drop if drop >= 0 else [])))


def test_emulated_rows_empty_and_refusals(emulated):
    x = cases.descriptor_rows(8, 8)
    lib = emulated.lib
    rc, out, _ = emulated.rows(x, 0, 8, 8, 3, 1, 1, None, 8)
    assert rc == 0 and out.size == 0                                                          # n = 0: nothing launched
    out = np.zeros((6, 9), np.float32)
    call = lambda *a: lib.vsc_score_norm_rows_f32(emulated.handle, *a)
    assert call(x.ctypes.data, 6, 8, 8, 8, 1, 0, None, out.ctypes.data, 9) != 0         # drop == d
    assert call(x.ctypes.data, 6, 8, 8, -2, 1, 0, None, out.ctypes.data, 9) != 0
    assert call(x.ctypes.data, 6, 8, 8, 0, 2, 0, None, out.ctypes.data, 9) != 0         # normalize
    assert call(x.ctypes.data, 6, 8, 8, 0, 1, 3, None, out.ctypes.data, 9) != 0         # append
    assert call(x.ctypes.data, 6, 8, 8, 0, 1, 2, None, out.ctypes.data, 9) != 0         # append = 2 without the column
    assert call(x.ctypes.data, 6, 8, 7, 0, 1, 0, None, out.ctypes.data, 9) != 0         # ldx < d
    assert call(x.ctypes.data, 6, 8, 8, -1, 1, 1, None, out.ctypes.data, 8) != 0        # ldo < 9
    assert call(x.ctypes.data, -1, 8, 8, 0, 1, 0, None, out.ctypes.data, 9) != 0
    # overlapping out: in place, shifted by one row, and ending inside x
    big = np.zeros(6 * 8 + 6 * 9, np.float32)
    xin = big[:48]
    assert call(xin.ctypes.data, 6, 8, 8, 0, 1, 0, None, xin.ctypes.data, 8) != 0
    assert call(xin.ctypes.data, 6, 8, 8, 0, 1, 0, None, big[8:].ctypes.data, 8) != 0
    assert call(big[40:].ctypes.data, 6, 8, 8, 0, 1, 0, None, big.ctypes.data, 7) != 0
    assert call(xin.ctypes.data, 6, 8, 8, 0, 1, 0, None, big[48:].ctypes.data, 7) == 0  # adjacent is not overlapping


@pytest.mark.parametrize("nk", cases.NKS)
def test_emulated_bias_equals_contract(emulated, nk):
    nq, ldk = 300, nk + 3                                  # two workgroups, padded rows
    topk, gate = cases.topk_scores(nq, nk, ldk)
    for beta in (1.2, 1.5):
        for g in (None, gate):
            rc, out = emulated.bias(topk, nq, ldk, nk, beta, g)
            want = C.bias(topk, nk, beta, g)
            assert rc == 0 and np.array_equal(C.bits(out), C.bits(want)), (nk, beta, g is not None)
            if g is not None:
                assert (out[gate != 0] == np.float32(-100.0)).all() and (out[gate == 0] != np.float32(-100.0)).all()


def test_emulated_bias_refusals(emulated):
    topk, gate = cases.topk_scores(4, 129, 130)
    out = np.zeros(4, np.float32)
    call = lambda *a: emulated.lib.vsc_score_norm_bias_f32(emulated.handle, *a)
    assert call(topk.ctypes.data, 4, 130, 129, -1.0, None, out.ctypes.data) != 0        # numpy's sum recurses beyond 128
    assert call(topk.ctypes.data, 4, 130, 0, -1.0, None, out.ctypes.data) != 0
    assert call(topk.ctypes.data, 4, 7, 8, -1.0, None, out.ctypes.data) != 0            # ldk < nk
    assert call(None, 4, 130, 8, -1.0, None, out.ctypes.data) != 0
    assert call(None, 0, 130, 8, -1.0, None, None) == 0                                 # nq = 0: nothing launched
    rc, got = emulated.bias(topk, 4, 130, 128, 1.0, None)
    assert rc == 0 and np.array_equal(C.bits(got), C.bits(C.bias(topk, 128, 1.0)))
