"""csrc/jpeg_scans.hip without a GPU: the kernel source (with csrc/jpeg_decode.hip, which owns the handle) is compiled as host C++
against tests/hip_emu by tests/hip_emu_build.py and must equal the executable contract (tests/jpeg_scans_contract.py) on every case
of tests/jpeg_scans_cases.py, byte and status: inputs and outputs between 0xFF guard bands at odd addresses, frames at odd output
offsets, the scratch (pixel planes and coefficient planes) an allocation of exactly its size.  A single-scan frame passed as a
scan list gives vsc_jpeg_decode_u8's bytes.  The damaged files (a flipped bit in an AC-refine scan, an EOBRUN past the last block,
a scan shortened by one byte, a wrong RSTn) give the contract's status, leave the guards and the bytes between the frames alone and
do not disturb their neighbours.  The same calls then run in a stand-alone program built with -fsanitize=address,undefined
(tests/hip_emu/jpeg_scans_sanitize_main.cpp), started as a child process: nothing sanitized is loaded into Python."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import jpeg_decode_cases as single  # noqa: E402
import jpeg_scans_cases as cases  # noqa: E402

P, I64 = ctypes.c_void_p, ctypes.c_int64
GUARD = 13
BATCH = 32          # files per emulated call


def source():
    return hip_emu_build.emulated_source("jpeg_decode.hip", "jpeg_scans.hip", header="jpeg_decode.h")


class Emulated:
    def __init__(self, lib):
        self.lib = lib

    def run(self, file_list, first_offset=1, gap=5, cap=0, fill=0x5A):
        """one call on a handle of its own -> (rc, status, [frame], chunks); asserts that guards, gaps and inputs are as they were"""
        data, rows, srows, ptr, tables, out_len, outs = cases.call(file_list, first_offset, gap)
        dbuf, dview = hip_emu_build.guarded(len(data), np.uint8, GUARD)
        dview[:] = data
        obuf, oview = hip_emu_build.guarded(out_len, np.uint8, GUARD, fill)
        status = np.full(len(rows) + 2, -7, np.int32)
        h = P()
        assert self.lib.vsc_jpeg_decode_create(None, ctypes.byref(h)) == 0
        if cap:
            assert self.lib.vsc_jpeg_decode_scratch(h, cap, None, None) == 0
        rc = self.lib.vsc_jpeg_decode_scans_u8(h, dview.ctypes.data, len(data), rows.ctypes.data, len(rows), srows.ctypes.data, ptr.ctypes.data, tables.ctypes.data,
                                               len(tables), oview.ctypes.data, out_len, status[1:].ctypes.data)
        chunks = I64(-1)
        assert self.lib.vsc_jpeg_decode_scratch(h, 0, ctypes.byref(chunks), None) == 0
        self.lib.vsc_jpeg_decode_destroy(h)
        assert hip_emu_build.guards_intact(dbuf, GUARD) and hip_emu_build.guards_intact(obuf, GUARD) and status[0] == -7 and status[-1] == -7, "a guard band was written"
        assert np.array_equal(dview, data), "the input was written"
        keep = np.ones(out_len, bool)
        for at, fh, fw in outs:
            keep[at:at + fh * fw * 3] = False
        assert (oview[keep] == fill).all(), "a byte between the frames was written"
        return rc, status[1:-1], [oview[at:at + fh * fw * 3].reshape(fh, fw, 3) for at, fh, fw in outs], chunks.value


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    return Emulated(hip_emu_build.build_shared(tmp_path_factory, "jpeg_scans", source()))


NAMES = cases.names()


@pytest.mark.parametrize("first", range(0, len(NAMES), BATCH))
def test_emulated_kernels_equal_contract(emulated, first):
    """BATCH cases per call: three launches"""
    names = NAMES[first:first + BATCH]
    before = emulated.lib.emu_launches()
    rc, status, frames, chunks = emulated.run([cases.file(n) for n in names])
    assert rc == 0 and (status == 0).all(), (rc, status.tolist())
    assert emulated.lib.emu_launches() - before == 3 and chunks == 1
    for n, got in zip(names, frames):
        ref = cases.contract(n)
        assert got.shape == ref.shape and np.array_equal(got, ref), (n, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())


def test_emulated_single_scan_frames_in_a_mixed_call(emulated):
    files = list(single.files("five_small")) + [cases.file("33x47_420_q75_noise"), single.files("64x48_restart_2_mcus")[0], cases.file("13x17_422_dht_redefined")]
    want = list(single.contract("five_small")) + [cases.contract("33x47_420_q75_noise"), single.contract("64x48_restart_2_mcus")[0], cases.contract("13x17_422_dht_redefined")]
    rc, status, frames, _ = emulated.run(files)
    assert rc == 0 and (status == 0).all()
    assert all(np.array_equal(a, b) for a, b in zip(frames, want))


def test_emulated_chunks(emulated):
    """the scratch of a frame is 3 bytes per padded sample: 13 x 17 4:2:0 is (16 * 32 + 2 * 8 * 16) * 3 = 2304, so a cap of 5000 holds two"""
    files = [cases.file("13x17_420_q75_noise")] * 5
    before = emulated.lib.emu_launches()
    rc, status, frames, chunks = emulated.run(files, cap=5000)
    assert rc == 0 and (status == 0).all() and chunks == 3 and emulated.lib.emu_launches() - before == 9
    assert all(np.array_equal(f, cases.contract("13x17_420_q75_noise")) for f in frames)
    rc, _, frames, chunks = emulated.run(files, cap=1)
    assert rc == 0 and chunks == 5 and all(np.array_equal(f, cases.contract("13x17_420_q75_noise")) for f in frames)


@pytest.mark.parametrize("name", sorted(cases.damaged()))
def test_emulated_damaged_scan_sets_its_status_only(emulated, name):
    data, want = cases.damaged()[name]
    good = [cases.file("33x47_420_q75_noise"), cases.file("16x16_gray_q30_ramp")]
    rc, status, frames, _ = emulated.run([good[0], data, good[1]])
    assert rc == 0 and status.tolist() == [0, want, 0] and want != 0, status.tolist()
    assert np.array_equal(frames[0], cases.contract("33x47_420_q75_noise")) and np.array_equal(frames[2], cases.contract("16x16_gray_q30_ramp"))


def test_emulated_refuses_bad_operands_before_any_launch(emulated):
    data, rows, srows, ptr, tables, out_len, outs = cases.call([cases.file("13x17_420_q75_noise")], 0, 0)
    lib = emulated.lib
    h = P()
    assert lib.vsc_jpeg_decode_create(None, ctypes.byref(h)) == 0
    out = np.full(out_len, 0x5A, np.uint8)
    status = np.full(1, 77, np.int32)
    before = lib.emu_launches()

    def call(rows=rows, srows=srows, ptr=ptr, n=1):
        return lib.vsc_jpeg_decode_scans_u8(h, data.ctypes.data, len(data), rows.ctypes.data, n, srows.ctypes.data, ptr.ctypes.data, tables.ctypes.data, len(tables),
                                            out.ctypes.data, out_len, status.ctypes.data)
    bad = []
    for col, value in ((1, len(data) + 1), (2, 8), (3, 64), (4, 64), (5, 14), (6, 14), (5, 1), (8, len(tables)), (9, 1 << 24), (7, -1), (0, -1)):
        s = srows.copy()
        s[1 if col in (5, 6) else 0, col] = value
        bad.append(call(srows=s))
    s = srows.copy()
    s[[0, 1]] = s[[1, 0]]                       # AC before DC
    bad.append(call(srows=s))
    bad.append(call(srows=srows[:-1].copy(), ptr=np.asarray([0, len(srows) - 1], np.int64)))       # a band left at Al 1
    bad.append(call(ptr=np.asarray([0, 0], np.int64)))
    r = rows.copy()
    r[0, 5] = 3
    bad.append(call(rows=r))
    r = rows.copy()
    r[0, 7] = 1
    bad.append(call(rows=r))
    assert all(rc != 0 for rc in bad), bad
    assert lib.emu_launches() == before and status[0] == 77 and (out == 0x5A).all()
    assert call() == 0 and status[0] == 0 and np.array_equal(out.reshape(13, 17, 3), cases.contract("13x17_420_q75_noise"))
    lib.vsc_jpeg_decode_destroy(h)


def calls_file(path):
    """the calls for tests/hip_emu/jpeg_scans_sanitize_main.cpp (format: its header): every case, BATCH a call, a chunked call and the
    damaged set"""
    pad = lambda a: np.concatenate([np.frombuffer(a.tobytes(), np.uint8), np.zeros(-a.nbytes % 8, np.uint8)]).tobytes()     # noqa: E731
    todo = [([cases.file(n) for n in NAMES[i:i + BATCH]], [cases.contract(n) for n in NAMES[i:i + BATCH]], [0] * len(NAMES[i:i + BATCH]), 0, 0)
            for i in range(0, len(NAMES), BATCH)]
    todo.append(([cases.file("13x17_420_q75_noise")] * 5, [cases.contract("13x17_420_q75_noise")] * 5, [0] * 5, 5000, 3))
    good = ["33x47_420_q75_noise", "16x16_gray_q30_ramp"]
    for data, status in cases.damaged().values():
        todo.append(([cases.file(good[0]), data, cases.file(good[1])], [cases.contract(good[0]), None, cases.contract(good[1])], [0, status, 0], 0, 0))
    blob = [np.int64(len(todo)).tobytes()]
    for file_list, want, expect, cap, chunks in todo:
        data, rows, srows, ptr, tables, out_len, outs = cases.call(file_list, 1, 5)
        ref = np.zeros(out_len, np.uint8)
        for (at, fh, fw), w in zip(outs, want):
            if w is not None:
                ref[at:at + fh * fw * 3] = w.reshape(-1)
        blob.append(np.asarray([len(rows), len(data), len(tables), out_len, cap, chunks, len(srows)], np.int64).tobytes())
        blob += [pad(rows), pad(srows), pad(ptr), np.asarray(expect, np.int64).tobytes(), pad(tables), pad(data), pad(ref)]
    with open(path, "wb") as f:
        f.write(b"".join(blob))
    return len(todo)


def test_emulated_under_the_sanitizers_as_a_child_process(tmp_path):
    exe = hip_emu_build.build_sanitized(tmp_path, source(), "jpeg_scans_sanitize_main.cpp")
    n = calls_file(str(tmp_path / "calls.bin"))
    r = subprocess.run([exe, str(tmp_path / "calls.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"ok ({n} calls" in r.stdout, r.stdout
