"""csrc/jpeg_decode.hip without a GPU: the kernel source is compiled as host C++ against tests/hip_emu/common.h by
tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads, device allocations as exactly sized host
allocations filled with 0xFF) plus tests/hip_emu/jpeg_decode.h (the wave-uniform marker as the identity) and must equal the executable
contract (tests/jpeg_decode_contract.py) bit for bit on every case of tests/jpeg_decode_cases.py small enough for one OS thread per lane:
bytes and outputs between 0xFF guard bands at odd addresses, frames at odd output offsets.  Damaged scans (a scan cut at a third,
a flipped byte, a deleted RSTn) give a status other than 0, leave the guards and the bytes between the frames alone and do not
disturb the other frames of their call.  The same cases then run in a stand-alone program built with -fsanitize=address,undefined
(tests/hip_emu/jpeg_decode_sanitize_main.cpp), started as a child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hip_emu_build  # noqa: E402
import jpeg_decode_cases as cases  # noqa: E402

P, I64 = ctypes.c_void_p, ctypes.c_int64
GUARD = 13          # bytes of 0xFF on both sides of every buffer: odd, so that inputs and outputs start at odd addresses
SMALL = cases.names(emulated=True)


def guarded(nbytes, fill=0xFF):
    return hip_emu_build.guarded(nbytes, np.uint8, GUARD, fill)


def guards_intact(buf):
    return hip_emu_build.guards_intact(buf, GUARD)


class Emulated:
    def __init__(self, lib):
        self.lib = lib

    def run(self, file_list, first_offset=1, gap=5, cap=0, fill=0x5A):
        """one call on a handle of its own -> (rc, status, [frame], chunks); frames packed from an odd offset with a gap between
        them; asserts that the guards, the gaps and the inputs are as they were"""
        data, rows, tables, out_len, outs = cases.call(file_list, first_offset, gap)
        dbuf, dview = guarded(len(data))
        dview[:] = data
        obuf, oview = guarded(out_len, fill)
        status = np.full(len(rows) + 2, -7, np.int32)
        h = P()
        assert self.lib.vsc_jpeg_decode_create(None, ctypes.byref(h)) == 0
        if cap:
            assert self.lib.vsc_jpeg_decode_scratch(h, cap, None, None) == 0
        rc = self.lib.vsc_jpeg_decode_u8(h, dview.ctypes.data, len(data), rows.ctypes.data, len(rows), tables.ctypes.data, len(tables), oview.ctypes.data,
                                         out_len, status[1:].ctypes.data)
        chunks = I64(-1)
        assert self.lib.vsc_jpeg_decode_scratch(h, 0, ctypes.byref(chunks), None) == 0
        self.lib.vsc_jpeg_decode_destroy(h)
        assert guards_intact(dbuf) and guards_intact(obuf) and status[0] == -7 and status[-1] == -7, "a guard band was written"
        assert np.array_equal(dview, data), "the input was written"
        keep = np.ones(out_len, bool)
        for at, fh, fw in outs:
            keep[at:at + fh * fw * 3] = False
        assert (oview[keep] == fill).all(), "a byte between the frames was written"
        return rc, status[1:-1], [oview[at:at + fh * fw * 3].reshape(fh, fw, 3) for at, fh, fw in outs], chunks.value


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    return Emulated(hip_emu_build.build_shared(tmp_path_factory, "jpeg_decode", hip_emu_build.source("jpeg_decode")))


@pytest.mark.parametrize("name", SMALL)
def test_emulated_kernels_equal_contract(emulated, name):
    """the whole case in one call: two launches per call, none for the empty one"""
    before = emulated.lib.emu_launches()
    rc, status, frames, chunks = emulated.run(cases.files(name))
    assert rc == 0 and (status == 0).all(), (rc, status.tolist())
    want = cases.contract(name)
    assert len(frames) == len(want)
    for i, (got, ref) in enumerate(zip(frames, want)):
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, i, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())
    assert emulated.lib.emu_launches() - before == (2 if want else 0) and chunks == (1 if want else 0)


def test_emulated_chunks(emulated):
    """five small frames under a scratch cap of 3500 bytes: (768 + 1728) + 2048 + (2304 + 1152) bytes of planes -> three chunks, six
    launches, the same bytes"""
    before = emulated.lib.emu_launches()
    rc, status, frames, chunks = emulated.run(cases.files("five_small"), cap=3500)
    assert rc == 0 and (status == 0).all() and chunks == 3 and emulated.lib.emu_launches() - before == 6
    assert all(np.array_equal(a, b) for a, b in zip(frames, cases.contract("five_small")))
    rc, _, frames, chunks = emulated.run(cases.files("five_small"), cap=1)        # every frame exceeds the cap: a chunk each
    assert rc == 0 and chunks == 5 and all(np.array_equal(a, b) for a, b in zip(frames, cases.contract("five_small")))


@pytest.mark.parametrize("name", sorted(cases.corrupt()))
def test_emulated_damaged_scan_sets_its_status_only(emulated, name):
    good = cases.files("five_small")
    rc, status, frames, _ = emulated.run([good[0], cases.corrupt()[name], good[2]])
    assert rc == 0 and status[0] == 0 and status[2] == 0 and status[1] != 0, status.tolist()
    want = cases.contract("five_small")
    assert np.array_equal(frames[0], want[0]) and np.array_equal(frames[2], want[2])


def test_emulated_statuses_name_the_fault(emulated):
    st = {k: int(emulated.run([v])[1][0]) for k, v in cases.corrupt().items()}
    assert st["scan_cut_at_a_third"] == 1 and st["deleted_rst"] == 4 and st["flipped_byte"] in (1, 2, 3, 4), st


def calls_file(path):
    """the well-formed cases and the damaged scans for tests/hip_emu/jpeg_decode_sanitize_main.cpp (format: its header)"""
    pad = lambda a: np.concatenate([np.frombuffer(a.tobytes(), np.uint8), np.zeros(-a.nbytes % 8, np.uint8)]).tobytes()     # noqa: E731
    good = cases.files("five_small")
    # (all but the 70-frame call: under the sanitizers its 70 + 78 workgroups of OS threads take as long as everything else together)
    todo = [(cases.files(n), cases.contract(n), [0] * len(cases.files(n)), 0, 0) for n in SMALL if n != "mixed70"]
    todo.append((cases.files("five_small"), cases.contract("five_small"), [0] * 5, 3500, 3))
    for v in cases.corrupt().values():
        todo.append(([good[0], v, good[2]], [cases.contract("five_small")[0], None, cases.contract("five_small")[2]], [0, 1, 0], 0, 0))
    blob = [np.int64(len(todo)).tobytes()]
    for file_list, want, expect, cap, chunks in todo:
        data, rows, tables, out_len, outs = cases.call(file_list, 1, 5)
        ref = np.zeros(out_len, np.uint8)
        for (at, fh, fw), w in zip(outs, want):
            if w is not None:
                ref[at:at + fh * fw * 3] = w.reshape(-1)
        blob.append(np.asarray([len(rows), len(data), len(tables), out_len, cap, chunks], np.int64).tobytes())
        blob += [pad(rows), np.asarray(expect, np.int64).tobytes(), pad(tables), pad(data), pad(ref)]
    with open(path, "wb") as f:
        f.write(b"".join(blob))
    return len(todo)


def test_emulated_under_the_sanitizers_as_a_child_process(tmp_path):
    exe = hip_emu_build.build_sanitized(tmp_path, hip_emu_build.source("jpeg_decode"), "jpeg_decode_sanitize_main.cpp")
    n = calls_file(str(tmp_path / "calls.bin"))
    r = subprocess.run([exe, str(tmp_path / "calls.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"ok ({n} calls" in r.stdout, r.stdout
