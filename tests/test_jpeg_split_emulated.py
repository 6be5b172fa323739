"""csrc/jpeg_split.hip without a GPU: csrc/jpeg_decode.hip and csrc/jpeg_split.hip are compiled as ONE host translation unit
against tests/hip_emu/jpeg_decode.h by tests/hip_emu_build.py (one OS thread per GPU thread, barriers for __syncthreads, device
allocations as exactly sized host allocations filled with 0xFF) and vsc_jpeg_decode_split_u8 must equal the
executable contract (tests/jpeg_split_contract.py) on every case of tests/jpeg_split_cases.py: output bytes between 0xFF guard
bands at odd addresses, status 0, and the four statistics of vsc_jpeg_decode_stats.

Damaged scans run here and in the sanitizer program only, for both kinds of cut: each must give the status vsc_jpeg_decode_u8
gives for the same bytes, leave guards and gaps alone and not disturb the other frames of its call.  One case has no counterpart
in vsc_jpeg_decode_u8, which takes no marker offsets: an offset of the CSR moved by one.  The item in front of it then finds its
marker at another byte than the row says, which is VSC_JPEG_STATUS_RESTART (include/vsc_hip.h) wherever that offset is an item
boundary, and no fault where the grouping does not use it.

The same calls and the entry's refusals then run in a stand-alone program built with -fsanitize=address,undefined
(tests/hip_emu/jpeg_split_sanitize_main.cpp), started as a child process."""
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
import jpeg_split_cases as sc  # noqa: E402
import jpeg_split_contract as contract  # noqa: E402
from vsc_hip import jpeg  # noqa: E402

RESTART = 4
P, I64 = ctypes.c_void_p, ctypes.c_int64
GUARD = 13          # bytes of 0xFF on both sides of every buffer: odd, so that inputs and outputs start at odd addresses


def guarded(nbytes, fill=0xFF):
    return hip_emu_build.guarded(nbytes, np.uint8, GUARD, fill)


def guards_intact(buf):
    return hip_emu_build.guards_intact(buf, GUARD)


class Emulated:
    def __init__(self, lib):
        self.lib = lib

    def run(self, file_list, mode=3, sub_bytes=sc.SUB_BYTES, rounds=2, item_bytes=1, cap=0, restarts=None, entry="split", repeat=1, fill=0x5A):
        """``repeat`` calls on one handle of its own -> (rc, status, [frame], chunks, stats) of the last; frames packed from an
        odd offset with a gap between them; asserts that the guards, the gaps and the inputs are as they were and that every
        repeat gives the same bits"""
        data, rows, tables, out_len, outs, ptr, off = sc.call(file_list, 1, 5, restarts)
        dbuf, dview = guarded(len(data))
        dview[:] = data
        h = P()
        assert self.lib.vsc_jpeg_decode_create(None, ctypes.byref(h)) == 0
        if cap:
            assert self.lib.vsc_jpeg_decode_scratch(h, cap, None, None) == 0
        assert self.lib.vsc_jpeg_decode_split(h, mode, sub_bytes, rounds, item_bytes) == 0
        first = None
        for _ in range(repeat):
            obuf, oview = guarded(out_len, fill)
            status = np.full(len(rows) + 2, -7, np.int32)
            stats = np.full(4, -1, np.int64)
            if entry == "split":
                rc = self.lib.vsc_jpeg_decode_split_u8(h, dview.ctypes.data, len(data), rows.ctypes.data, len(rows), tables.ctypes.data, len(tables), ptr.ctypes.data,
                                                       off.ctypes.data if len(off) else None, oview.ctypes.data, out_len, status[1:].ctypes.data)
                assert self.lib.vsc_jpeg_decode_stats(h, stats.ctypes.data) == 0
            else:
                rc = self.lib.vsc_jpeg_decode_u8(h, dview.ctypes.data, len(data), rows.ctypes.data, len(rows), tables.ctypes.data, len(tables), oview.ctypes.data,
                                                 out_len, status[1:].ctypes.data)
            assert guards_intact(dbuf) and guards_intact(obuf) and status[0] == -7 and status[-1] == -7, "a guard band was written"
            assert np.array_equal(dview, data), "the input was written"
            keep = np.ones(out_len, bool)
            for at, fh, fw in outs:
                keep[at:at + fh * fw * 3] = False
            assert (oview[keep] == fill).all(), "a byte between the frames was written"
            if first is None:
                first = (oview.copy(), status.copy())
            assert np.array_equal(first[0], oview) and np.array_equal(first[1], status), "a repeated call gives other bits"
        chunks = I64(-1)
        assert self.lib.vsc_jpeg_decode_scratch(h, 0, ctypes.byref(chunks), None) == 0
        self.lib.vsc_jpeg_decode_destroy(h)
        return rc, status[1:-1], [oview[at:at + fh * fw * 3].reshape(fh, fw, 3) for at, fh, fw in outs], chunks.value, tuple(int(v) for v in stats)


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    return Emulated(hip_emu_build.build_shared(tmp_path_factory, "jpeg_split", hip_emu_build.source("jpeg_split")))


def nsub(data, sub_bytes=sc.SUB_BYTES):
    f = jpeg.parse(data)
    return -(-(f.seg_end - f.seg_start) // sub_bytes)


@pytest.mark.parametrize("item_bytes", sc.ITEM_BYTES)
@pytest.mark.parametrize("name", sorted(sc.marker()))
def test_emulated_marker_items_equal_contract(emulated, name, item_bytes):
    data = sc.marker()[name][0]
    want = contract.split(data, item_bytes=item_bytes)
    rc, status, frames, _, stats = emulated.run([data], item_bytes=item_bytes)
    assert rc == 0 and status.tolist() == [0] and np.array_equal(frames[0], sc.reference(name))
    assert want.kind == "markers" and stats == contract.stats([want]), (stats, contract.stats([want]))


@pytest.mark.parametrize("name", sorted(sc.substream()))
def test_emulated_substreams_equal_contract(emulated, name):
    """rounds = the number of sub-streams: the fixed point is reached whatever the data, so the frame is cut"""
    data = sc.substream()[name]
    rounds = nsub(data)
    want = contract.split(data, sc.SUB_BYTES, rounds)
    before = emulated.lib.emu_launches()
    rc, status, frames, _, stats = emulated.run([data], rounds=rounds)
    assert rc == 0 and status.tolist() == [0] and np.array_equal(frames[0], sc.reference(name))
    assert want.kind == "substreams" and stats == (0, 1, 0, rounds) == contract.stats([want]), (stats, contract.stats([want]))
    assert emulated.lib.emu_launches() - before == rounds + 1 + 1 + 3       # sync rounds, item table, then items, statuses, colour


def test_emulated_too_few_rounds_fall_back(emulated):
    """noise_q100[0] cut at 32 bytes: a handful of the states are right after the speculative round, so one verification round
    changes exits and the frame is decoded as one item -- to the same bytes"""
    data = cases.files("noise_q100")[0]
    want = contract.split(data, 32, 1)
    assert want.kind == "fallback" and not want.converged and want.right_after_round0 < len(want.exits[0]) // 4
    rc, status, frames, _, stats = emulated.run([data], sub_bytes=32, rounds=1)
    assert rc == 0 and status.tolist() == [0] and np.array_equal(frames[0], cases.contract("noise_q100")[0])
    assert stats == (0, 0, 1, len(want.exits[0])) == contract.stats([want])
    # and with the default two rounds at 64 bytes the frames of the table in DESIGN that need more than two fall back as well
    for name in ("noise_q75", "checker_q100[0]"):
        want = contract.split(sc.substream()[name], sc.SUB_BYTES, 2)
        rc, status, frames, _, stats = emulated.run([sc.substream()[name]], rounds=2)
        assert rc == 0 and status.tolist() == [0] and np.array_equal(frames[0], sc.reference(name)) and stats == contract.stats([want]) and want.kind == "fallback"


def test_emulated_mixed_call(emulated):
    """marker frames, sub-stream frames, a one-component frame and 1 x 1 frames in one call, in chunks under a small cap, three
    times on one handle; eight rounds are enough for every frame but checker_q100[0], which is decoded as one item"""
    files = sc.mixed()
    want = [contract.split(f, sc.SUB_BYTES, 8, 300) for f in files]
    rc, status, frames, chunks, stats = emulated.run(files, rounds=8, item_bytes=300, cap=9000, repeat=3)
    assert rc == 0 and (status == 0).all() and chunks > 2, (status.tolist(), chunks)
    assert all(np.array_equal(a, b) for a, b in zip(frames, sc.mixed_reference()))
    assert stats == contract.stats(want), (stats, contract.stats(want))
    assert stats[0] == 4 and stats[1] == 4 and stats[2] == 1


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_emulated_modes(emulated, mode):
    """a frame is cut only by what the mode names; mode 0 is one item per frame"""
    files = [sc.marker()["24x40_420_every_mcu"][0], sc.substream()["37x53_gray"]]
    want = [contract.split(f, sc.SUB_BYTES, 2, 1, mode) for f in files]
    rc, status, frames, _, stats = emulated.run(files, mode=mode, rounds=2, item_bytes=1)
    assert rc == 0 and (status == 0).all() and np.array_equal(frames[0], sc.reference("24x40_420_every_mcu")) and np.array_equal(frames[1], sc.reference("37x53_gray"))
    assert stats == contract.stats(want) == ((0, 0, 0, 2), (1, 0, 0, 7), (0, 1, 0, 14))[mode], stats


def damaged():
    """name -> (files of the call, index of the damaged frame, marker offsets override or None, RESTART expected instead of the
    one-wave status)"""
    good = cases.files("five_small")
    rst = sc.marker()["40x56_444_q90_interval_3"][0]
    f = jpeg.parse(rst)
    off = jpeg.restart_offsets(np.frombuffer(rst, np.uint8), f).tolist()
    d1 = f.seg_start + off[1]
    assert rst[d1:d1 + 2] == b"\xff\xd1"
    renumbered = rst[:d1 + 1] + b"\xd3" + rst[d1 + 2:]
    flipped = bytearray(rst)
    flipped[f.seg_start + off[1] + 2 + (off[2] - off[1] - 2) // 2] ^= 0xFF            # inside the third interval: the third item at item_bytes 1
    moved = list(off)
    moved[off.index(contract.split(rst, item_bytes=300).items[0].end_off)] += 1    # an item boundary at item_bytes 1 and at 300
    sub = sc.substream()["37x53_444"]
    g = jpeg.parse(sub)
    sub_flipped = bytearray(sub)
    sub_flipped[g.seg_start + 2 * sc.SUB_BYTES + 20] ^= 0xFF                          # inside the third sub-stream
    third = lambda data, fr: data[:fr.seg_start + (fr.seg_end - fr.seg_start) // 3]     # noqa: E731
    return {
        "deleted_rst": ([good[0], rst[:d1] + rst[d1 + 2:], good[2]], 1, None, False),
        "renumbered_rst": ([good[0], renumbered, good[2]], 1, None, False),
        "moved_offset": ([good[0], rst, good[2]], 1, {1: moved}, True),
        "flipped_byte_markers": ([good[0], bytes(flipped), good[2]], 1, None, False),
        "flipped_byte_substreams": ([good[0], bytes(sub_flipped), good[2]], 1, None, False),
        "cut_at_a_third_markers": ([good[0], third(rst, f), good[2]], 1, None, False),
        "cut_at_a_third_substreams": ([good[0], third(sub, g), good[2]], 1, None, False),
    }


@pytest.mark.parametrize("item_bytes", [1, 300])
@pytest.mark.parametrize("name", sorted(damaged()))
def test_emulated_damaged_scan_gives_the_one_wave_status(emulated, name, item_bytes):
    files, bad, restarts, lying = damaged()[name]
    rounds = max(nsub(f) for f in files)
    _, one, one_frames, _, _ = emulated.run(files, entry="u8")
    rc, status, frames, _, stats = emulated.run(files, rounds=rounds, item_bytes=item_bytes, restarts=restarts)
    assert rc == 0 and status[0] == 0 and status[2] == 0, status.tolist()
    if lying:
        assert one[bad] == 0 and status[bad] == RESTART, (one.tolist(), status.tolist())
    elif name.startswith("flipped_byte"):
        # a flipped byte may leave a scan that decodes (to other pixels): then both entries decode it, to the same bytes
        assert status[bad] == one[bad] and (one[bad] != 0 or np.array_equal(frames[bad], one_frames[bad])), (one.tolist(), status.tolist())
    else:
        assert one[bad] != 0 and status[bad] == one[bad], (one.tolist(), status.tolist())
    want = cases.contract("five_small")
    assert np.array_equal(frames[0], want[0]) and np.array_equal(frames[2], want[2])
    if name == "deleted_rst":
        assert status[bad] == RESTART and stats[2] == 1                            # the count rule: taken as unsplit


def test_emulated_moved_offset_is_harmless_where_no_item_ends_there(emulated):
    files, bad, restarts, _ = damaged()["moved_offset"]
    rc, status, frames, _, _ = emulated.run(files, item_bytes=1 << 30, restarts=restarts)
    assert rc == 0 and (status == 0).all() and np.array_equal(frames[bad], sc.reference("40x56_444_q90_interval_3"))


def calls_file(path):
    """well-formed and damaged calls for tests/hip_emu/jpeg_split_sanitize_main.cpp (format: its header)"""
    pad = lambda a: np.concatenate([np.frombuffer(a.tobytes(), np.uint8), np.zeros(-a.nbytes % 8, np.uint8)]).tobytes()     # noqa: E731
    todo = []      # (files, references or None per frame, expect per frame, cap, mode, sub_bytes, rounds, item_bytes, restarts)
    for name, item_bytes in (("24x40_420_every_mcu", 1), ("40x56_444_q90_interval_3", 300), ("40x56_gray_interval_2", 1), ("noise_q100_every_mcu", 300), ("1x1_interval_1", 1)):
        todo.append(([sc.marker()[name][0]], [sc.reference(name)], [0], 0, 3, sc.SUB_BYTES, 1, item_bytes, None))
    # (as many rounds as each frame needs, not as many as it has sub-streams: under the sanitizers every workgroup of OS threads costs)
    for name, rounds in (("37x53_420", 4), ("shorter_than_a_substream", 1)):
        data = sc.substream()[name]
        assert contract.split(data, sc.SUB_BYTES, rounds).kind == "substreams" and contract.split(data, sc.SUB_BYTES, rounds - 1 or 1).kind in ("fallback", "substreams")
        todo.append(([data], [sc.reference(name)], [0], 0, 3, sc.SUB_BYTES, rounds, 1, None))
    todo.append(([cases.files("noise_q100")[0]], [cases.contract("noise_q100")[0]], [0], 0, 3, 32, 1, 1, None))
    mixed = ("40x56_420_interval_5", "37x53_gray", "1x1_interval_1", "shorter_than_a_substream", "40x56_gray_interval_2")      # chunked under a small cap
    todo.append(([sc.all_files()[n] for n in mixed], [sc.reference(n) for n in mixed], [0] * len(mixed), 6000, 3, sc.SUB_BYTES, 2, 300, None))
    five = cases.contract("five_small")
    for name, (fl, bad, restarts, lying) in damaged().items():
        todo.append((fl, [five[0], None, five[2]], [0, 2 if lying else 3 if name.startswith("flipped_byte") else 1, 0], 0, 3, sc.SUB_BYTES, 2 if name.endswith("substreams") else 1, 1, restarts))
    blob = [np.int64(len(todo)).tobytes()]
    for fl, want, expect, cap, mode, sub_bytes, rounds, item_bytes, restarts in todo:
        data, rows, tables, out_len, outs, ptr, off = sc.call(fl, 1, 5, restarts)
        splits = [contract.split(f, sub_bytes, rounds, item_bytes, mode, None if not restarts or i not in restarts else restarts[i]) for i, f in enumerate(fl)]
        ref = np.zeros(out_len, np.uint8)
        for (at, fh, fw), w in zip(outs, want):
            if w is not None:
                ref[at:at + fh * fw * 3] = w.reshape(-1)
        blob.append(np.asarray([len(rows), len(data), len(tables), out_len, cap, mode, sub_bytes, rounds, item_bytes, len(off), *contract.stats(splits)], np.int64).tobytes())
        blob += [pad(rows), np.asarray(expect, np.int64).tobytes(), ptr.tobytes(), pad(off), pad(tables), pad(data), pad(ref)]
    with open(path, "wb") as f:
        f.write(b"".join(blob))
    return len(todo)


def test_emulated_under_the_sanitizers_as_a_child_process(tmp_path):
    exe = hip_emu_build.build_sanitized(tmp_path, hip_emu_build.source("jpeg_split"), "jpeg_split_sanitize_main.cpp")
    n = calls_file(str(tmp_path / "calls.bin"))
    r = subprocess.run([exe, str(tmp_path / "calls.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"ok ({n} calls" in r.stdout, r.stdout
