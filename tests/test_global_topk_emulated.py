"""csrc/global_topk.hip (and with it the scans and the radix sort of csrc/scan_sort.h on 32-bit keys) without a GPU: the kernel
source is compiled as host C++ against tests/hip_emu/common.h by tests/hip_emu_build.py (one OS thread per GPU thread, barriers for
__syncthreads and the wave intrinsics, real atomics under real races, one scratch buffer per slot, filled with 0xFF when fresh) and
must equal the executable contract (tests/global_topk_contract.py) exactly, scores as uint32 bit patterns: the radix select, the
stable compaction, the sort over one, two and three tiles and over a grown tile, the gather, the pair table, the refusals.  No case
above 5 000 entries; the GPU suite (tests/test_gpu_global_topk.py) checks the same, and the large cases, on the device.  The same
entries then run in a stand-alone program built with -fsanitize=address,undefined (tests/hip_emu/global_topk_sanitize_main.cpp),
started as a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import global_topk_contract as C  # noqa: E402
import hip_emu_build  # noqa: E402
from hip_emu_build import guarded, guards_intact  # noqa: E402     (guards of 8 elements of 0xFF bytes; as floats NaN)

FMAX = np.finfo(np.float32).max
UNTOUCHED32, UNTOUCHED64 = np.uint32(0xFFFFFFFF), np.int64(-1)


class Emulated:
    def __init__(self, lib):
        self.lib = lib

    def topk(self, scores, ids, want, rows=None, row_stride=1):
        """-> (rc, count, rows, ids, scores); the outputs hold min(want, n) elements, as the entry asks, and start as 0xFF bytes"""
        scores, ids = np.ascontiguousarray(scores, np.float32).reshape(-1), np.ascontiguousarray(ids, np.int64).reshape(-1)
        rows = None if rows is None else np.ascontiguousarray(rows, np.int64).reshape(-1)
        n, cap = len(scores), min(max(want, 0), len(scores))
        bufs = [guarded(cap, np.int64), guarded(cap, np.int64), guarded(cap, np.float32), guarded(1, np.int64)]
        rc = self.lib.vsc_global_topk_f32(scores.ctypes.data, None if rows is None else rows.ctypes.data, ids.ctypes.data, n, row_stride, want,
                                          *(v.ctypes.data for _, v in bufs), None)
        assert all(guards_intact(b) for b, _ in bufs)
        return rc, int(bufs[3][1][0]), bufs[0][1], bufs[1][1], bufs[2][1]

    def check_topk(self, scores, ids, want, rows=None, row_stride=1):
        """the call equals the contract; the count is read from the device word; nothing is written beyond it"""
        rc, count, r, i, s = self.topk(scores, ids, want, rows, row_stride)
        ref = C.global_topk(scores, ids, want, rows=rows, row_stride=row_stride)
        assert rc == 0 and count == len(ref[0]), (rc, count, len(ref[0]))
        assert np.array_equal(r[:count], ref[0]), f"rows differ first at {np.flatnonzero(r[:count] != ref[0])[:5]}"
        assert np.array_equal(i[:count], ref[1]), f"ids differ first at {np.flatnonzero(i[:count] != ref[1])[:5]}"
        assert np.array_equal(C.bits(s[:count]), C.bits(ref[2])), "scores are not bit-identical"
        assert (r[count:] == UNTOUCHED64).all() and (i[count:] == UNTOUCHED64).all() and (s[count:].view(np.uint32) == UNTOUCHED32).all()
        return r[:count], i[:count], s[:count]

    def pairs(self, rows, ids, q_video, r_video, n_r_videos, limit):
        rows, ids = np.ascontiguousarray(rows, np.int64), np.ascontiguousarray(ids, np.int64)
        q_video, r_video = np.ascontiguousarray(q_video, np.int32), np.ascontiguousarray(r_video, np.int32)
        n = len(rows)
        cap = n if limit < 0 else min(n, limit)
        pos, cnt = guarded(cap, np.int64), guarded(1, np.int64)
        rc = self.lib.vsc_pair_first_hits(rows.ctypes.data, ids.ctypes.data, n, q_video.ctypes.data, r_video.ctypes.data, n_r_videos, limit,
                                          pos[1].ctypes.data, cnt[1].ctypes.data, None)
        assert guards_intact(pos[0]) and guards_intact(cnt[0])
        return rc, int(cnt[1][0]), pos[1]

    def check_pairs(self, rows, ids, q_video, r_video, n_r_videos, limit):
        rc, count, pos = self.pairs(rows, ids, q_video, r_video, n_r_videos, limit)
        ref = C.pair_first_hits(rows, ids, q_video, r_video, n_r_videos, limit)
        assert rc == 0 and count == len(ref), (rc, count, len(ref))
        assert np.array_equal(pos[:count], ref) and (pos[count:] == UNTOUCHED64).all()
        return pos[:count]


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    return Emulated(hip_emu_build.build_shared(tmp_path_factory, "global_topk", hip_emu_build.source("global_topk")))


def random(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.integers(0, 1 << 40, n)


# ---- vsc_global_topk_f32: sizes and tiles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_emulated_topk_sizes(emulated, n):
    """a wave, a workgroup and a tile, each - 1 / exactly / + 1, and two tiles + 1; every want from nothing to more than there is"""
    s, i = random(n, n)
    for want in sorted({0, 1, n // 3, n - 1, n, n + 5}):
        assert len(emulated.check_topk(s, i, want)[0]) == min(want, n)


def test_emulated_topk_survivors_span_three_sort_tiles(emulated):
    s, i = random(4500, 11)
    emulated.check_topk(s, i, 4400)


# ---- vsc_global_topk_f32: key content ----------------------------------------------------------------------------------------------
def test_emulated_topk_ties_at_the_cut(emulated):
    """all scores equal, want = n / 2: the cut falls inside one tie run that spans the workgroups -- the first half in input order;
    three distinct scores with the cut inside the middle run"""
    n = 4500
    ids = np.arange(n, dtype=np.int64)[::-1].copy()
    got = emulated.check_topk(np.full(n, 0.25, np.float32), ids, n // 2)
    assert np.array_equal(got[1], ids[: n // 2])
    s = np.random.default_rng(3).choice(np.array([0.125, 0.5, 0.75], np.float32), 2500)
    top, mid = int((s == np.float32(0.75)).sum()), int((s == np.float32(0.5)).sum())
    got = emulated.check_topk(s, np.arange(2500), top + mid // 2)
    assert got[2][-1] == np.float32(0.5) and mid > mid // 2 > 0


def test_emulated_topk_signed_zeros_and_extremes(emulated):
    n = 2500
    s = np.where(np.arange(n) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)     # -0, +0, -0, ...: all equal
    got = emulated.check_topk(s, np.arange(n), 1001)
    assert np.array_equal(got[1], np.arange(1001)) and np.signbit(got[2][0]) and not np.signbit(got[2][1])
    s, i = random(n, 5)
    s[::3] = -np.abs(s[::3])
    s[7], s[11], s[1200], s[2400] = FMAX, -FMAX, FMAX, -FMAX
    for want in (2, 3, n - 1, n):
        emulated.check_topk(s, i, want)
    emulated.check_topk(-np.abs(s), i, n // 2)         # negative scores only


def test_emulated_topk_digit_coverage(emulated):
    """scores that differ only in the lowest key byte / only in the highest"""
    rng = np.random.default_rng(6)
    n = 2500
    low = (np.float32(1.0).view(np.uint32) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    emulated.check_topk(low, np.arange(n), n // 2)
    high = (rng.integers(0, 255, n).astype(np.uint32) << np.uint32(24)).view(np.float32)      # exponents 0 .. 0xFD: finite, both signs
    assert np.isfinite(high).all()
    emulated.check_topk(high, np.arange(n), n // 2)
    emulated.check_topk(high, np.arange(n), n)


# ---- vsc_global_topk_f32: padding and rows -----------------------------------------------------------------------------------------
def test_emulated_topk_padding_and_row_arguments(emulated):
    rng = np.random.default_rng(7)
    nq, k = 330, 7
    s = rng.standard_normal((nq, k)).astype(np.float32)
    i = rng.integers(0, 5000, (nq, k))
    i[:40] = -1               # at the start
    i[-30:] = -1              # at the end
    i[150] = -1               # a whole row
    i[:, k - 1][::2] = -1     # the tail of every other row, as the search pads
    s[i < 0] = -FMAX
    valid = int((i >= 0).sum())
    rows = np.repeat(np.arange(nq), k)
    for want in (1, valid - 1, valid, valid + 1, nq * k):
        got = emulated.check_topk(s, i, want, row_stride=k)          # rows = NULL: row = position // 7
        assert len(got[0]) == min(want, valid) and (got[1] >= 0).all()
        explicit = emulated.check_topk(s, i, want, rows=rows, row_stride=0)
        assert all(np.array_equal(a, b) for a, b in zip(got, explicit))
    emulated.check_topk(s, i, 700, rows=rng.integers(0, 99, nq * k), row_stride=3)      # rows that are not position // stride: they win
    rc, count, r, ids, sc = emulated.topk(s, np.full_like(i, -1), 100, row_stride=k)     # every entry is padding
    assert rc == 0 and count == 0
    assert (r == UNTOUCHED64).all() and (ids == UNTOUCHED64).all() and (sc.view(np.uint32) == UNTOUCHED32).all()


# ---- vsc_pair_first_hits -----------------------------------------------------------------------------------------------------------
def test_emulated_pair_first_hits_sizes_and_limits(emulated):
    rng = np.random.default_rng(8)
    q_video, r_video = rng.integers(0, 30, 500), rng.integers(0, 40, 800)
    for n in (0, 1, 3000):
        rows, ids = rng.integers(0, 500, n), rng.integers(0, 800, n)
        count = len(C.pair_first_hits(rows, ids, q_video, r_video, 40))
        for limit in (0, 1, count, count + 1, -1):
            emulated.check_pairs(rows, ids, q_video, r_video, 40, limit)
    n = 3000
    assert emulated.check_pairs(np.full(n, 3), np.full(n, 9), q_video, r_video, 40, -1).tolist() == [0]          # one single pair
    distinct = emulated.check_pairs(np.arange(n), np.zeros(n, int), np.arange(n), np.zeros(1, int), 1, 1234)     # all pairs distinct
    assert np.array_equal(distinct, np.arange(1234))


def test_emulated_pair_first_hits_wide_keys_and_long_probe_runs(emulated):
    """pair keys above 2^32; 3 000 hits over about 40 pairs: the lanes race for few table slots, and two calls give the same positions"""
    rng = np.random.default_rng(9)
    q_video, r_video = np.array([69999, 5, 69998, 0, 69999]), np.array([69999, 0, 3, 69998])
    assert 69999 * 70000 + 69999 > 1 << 32
    emulated.check_pairs(rng.integers(0, 5, 1000), rng.integers(0, 4, 1000), q_video, r_video, 70000, -1)
    q_video, r_video = rng.integers(0, 5, 300), rng.integers(0, 8, 900)
    rows, ids = rng.integers(0, 300, 3000), rng.integers(0, 900, 3000)
    first = emulated.check_pairs(rows, ids, q_video, r_video, 8, -1)
    assert 30 <= len(first) <= 40
    assert np.array_equal(first, emulated.check_pairs(rows, ids, q_video, r_video, 8, -1))


# ---- refusals, scratch -------------------------------------------------------------------------------------------------------------
def test_emulated_refusals_and_empty_calls_launch_nothing(emulated):
    lib = emulated.lib
    s, i, v = np.ones(4, np.float32), np.arange(4, dtype=np.int64), np.zeros(4, np.int32)
    out, of, cnt = np.zeros(8, np.int64), np.zeros(8, np.float32), np.full(1, -1, np.int64)
    a = lambda x: x.ctypes.data     # noqa: E731
    topk = lambda n, stride, want, *p: lib.vsc_global_topk_f32(a(s), None, a(i), n, stride, want, *p, None)     # noqa: E731
    good = (a(out), a(out), a(of), a(cnt))
    before = lib.emu_launches()
    assert topk(-1, 1, 2, *good) != 0 and topk(1 << 31, 1, 2, *good) != 0 and topk(4, 1, -1, *good) != 0
    assert topk(4, 1, 2, None, *good[1:]) != 0 and topk(4, 1, 2, *good[:3], None) != 0
    assert lib.vsc_global_topk_f32(None, None, a(i), 4, 1, 2, *good, None) != 0
    assert topk(4, 0, 2, *good) != 0                                                   # row_stride = 0 without rows
    pairs = lambda n, nrv, limit, *p: lib.vsc_pair_first_hits(a(i), a(i), n, a(v), a(v), nrv, limit, *p, None)     # noqa: E731
    assert pairs(-1, 1, -1, a(out), a(cnt)) != 0 and pairs(1 << 31, 1, -1, a(out), a(cnt)) != 0
    assert pairs(4, 0, -1, a(out), a(cnt)) != 0                                        # n_r_videos = 0
    assert pairs(4, 1, -1, None, a(cnt)) != 0 and pairs(4, 1, -1, a(out), None) != 0
    assert lib.vsc_pair_first_hits(None, a(i), 4, a(v), a(v), 1, -1, a(out), a(cnt), None) != 0
    for call in (lambda: topk(0, 1, 2, None, None, None, a(cnt)), lambda: topk(4, 1, 0, None, None, None, a(cnt)),
                 lambda: pairs(0, 1, -1, None, a(cnt)), lambda: pairs(4, 1, 0, None, a(cnt))):      # empty: count 0, nothing read
        cnt[0] = -1
        assert call() == 0 and cnt[0] == 0
    assert lib.emu_launches() == before
    emulated.check_topk(*random(300, 2), 100)                                          # and the entries still work


def test_emulated_scratch_is_reused_across_sizes(emulated):
    """a larger call, then smaller ones back to back on the same grow-only slots: a smaller call finds the larger call's leftovers
    in every buffer and must not read them; the slots do not grow"""
    rng = np.random.default_rng(12)
    q_video, r_video = rng.integers(0, 30, 500), rng.integers(0, 40, 800)
    emulated.check_topk(*random(4500, 13), 4500)
    emulated.check_pairs(rng.integers(0, 500, 4500), rng.integers(0, 800, 4500), q_video, r_video, 40, -1)
    before = emulated.lib.emu_scratch_allocs()
    for n, want in ((257, 100), (9, 9), (2049, 2049), (128, 1), (1000, 999), (1, 1), (2500, 700), (7, 20)):
        emulated.check_topk(*random(n, n + 1), want)
        emulated.check_pairs(rng.integers(0, 500, n), rng.integers(0, 800, n), q_video, r_video, 40, -1)
    assert emulated.lib.emu_scratch_allocs() == before, "a call no larger than an earlier one grew the scratch"


# ---- the grown tile ----------------------------------------------------------------------------------------------------------------
def test_emulated_topk_grown_sort_tile(emulated, tmp_path_factory):
    """built with VSC_SORT_MAX_TILES = 2: 5 000 survivors take a tile of 2 560 -- two tiles, ten rounds each, a ragged last one --;
    scores from a set of 40 values, so every pass carries runs of equal keys across the tiles"""
    grown = Emulated(hip_emu_build.build_shared(tmp_path_factory, "global_topk_grown", hip_emu_build.source("global_topk"), ["-DVSC_SORT_MAX_TILES=2"]))
    n = 5000
    s = np.random.default_rng(4).integers(-20, 20, n).astype(np.float32)
    blocks = []
    for emu in (emulated, grown):
        before = emu.lib.emu_blocks()
        emu.check_topk(s, np.arange(n), n)
        blocks.append(emu.lib.emu_blocks() - before)
    assert blocks[0] - blocks[1] == 4 * 2 * (3 - 2), blocks      # 4 passes x (histogram, scatter) x one tile fewer than the three of 2 048


# ---- under the sanitizers ----------------------------------------------------------------------------------------------------------
def test_emulated_under_the_sanitizers_as_a_child_process(tmp_path):
    exe = hip_emu_build.build_sanitized(tmp_path, hip_emu_build.source("global_topk"), "global_topk_sanitize_main.cpp")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "under the sanitizers: ok" in r.stdout, r.stdout
