"""vsc_global_topk_f32 / vsc_pair_first_hits through the C ABI (vsc_hip.ops) against their numpy contract
(tests/global_topk_contract.py) -- ids as integers, scores as uint32 bit patterns, no tolerance anywhere -- then the opt-in
selection="hip" path of vsc/index.py, `--candidates hip` and the sharded form against the host path, list for list."""
import numpy as np
import pytest
import torch

import global_topk_contract as contract
from tools import synth

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def _tile():
    from vsc_hip import ops
    return ops.GLOBAL_TOPK_TILE


def _run_topk(dev, scores, ids, want, rows=None):
    from vsc_hip import ops
    got = ops.global_topk(torch.from_numpy(np.ascontiguousarray(scores, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(ids, np.int64)).to(dev),
                          want, rows=None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, np.int64)).to(dev))
    return tuple(t.cpu().numpy() for t in got)


def _check_topk(dev, scores, ids, want, rows=None):
    got = _run_topk(dev, scores, ids, want, rows)
    ref = contract.global_topk(scores, ids, want, rows=rows)
    assert len(got[0]) == len(ref[0]), (len(got[0]), len(ref[0]))
    assert np.array_equal(got[0], ref[0]), f"rows differ first at {np.flatnonzero(got[0] != ref[0])[:5]}"
    assert np.array_equal(got[1], ref[1]), f"ids differ first at {np.flatnonzero(got[1] != ref[1])[:5]}"
    assert np.array_equal(contract.bits(got[2]), contract.bits(ref[2])), "scores are not bit-identical"
    return got


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.integers(0, 1 << 40, n)


@pytest.mark.parametrize("n", [0, 1])
def test_topk_empty_and_tiny(dev, n):
    s, i = _random(n, 1)
    for want in sorted({0, 1, max(n - 1, 0), n, n + 5}):
        assert len(_check_topk(dev, s, i, want)[0]) == min(want, n)


def test_topk_sizes_at_the_tile_edge_and_across_workgroups(dev):
    """one workgroup's tile - 1 / exactly / + 1; three workgroups and a ragged tail; ~300k entries: every radix pass moves data
    between workgroups"""
    tile = _tile()
    for n in (tile - 1, tile, tile + 1, 70001, 300007):
        s, i = _random(n, n)
        for want in sorted({1, n - 1, n, n + 5, n // 3, min(n, tile + 1)}):
            _check_topk(dev, s, i, want)


def test_topk_more_survivors_than_the_sort_has_tiles_for(dev):
    """more than 4 096 x 2 048 survivors: the sort's tile grows (one workgroup ranks several rounds of its tile), the only size at
    which that path is taken; scores from a small set, so every digit pass carries long runs of equal keys across tiles"""
    n = 4096 * _tile() + 4097
    rng = np.random.default_rng(4)
    s = rng.integers(-300, 300, n).astype(np.float32)
    _check_topk(dev, s, np.arange(n), n)


def test_topk_ties_at_the_cut(dev):
    """all scores equal, want = n / 2: the cut falls inside one tie run that spans many workgroups -- the first half in input
    order; three distinct scores with the cut inside the middle run; twice the same call: identical tensors"""
    n = 300000
    ids = np.arange(n, dtype=np.int64)[::-1].copy()
    got = _check_topk(dev, np.full(n, 0.25, np.float32), ids, n // 2)
    assert np.array_equal(got[1], ids[: n // 2])
    again = _run_topk(dev, np.full(n, 0.25, np.float32), ids, n // 2)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    rng = np.random.default_rng(3)
    s = rng.choice(np.array([0.125, 0.5, 0.75], np.float32), 70001)
    want = int((s == np.float32(0.75)).sum() + (s == np.float32(0.5)).sum() // 2)
    got = _check_topk(dev, s, np.arange(70001), want)
    assert got[2][-1] == np.float32(0.5) and (s == np.float32(0.5)).sum() > want - (s == np.float32(0.75)).sum() > 0


def test_topk_signed_zeros_and_extremes(dev):
    n = 10001
    s = np.where(np.arange(n) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)     # -0, +0, -0, ...: all equal
    got = _check_topk(dev, s, np.arange(n), 4001)
    assert np.array_equal(got[1], np.arange(4001)) and np.signbit(got[2][0]) and not np.signbit(got[2][1])
    s, i = _random(n, 5)
    s[::3] = -np.abs(s[::3])
    s[7], s[11], s[5000], s[9000] = FMAX, -FMAX, FMAX, -FMAX
    for want in (1, 2, 3, n - 2, n - 1, n):
        _check_topk(dev, s, i, want)
    _check_topk(dev, -np.abs(s), i, n // 2)         # negative scores only


def test_topk_digit_coverage(dev):
    """scores that differ only in the lowest key byte / only in the highest"""
    rng = np.random.default_rng(6)
    n = 20011
    low = (np.float32(1.0).view(np.uint32) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    _check_topk(dev, low, np.arange(n), n // 2)
    high = (rng.integers(0, 255, n).astype(np.uint32) << np.uint32(24)).view(np.float32)      # exponents 0 .. 0xFD: finite, both signs
    assert np.isfinite(high).all()
    _check_topk(dev, high, np.arange(n), n // 2)
    _check_topk(dev, high, np.arange(n), n)


def test_topk_padding_and_row_arguments(dev):
    rng = np.random.default_rng(7)
    nq, k = 1300, 7
    s = rng.standard_normal((nq, k)).astype(np.float32)
    i = rng.integers(0, 5000, (nq, k))
    i[:40] = -1               # at the start
    i[-30:] = -1              # at the end
    i[600] = -1               # a whole row
    i[:, k - 1][::2] = -1     # the tail of every other row, as the search pads
    s[i < 0] = -FMAX
    valid = int((i >= 0).sum())
    for want in (1, 1000, valid - 1, valid, valid + 1, nq * k):
        got = _check_topk(dev, s, i, want)                 # rows = None: row = position // 7
        assert len(got[0]) == min(want, valid) and (got[1] >= 0).all()
        rows = np.repeat(np.arange(nq), k).reshape(nq, k)
        explicit = _run_topk(dev, s, i, want, rows=rows)
        assert all(np.array_equal(a, b) for a, b in zip(got, explicit))
    other = rng.integers(0, 99, (nq, k))                   # rows that are not position // stride
    _check_topk(dev, s, i, 2000, rows=other)
    none = _check_topk(dev, s, np.full_like(i, -1), 100)   # every entry is padding
    assert len(none[0]) == 0


# ---- pair_first_hits ---------------------------------------------------------------------------------------------------------------
def _check_pairs(dev, rows, ids, q_video, r_video, n_r_videos, limit):
    from vsc_hip import ops
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    got = ops.pair_first_hits(t(rows, np.int64), t(ids, np.int64), t(q_video, np.int32), t(r_video, np.int32), n_r_videos, limit).cpu().numpy()
    ref = contract.pair_first_hits(rows, ids, q_video, r_video, n_r_videos, limit)
    assert np.array_equal(got, ref), (len(got), len(ref))
    return got


def test_pair_first_hits_small_and_limits(dev):
    rng = np.random.default_rng(8)
    q_video, r_video = rng.integers(0, 30, 500), rng.integers(0, 40, 800)
    for n in (0, 1, 5000):
        rows, ids = rng.integers(0, 500, n), rng.integers(0, 800, n)
        count = len(contract.pair_first_hits(rows, ids, q_video, r_video, 40))
        for limit in (0, 1, count, count + 1, None):
            _check_pairs(dev, rows, ids, q_video, r_video, 40, limit)
    n = 5000
    same = _check_pairs(dev, np.full(n, 3), np.full(n, 9), q_video, r_video, 40, None)          # one pair: its first position
    assert same.tolist() == [0]
    distinct = _check_pairs(dev, np.arange(n), np.zeros(n, int), np.arange(n), np.zeros(1, int), 1, 1234)   # n_r_videos = 1, all distinct
    assert np.array_equal(distinct, np.arange(1234))
    _check_pairs(dev, rng.integers(0, 500, n), rng.integers(0, 800, n), q_video, np.zeros(800, int), 1, None)


def test_pair_first_hits_wide_keys_and_collisions(dev):
    """pair keys above 2^32 (q video 69 999 of 70 000 reference videos: tables only, no bank); ~200k hits over ~5 000 pairs:
    the table's probe sequences collide, and two runs give the same positions"""
    rng = np.random.default_rng(9)
    q_video = np.array([69999, 5, 69998, 0, 69999])
    r_video = np.array([69999, 0, 3, 69998])
    assert 69999 * 70000 + 69999 > 1 << 32
    _check_pairs(dev, rng.integers(0, 5, 4000), rng.integers(0, 4, 4000), q_video, r_video, 70000, None)
    q_video, r_video = rng.integers(0, 70, 3000), rng.integers(0, 75, 9000)
    rows, ids = rng.integers(0, 3000, 200003), rng.integers(0, 9000, 200003)
    first = _check_pairs(dev, rows, ids, q_video, r_video, 75, None)
    assert 4000 < len(first) <= 70 * 75
    assert np.array_equal(first, _check_pairs(dev, rows, ids, q_video, r_video, 75, None))
    _check_pairs(dev, rows, ids, q_video, r_video, 75, 1000)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _videos(prefix, x, frames):
    from vsc.index import VideoFeature
    return [VideoFeature(f"{prefix}{100000 + v:06d}", np.arange(float(frames)), x[v * frames:(v + 1) * frames]) for v in range(len(x) // frames)]


# (query rows, global_k, MAX_K): the three regimes of test_host_logic.py::test_global_threshold_search_host_logic -- the probe is
# sufficient; one row owns more winners than the probe holds (2 000 near-copies of a query row: with global_k = 60 the probe of
# 6 x 16 holds enough pairs but not that row's, a range sweep at the provisional threshold answers; with 6 000 it holds too few
# and the radius is found by counting); the probe is smaller than global_k -- and global_k > nq * nr
REGIMES = ((6, 30, 1024), (6, 60, 16), (6, 6000, 16), (2, 250, 64), (2, 799, 32), (2, 50000, 32))


@pytest.mark.parametrize("duplicates", [False, True])
def test_selection_hip_equals_host(dev, duplicates):
    import vsc.index as vi
    from vsc.candidates import CandidateGeneration, MaxScoreAggregation
    rng = np.random.RandomState(0)
    for nq, gk, probe in REGIMES:
        q = synth.descriptor_bank(300 + nq + gk, nq, 16)
        r = synth.descriptor_bank(400 + gk, 4000, 16)
        if probe == 16:
            r[1000:3000] = q[2] + 0.01 * rng.randn(2000, 16).astype(np.float32)
        if duplicates:
            r[7::400] = r[3]         # exact ties across reference rows (and across reference videos)
            q[-1] = q[0]             # and across query rows
        refs, queries = _videos("R", r, 40), _videos("Q", q, 2)
        old, vi.MAX_K = vi.MAX_K, probe
        try:
            lists = {}
            for selection in ("host", "hip"):
                cg = CandidateGeneration(refs, MaxScoreAggregation(), selection=selection)
                hits = cg.index._global_threshold_hits(q, gk)
                lists[selection] = (hits, cg.query(queries, gk), cg.query(queries, gk, limit=7))
        finally:
            vi.MAX_K = old
        (h_hits, h_all, h_cut), (d_hits, d_all, d_cut) = lists["host"], lists["hip"]
        assert len(h_hits[0]) == min(gk, nq * 4000)
        assert np.array_equal(h_hits[0], d_hits[0]) and np.array_equal(h_hits[1], d_hits[1]), (nq, gk, probe)
        assert np.array_equal(contract.bits(h_hits[2]), contract.bits(d_hits[2])), (nq, gk, probe)
        assert h_all == d_all and h_cut == d_cut and len(h_all) > 0, (nq, gk, probe)


def test_entry_point_candidates_hip_writes_the_same_csv(dev, tmp_path):
    import vsc.baseline.sscd_baseline as entry
    from vsc.storage import store_features
    store_features(tmp_path / "q.npz", _videos("Q", synth.descriptor_bank(21, 12 * 5, 64), 5))
    store_features(tmp_path / "r.npz", _videos("R", synth.descriptor_bank(22, 90 * 8, 64), 8))
    out = {}
    for selection in ("host", "hip"):
        args = entry.build_parser().parse_args(["--query_features", str(tmp_path / "q.npz"), "--ref_features", str(tmp_path / "r.npz"),
                                                "--output_path", str(tmp_path / selection), "--overwrite", "--candidates", selection])
        entry.main(args)
        out[selection] = (tmp_path / selection / "candidates.csv").read_bytes()
    assert out["hip"] == out["host"] and out["host"].count(b"\n") == 1 + 25 * 12


def test_sharded_global_topk_world1_equals_single_device(dev):
    """the default HIP knn and select, no process group: the list of VideoIndex(selection="hip") -- where the probe suffices, and
    where a row owns more winners than it holds (k' doubles there, the single-device path sweeps a range: the same list)"""
    import vsc.index as vi
    from vsc_hip import distributed as vdist
    rng = np.random.RandomState(1)
    q = synth.descriptor_bank(31, 9, 32)
    r = synth.descriptor_bank(32, 3000, 32)
    r[500:700] = q[4] + 0.01 * rng.randn(200, 32).astype(np.float32)
    # (bank rows, global_k): 40 -- query row 4 owns all of them, more than the probe of 16; 700 -- the probe suffices;
    # global_k > nq * nr on a bank within the largest probe (beyond MAX_K rows the sharded form refuses: see its docstring)
    for nr, gk in ((3000, 40), (3000, 700), (600, 9 * 600 + 5)):
        index = vi.VideoIndex(32, selection="hip")
        index.add(_videos("R", r[:nr], 30))
        want = index._global_threshold_hits(q, gk)
        assert len(want[0]) == min(gk, 9 * nr)
        got = vdist.sharded_global_topk(torch.from_numpy(q).to(dev), torch.from_numpy(r[:nr]).to(dev), gk)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), gk
        assert np.array_equal(contract.bits(got[2].cpu().numpy()), contract.bits(want[2])), gk
