"""The global top-k selection without a GPU: the numpy contract (tests/global_topk_contract.py) against what the host path of
vsc/index.py produces today, the opt-in plumbing (`--candidates`, `selection=`), and the sharded form under gloo with the oracle
and the contract standing in for the HIP entries through the documented hooks.  The kernels themselves: tests/test_gpu_global_topk.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import global_topk_contract as contract
from vsc_hip import distributed as vdist


class _NumpySweep:
    """vsc_hip.ops on CPU tensors: the sweeps are the oracle's chains, the two selection entries are the contract."""

    @staticmethod
    def knn_ip(q, r, k, ref_id_offset=0, floor=None):
        from oracle import knn_oracle
        if q.shape[0] == 0:
            return torch.empty((0, k)), torch.empty((0, k), dtype=torch.int64)
        D, I = knn_oracle.knn_ip(q.numpy(), r.numpy(), k)
        return torch.from_numpy(D), torch.from_numpy(I + ref_id_offset * (I >= 0))

    @staticmethod
    def range_search_ip(q, r, radius, ref_id_offset=0, capacity=0):
        from oracle import knn_oracle
        lims, D, I = knn_oracle.range_search_ip(q.numpy(), r.numpy(), float(radius))
        return torch.from_numpy(lims), torch.from_numpy(D), torch.from_numpy(I)

    @staticmethod
    def range_count_ip(q, r, radius):
        from oracle import knn_oracle
        return int(knn_oracle.range_search_ip(q.numpy(), r.numpy(), float(radius))[0][-1])

    @staticmethod
    def global_topk(scores, ids, want, rows=None):
        out = contract.global_topk(scores.numpy(), ids.numpy(), want, rows=None if rows is None else rows.numpy())
        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in out)

    @staticmethod
    def pair_first_hits(rows, ids, q_video, r_video, n_r_videos, limit=None):
        return torch.from_numpy(contract.pair_first_hits(rows.numpy(), ids.numpy(), q_video.numpy(), r_video.numpy(), n_r_videos, limit))


@pytest.fixture
def cpu_sweep(monkeypatch):
    import vsc.index as vi
    from vsc_hip import ops
    monkeypatch.setattr(vi.FlatIPBank, "_to_device", staticmethod(lambda host: torch.from_numpy(np.ascontiguousarray(host))))
    for name in ("knn_ip", "range_search_ip", "range_count_ip", "global_topk", "pair_first_hits"):
        monkeypatch.setattr(ops, name, getattr(_NumpySweep, name))
    return vi


def _banks(rng, nq_videos, q_frames, n_r_videos, r_frames, d=16):
    def unit(n):
        x = rng.randn(n, d).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    return unit(nq_videos * q_frames), unit(n_r_videos * r_frames)


def _videos(vi, prefix, x, frames):
    return [vi.VideoFeature(f"{prefix}{v:03d}", np.arange(float(frames)), x[v * frames:(v + 1) * frames]) for v in range(len(x) // frames)]


# (query videos, global_k, MAX_K): the probe is sufficient / one row owns more winners than the probe holds (60: the probe holds
# enough pairs, a range sweep at the provisional threshold; 300: it holds too few, radius found by counting) / the probe is
# smaller than global_k / global_k beyond nq * nr -- the regimes of test_host_logic.py::test_global_threshold_search_host_logic
REGIMES = ((3, 30, 1024), (3, 60, 16), (3, 300, 16), (1, 250, 64), (1, 799, 32), (1, 5000, 32))


@pytest.mark.parametrize("duplicates", [False, True])
def test_contract_is_what_the_host_path_produces(cpu_sweep, duplicates):
    """contract.global_topk over the FULL score matrix == VideoIndex._global_threshold_hits (rows, refs, score bits, order), and
    contract.pair_first_hits over that list == search_pair_maxima, in every regime; and the selection="hip" plumbing -- with
    the contract behind ops.global_topk / ops.pair_first_hits -- returns the same lists as selection="host"."""
    vi = cpu_sweep
    from oracle import knn_oracle
    rng = np.random.RandomState(0)
    for nqv, gk, probe in REGIMES:
        q, r = _banks(rng, nqv, 2, 20, 20)
        if probe == 16:
            r[50:200] = q[2] + 0.01 * rng.randn(150, 16).astype(np.float32)
        if duplicates:
            r[7::40] = r[3]          # the same reference row in several videos: exact ties across ids
            q[-1] = q[0]             # and the same query row twice: exact ties across rows
        refs, queries = _videos(vi, "R", r, 20), _videos(vi, "Q", q, 2)
        host, hip = vi.VideoIndex(16), vi.VideoIndex(16, selection="hip")
        host.add(refs)
        hip.add(refs)
        S = knn_oracle.ip_matrix(q, r)
        ids = np.broadcast_to(np.arange(S.shape[1]), S.shape)
        want_rows, want_ids, want_scores = contract.global_topk(S, ids, gk)
        old, vi.MAX_K = vi.MAX_K, probe
        try:
            got = host._global_threshold_hits(q, gk)
            got_hip = hip._global_threshold_hits(q, gk)
            pairs = [host.search_pair_maxima(queries, gk, limit) for limit in (None, 5)]
            pairs_hip = [hip.search_pair_maxima(queries, gk, limit) for limit in (None, 5)]
        finally:
            vi.MAX_K = old
        assert len(want_rows) == min(gk, S.size)
        for g in (got, got_hip):
            assert np.array_equal(g[0], want_rows) and np.array_equal(g[1], want_ids)
            assert np.array_equal(contract.bits(g[2]), contract.bits(want_scores))
        r_names, r_of_row = np.unique(np.repeat([v.video_id for v in refs], 20), return_inverse=True)
        q_of_row = np.repeat(np.arange(len(queries)), 2)
        for limit, p, ph in zip((None, 5), pairs, pairs_hip):
            first = contract.pair_first_hits(want_rows, want_ids, q_of_row, r_of_row, len(r_names), limit)
            assert p[0] == [queries[i].video_id for i in q_of_row[want_rows[first]]]
            assert p[1] == r_names[r_of_row[want_ids[first]]].tolist()
            assert p[2] == want_scores[first].tolist()
            assert ph == p


def test_candidates_option_and_selection_argument(cpu_sweep):
    vi = cpu_sweep
    from vsc.baseline import sscd_baseline
    from vsc.candidates import CandidateGeneration, MaxScoreAggregation
    base = ["--query_features", "q.npz", "--ref_features", "r.npz", "--output_path", "out"]
    assert sscd_baseline.build_parser().parse_args(base).candidates == "host"
    assert sscd_baseline.build_parser().parse_args(base + ["--candidates", "hip"]).candidates == "hip"
    with pytest.raises(SystemExit):
        sscd_baseline.build_parser().parse_args(base + ["--candidates", "faiss"])
    with pytest.raises(ValueError, match="METRIC_L2"):
        vi.VideoIndex(16, "Flat", vi.METRIC_L2, selection="hip")
    with pytest.raises(ValueError, match="selection"):
        vi.VideoIndex(16, selection="device")
    assert vi.VideoIndex(16).selection == "host"
    rng = np.random.RandomState(1)
    q, r = _banks(rng, 4, 3, 6, 10)
    refs, queries = _videos(vi, "R", r, 10), _videos(vi, "Q", q, 3)
    lists = [CandidateGeneration(refs, MaxScoreAggregation(), selection=s).query(queries, global_k=40, limit=7) for s in ("host", "hip")]
    assert lists[0] == lists[1] and len(lists[0]) == 7
    assert sscd_baseline.search(queries, refs, 10.0, 2.0, selection="hip") == sscd_baseline.search(queries, refs, 10.0, 2.0)


# ---- sharded form under gloo ------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sharded_problem(copies=True):
    """7 query rows, 120 reference rows, d = 16.  Rows 1 and 5 are the same query (they land on different ranks: equal scores
    whose order is the row order across two ranks' lists), reference rows 10 / 70 / 119 are the same row (ties across reference
    shards), and 50 references are near-copies of query row 0, so that row owns most of the 60 best pairs: more than the first
    probe of 32 holds, which forces one doubling of k'."""
    rng = np.random.RandomState(5)
    q = rng.randn(7, 16).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r = rng.randn(120, 16).astype(np.float32)
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    q[5] = q[1]
    if copies:
        r[20:70] = q[0] + 0.01 * rng.randn(50, 16).astype(np.float32)
    r[70] = r[119] = r[10]
    return q, r


# uneven shards; at world 3 the middle rank holds no queries; query rows 1 and 5 always sit on different ranks
Q_CUTS = {2: [0, 4, 7], 3: [0, 3, 3, 7]}
R_CUTS = {2: [0, 75, 120], 3: [0, 15, 100, 120]}


def _sharded_worker(rank, world_size, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        from oracle import knn_oracle
        probes = []

        def knn(qq, rr, k, **kw):
            probes.append(k)
            return _NumpySweep.knn_ip(qq, rr, k, **kw)

        q_cuts, r_cuts = Q_CUTS[world_size], R_CUTS[world_size]
        # (near-copies, global_k, the probe sizes expected): without the copies one probe of 16 holds the 20 best; with them query
        # row 0 owns more than the probe holds, so k' doubles once (16 -> min(32, 20); 32 -> min(64, 60)); 5000 > nq * nr: the
        # probe is the whole bank at once
        for copies, gk, expect_probes in ((False, 20, [16]), (True, 20, [16, 20]), (True, 60, [32, 60]), (True, 5000, [120])):
            q, r = _sharded_problem(copies)
            S = knn_oracle.ip_matrix(q, r)
            ids = np.broadcast_to(np.arange(120), S.shape)
            q_mine = torch.from_numpy(q[q_cuts[rank]:q_cuts[rank + 1]])
            r_mine = torch.from_numpy(r[r_cuts[rank]:r_cuts[rank + 1]])
            del probes[:]
            got = vdist.sharded_global_topk(q_mine, r_mine, gk, knn=knn, select=_NumpySweep.global_topk)
            want = contract.global_topk(S, ids, gk)
            assert len(want[0]) == min(gk, S.size)
            assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), (rank, gk)
            assert np.array_equal(contract.bits(got[2].numpy()), contract.bits(want[2])), (rank, gk)
            assert probes == expect_probes, (rank, copies, gk, probes)
        # (the last list holds every pair: the tie between query rows 1 and 5 -- two ranks' lists -- came out in row order)
        hits = list(zip(got[0].tolist(), got[1].tolist()))
        assert S[1, 33] == S[5, 33] and hits.index((1, 33)) < hits.index((5, 33))
        # a row that owns more winners than the largest probe holds: refused, naming the single-device path
        old, vdist.MAX_K = vdist.MAX_K, 32
        try:
            with pytest.raises(NotImplementedError, match="single-device"):
                vdist.sharded_global_topk(q_mine, r_mine, 60, knn=knn, select=_NumpySweep.global_topk)
        finally:
            vdist.MAX_K = old
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world_size", [2, 3])
def test_sharded_global_topk_equals_the_contract_on_every_rank(world_size):
    mp.spawn(_sharded_worker, args=(world_size, _free_port()), nprocs=world_size, join=True)


def test_sharded_global_topk_single_process():
    """no process group: the local selection is the global one"""
    from oracle import knn_oracle
    q, r = _sharded_problem()
    S = knn_oracle.ip_matrix(q, r)
    got = vdist.sharded_global_topk(torch.from_numpy(q), torch.from_numpy(r), 60, knn=_NumpySweep.knn_ip, select=_NumpySweep.global_topk)
    want = contract.global_topk(S, np.broadcast_to(np.arange(120), S.shape), 60)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got[:2], want[:2]))
    assert np.array_equal(contract.bits(got[2].numpy()), contract.bits(want[2]))
    none = vdist.sharded_global_topk(torch.from_numpy(q[:0]), torch.from_numpy(r), 60, knn=_NumpySweep.knn_ip, select=_NumpySweep.global_topk)
    assert [t.numel() for t in none] == [0, 0, 0]
