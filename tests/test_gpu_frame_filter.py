"""The near-duplicate frame filter on the device (csrc/frame_filter.hip, ops.frame_filter, ``frame_filter="hip"``,
``extract_query_feats.py --frame_filter hip``): the entry through ctypes against the executable contract
(tests/frame_filter_contract.py) on every case of tests/frame_filter_cases.py -- the ones of 1 088, 1 089 and 1 100 rows included,
the two sides of the size at which the adjacency bits leave LDS for the scratch -- between 0xFF guard bands; select_frames,
process_query_group and run_query_videos with ``frame_filter="hip"`` against the default path, bit for bit, on tie-free inputs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_filter_cases as cases  # noqa: E402
import frame_filter_contract as C  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512                     # bytes of 0xFF on both sides of every output: -1 as int32, NaN as float32
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wants():
    """the contract's (kept, mean, order) of every case, computed once"""
    return {name: C.keep(cases.get(name)["s"], cases.get(name)["thr"]) for name in cases.names()}


def guarded(nbytes, dev):
    whole = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + nbytes]


def run_entry(flat_dev, items, thr, dev, optional=True, check=True):
    """one vsc_frame_filter_f32 call with guarded outputs on the null stream -> (rc, {name: host bytes of the body}, guards intact)"""
    from vsc_hip import _lib
    lib = _lib.load()
    items = np.ascontiguousarray(items, np.int64).reshape(-1, 2)
    n, total = len(items), int(items[:, 1].clip(min=0).sum()) if len(items) else 0
    out = {k: guarded(b, dev) for k, b in (("kept", 4 * total), ("counts", 4 * n), ("means", 4 * total), ("order", 4 * total))}
    p = {k: P(body.data_ptr()) for k, (_, body) in out.items()}
    if not optional:
        p["means"] = p["order"] = None
    h = P()
    _lib.check(lib.vsc_frame_filter_create(None, ctypes.byref(h)))
    try:
        rc = lib.vsc_frame_filter_f32(h, P(flat_dev.data_ptr()) if flat_dev.numel() else None, flat_dev.numel(), items.ctypes.data, n,
                                      float(thr), p["kept"], p["counts"], p["means"], p["order"])
    finally:
        lib.vsc_frame_filter_destroy(h)              # host state only: what is enqueued does not refer to it
    torch.cuda.synchronize()
    if check:
        assert rc == 0, _lib.load().vsc_last_error()
    intact = True
    for whole, _ in out.values():
        w = whole.cpu().numpy()
        intact = intact and bool((w[:GUARD] == 0xFF).all() and (w[len(w) - GUARD:] == 0xFF).all())
    return rc, {k: body.cpu().numpy() for k, (_, body) in out.items()}, intact


def assert_items(host, mats, want_list, names, with_optional=True):
    kept, counts = host["kept"].view(np.int32), host["counts"].view(np.int32)
    means, order = host["means"].view(np.uint32), host["order"].view(np.int32)
    at = 0
    for k, (s, (w_kept, w_mean, w_order), name) in enumerate(zip(mats, want_list, names)):
        L = len(s)
        print(f"{name}: rows {L} kept {int(counts[k])} contract {len(w_kept)}")
        assert counts[k] == len(w_kept), (name, int(counts[k]), len(w_kept))
        assert kept[at:at + counts[k]].tolist() == w_kept.tolist(), (name, "kept rows")
        assert (kept[at + counts[k]:at + L] == -1).all(), (name, "the tail is not -1")
        if with_optional:
            assert np.array_equal(means[at:at + L], C.bits(w_mean)), (name, "mean bits", np.nonzero(means[at:at + L] != C.bits(w_mean))[0][:8])
            assert order[at:at + L].tolist() == w_order.tolist(), (name, "visit order")
        at += L
    assert at == len(kept)


@pytest.mark.parametrize("name", cases.names())
def test_entry_equals_the_contract_between_guard_bands(dev, wants, name):
    """kept, counts, mean bits and visit order; without the optional outputs the same kept rows; three calls, the same bytes"""
    case = cases.get(name)
    s, L = case["s"], len(case["s"])
    flat = torch.from_numpy(np.array(s).reshape(-1)).to(dev)
    rc, host, intact = run_entry(flat, [(0, L)], case["thr"], dev)
    assert intact, (name, "a guard band changed")
    assert_items(host, [s], [wants[name]], [name])
    rc, bare, intact = run_entry(flat, [(0, L)], case["thr"], dev, optional=False)
    assert intact and np.array_equal(bare["kept"], host["kept"]) and np.array_equal(bare["counts"], host["counts"])
    assert (bare["means"] == 0xFF).all() and (bare["order"] == 0xFF).all(), "a NULL output was written somewhere else"
    for _ in range(2):
        rc, again, intact = run_entry(flat, [(0, L)], case["thr"], dev)
        assert intact and all(np.array_equal(again[k], host[k]) for k in host), (name, "two runs, different bytes")


def test_batches_of_mixed_sizes_at_odd_offsets(dev, wants):
    """every case at the default threshold in one call -- LDS and scratch items in one launch, empty ones among them -- at element
    offsets that are no multiples of 64; then more items than one launch holds"""
    sel = cases.default_thr_names()
    flat, items = cases.batch(sel)
    assert any(rows > 1088 for _, rows in items) and any(0 < rows <= 1088 for _, rows in items) and any(off % 64 for off, _ in items)
    rc, host, intact = run_entry(torch.from_numpy(flat).to(dev), items, cases.THR, dev)
    assert intact
    assert_items(host, [cases.get(n)["s"] for n in sel], [wants[n] for n in sel], sel)
    flat, items, mats = cases.many_small()
    rc, host, intact = run_entry(torch.from_numpy(flat).to(dev), items, cases.THR, dev)
    assert intact
    assert_items(host, mats, [C.keep(s, cases.THR) for s in mats], [f"small {k}" for k in range(len(mats))])


def test_refusals_write_nothing(dev):
    """above the row limit, past sims_len, negative sizes, a non-finite threshold, a bad item behind a good one, no handle: refused
    before anything is launched.  The outputs are sized for 65 rows per item whatever the table says, so a call that did launch
    would have somewhere to write."""
    from vsc_hip import _lib
    lib = _lib.load()
    s = cases.get("planted_65")["s"]
    flat = torch.from_numpy(np.array(s).reshape(-1)).to(dev)
    bad_calls = [([(0, 4097)], 0.975), ([(1, 65)], 0.975), ([(flat.numel() + 1, 0)], 0.975), ([(-1, 3)], 0.975), ([(0, -3)], 0.975),
                 ([(0, 65)], float("nan")), ([(0, 65)], float("inf")), ([(0, 65), (0, 4097)], 0.975)]
    h = P()
    _lib.check(lib.vsc_frame_filter_create(None, ctypes.byref(h)))
    for items, thr in bad_calls:
        table = np.asarray(items, np.int64)
        out = {k: guarded(4 * 65 * len(items), dev) for k in ("kept", "counts", "means", "order")}
        ptrs = [P(out[k][1].data_ptr()) for k in ("kept", "counts", "means", "order")]
        rc = lib.vsc_frame_filter_f32(h, P(flat.data_ptr()), flat.numel(), table.ctypes.data, len(items), thr, *ptrs)
        assert rc != 0, (items, thr)
        torch.cuda.synchronize()
        assert all(bool((whole == 0xFF).all()) for whole, _ in out.values()), (items, thr, "a refused call wrote")
    table = np.asarray([[0, 65]], np.int64)
    out = {k: guarded(4 * 65, dev) for k in ("kept", "counts")}
    assert lib.vsc_frame_filter_f32(None, P(flat.data_ptr()), flat.numel(), table.ctypes.data, 1, 0.975, P(out["kept"][1].data_ptr()),
                                    P(out["counts"][1].data_ptr()), None, None) != 0
    assert b"null handle" in lib.vsc_last_error()
    assert lib.vsc_frame_filter_f32(h, P(flat.data_ptr()), flat.numel(), table.ctypes.data, 1, 0.975, None, P(out["counts"][1].data_ptr()),
                                    None, None) != 0                                   # no kept
    torch.cuda.synchronize()
    assert all(bool((whole == 0xFF).all()) for whole, _ in out.values())
    lib.vsc_frame_filter_destroy(h)


def planted_descriptors(rng, n, d, dups):
    """[n, d] float32 rows; `dups` of them are SCALED copies of other rows plus a perturbation of 3 % of the row's norm: cosine
    ~0.9995 to their source, descriptors (and frame means) not equal"""
    x = rng.normal(size=(n, d)).astype(np.float32)
    for dst, src in zip(rng.permutation(n)[:dups], rng.integers(0, n, dups)):
        if dst != src:
            noise = rng.normal(size=d).astype(np.float32)
            x[dst] = x[src] * np.float32(rng.uniform(0.5, 2.0)) + noise * np.float32(0.03 * np.linalg.norm(x[src]) / np.linalg.norm(noise))
    return x


def host_means_of(features):
    """the frame means the host path ranks by, from the same launches"""
    from src.query_postprocess import HipOps
    feat = HipOps.normalize(features)
    return (HipOps.self_similarity(feat) - np.eye(len(feat), dtype=np.float32)).mean(0)


def test_select_frames_hip_equals_host(dev):
    from src.query_postprocess import select_frames
    rng = np.random.default_rng(21)
    for n, dups in ((1, 0), (40, 12), (130, 50), (300, 120)):
        x = planted_descriptors(rng, n, 48, dups)
        assert len(np.unique(host_means_of(x))) == n, "the descriptors tie"
        host, hip = select_frames(x), select_frames(x, frame_filter="hip")
        print(f"select_frames: {n} rows, kept {len(host)}")
        assert hip == host and (dups == 0 or 0 < len(host) < n)
    assert select_frames(np.zeros((0, 48), np.float32), frame_filter="hip") == []


class Fitted:
    mean_ = np.linspace(-0.01, 0.01, 64).astype(np.float32)
    components_ = (np.random.default_rng(5).normal(size=(16, 64)) / 4.0).astype(np.float32)
    whiten = False


def test_process_query_group_hip_equals_host(dev, monkeypatch):
    """accepted, rejected and frameless videos; two views per video (timestamps tiled); one video of 260 rows"""
    from src import query_postprocess as Q
    rng = np.random.default_rng(22)
    frames = [20, 9, 0, 130, 33, 0, 7]                     # per view
    views = [2, 2, 2, 2, 1, 1, 2]
    scores = [1.0, 0.0, 1.0, 0.5, 0.002, 0.0, 0.0005]      # rejected: 1, 5 and 6 (below 0.001); 2 is accepted but frameless
    ids = [f"Q{i:06d}" for i in range(len(frames))]
    rows = [f * v for f, v in zip(frames, views)]
    assert max(rows) >= 257
    full = [planted_descriptors(rng, r, 64, r // 3) if r else np.zeros((0, 64), np.float32) for r in rows]
    subs_by_model = [[torch.from_numpy(np.ascontiguousarray(x[:, lo:hi])).to(dev) for x in full] for lo, hi in ((0, 24), (24, 64))]
    stamps = [np.arange(f) for f in frames]
    pca = Q.HipPCA(Fitted)
    want = Q.process_query_group(ids, subs_by_model, stamps, scores, pca.transform, 3)
    # every accepted video is tie-free, and the filter dropped some but not all rows of at least two of them
    partly = 0
    for v, r in enumerate(rows):
        if scores[v] >= Q.SCORE_THRESHOLD and r:
            feat = np.concatenate([Q.HipOps.normalize(x) for x in (full[v][:, :24], full[v][:, 24:])], axis=1)
            assert len(np.unique(host_means_of(feat))) == r, (ids[v], "frame means tie")
            partly += 0 < len(want[0][v].feature) < r
    assert partly >= 2

    def boom(*a, **k):
        raise AssertionError("greedy_select ran on the hip path")

    monkeypatch.setattr(Q, "greedy_select", boom)
    got = Q.process_query_group(ids, subs_by_model, stamps, scores, pca.transform, 3, frame_filter="hip")
    assert got[2] == want[2]
    for v, (a, b) in enumerate(zip(got[0], want[0])):
        assert a.video_id == b.video_id and a.feature.dtype == b.feature.dtype and a.feature.shape == b.feature.shape, ids[v]
        assert np.array_equal(a.feature.view(np.uint32), b.feature.view(np.uint32)), (ids[v], "final features")
        assert np.array_equal(a.timestamps, b.timestamps) and a.timestamps.dtype == b.timestamps.dtype, (ids[v], "timestamps")
    for pa, pb in zip(got[1], want[1]):
        assert len(pa) == len(pb) == 2
        for a, b in zip(pa, pb):
            assert np.array_equal(a.feature.view(np.uint32), b.feature.view(np.uint32)) and np.array_equal(a.timestamps, b.timestamps)
    assert len(got[0][0].timestamps) < 40 and got[0][1].feature.shape == (1, 512) and got[0][2].feature.shape == (1, 512)


def test_run_query_videos_hip_equals_host(dev):
    """the tiny ViT + tiny Swin of tests/test_query_pipeline.py; per video one near-duplicated frame (a copy with a few pixels moved by
    one 8-bit step): close descriptors, not equal ones"""
    from tools import synth
    from src.query_pipeline import run_query_videos
    from src.query_postprocess import HipOps, HipPCA
    from vsc_hip.config import get_config
    from vsc_hip.encoder import HipEncoder
    from vsc_hip.swin_config import get_swin_config
    from vsc_hip.swin_encoder import SwinHipEncoder
    vcfg, scfg = get_config("tiny"), get_swin_config("tiny_swin")
    vit = HipEncoder(vcfg, synth.encoder_weights(3, vcfg), max_batch=8)
    swin = SwinHipEncoder(scfg, synth.swin_weights(4, scfg), max_batch=8)
    vids, lens = [], [11, 4, 9, 1, 6]
    for i, n in enumerate(lens):
        fr, sf = synth.structured_frames(10 + i, n, vcfg), synth.structured_frames(20 + i, n, scfg)
        for f in (fr, sf):
            if n > 1:
                f[n // 2] = f[0]
                f[n // 2, :, 1, 1:4] += np.float32(2.0 / 255.0)
        vids.append((f"Q{i:06d}", {vcfg.image_size: torch.from_numpy(fr), scfg.image_size: torch.from_numpy(sf)}, np.arange(n)))

    class Fit:
        mean_ = synth.normalish(6, (vcfg.out_dim + scfg.out_dim,)) * 0.01
        components_ = synth.normalish(5, (16, vcfg.out_dim + scfg.out_dim)) / 4.0
        whiten = False

    pca = HipPCA(Fit)
    enc = [(vit, vcfg.image_size), (swin, scfg.image_size)]
    scores = {"Q000001": 0.0, "Q000003": 0.0005}
    for vid, frames, _ in vids:                     # tie-free where it matters: the accepted videos
        if scores.get(vid, 1.0) >= 0.001:
            feat = np.concatenate([HipOps.normalize(vit(frames[vcfg.image_size].to(dev)).cpu().numpy()),
                                   HipOps.normalize(swin(frames[scfg.image_size].to(dev)).cpu().numpy())], axis=1)
            assert len(np.unique(host_means_of(feat))) == len(feat), (vid, "frame means tie")
    for group_frames in (1, 14, 1024):
        want, want_pm = run_query_videos(vids, enc, pca.transform, dict(scores), dev, chunk=8, group_frames=group_frames)
        got, got_pm = run_query_videos(vids, enc, pca.transform, dict(scores), dev, chunk=8, group_frames=group_frames, frame_filter="hip")
        for a, b in zip(got, want):
            assert a.video_id == b.video_id and a.feature.shape == b.feature.shape, (group_frames, a.video_id)
            assert np.array_equal(a.feature.view(np.uint32), b.feature.view(np.uint32)) and np.array_equal(a.timestamps, b.timestamps)
        for pa, pb in zip(got_pm, want_pm):
            assert all(np.array_equal(x.feature, y.feature) for x, y in zip(pa, pb))
    for i in (0, 2, 4):                             # the near-duplicate and its source are never both kept
        kept = got[i].timestamps.tolist()
        print(f"{vids[i][0]}: {lens[i]} frames, kept {kept}")
        assert not (0 in kept and lens[i] // 2 in kept), (vids[i][0], kept)


def test_a_video_above_the_row_limit_is_refused_by_name_before_any_launch(dev, monkeypatch):
    from src import query_postprocess as Q
    from vsc_hip import ops

    def boom(*a, **k):
        raise AssertionError("something was launched")

    for name in ("l2_normalize_", "pair_similarity", "frame_filter"):
        monkeypatch.setattr(ops, name, boom)

    class FakeRows:
        """a device tensor's shape without its 4097 x d floats"""
        shape = (4097, 8)

    with pytest.raises(ValueError, match=r"video Q000001 has 4097 descriptor rows .* at most 4096"):
        Q.process_query_group(["Q000000", "Q000001"], [[torch.zeros((3, 8), device=dev), FakeRows()]], [np.arange(3), np.arange(4097)],
                              [1.0, 1.0], lambda x: x, 0, frame_filter="hip")
    with pytest.raises(ValueError, match=r"video Q000009 has 4097 descriptor rows"):
        Q.select_frames(np.zeros((4097, 2), np.float32), frame_filter="hip", video_id="Q000009")
