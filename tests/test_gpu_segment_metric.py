"""The matching-track segment AP on the device (vsc_segment_metric_*, vsc_hip/segment_metric.py, vsc.metrics.match_metric /
evaluate_matching_track, `sscd_baseline --segment_metric hip`): both entries against the executable contract
(tests/segment_metric_contract.py) on uint64 views, the metric against the reference's recorded results
(tests/golden/segment_metric.json) bit for bit, and the placement properties of the two entries -- guard bands, stream order behind
a delay with decoy operands, scratch reused across handles -- which this file proves itself because the handle fixes the stream at
creation (tests/abi_cases.py covers the entries that take a stream per call)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import segment_metric_cases as cases
import segment_metric_contract as C
from vsc.metrics import Match

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = {r["name"]: r for r in json.load(open(os.path.join(HERE, "golden", "segment_metric.json")))}
CASES = {name: (gts, preds) for name, gts, preds in cases.cases()}
WITH_PREDS = [name for name, (gts, preds) in CASES.items() if preds]
GUARD = 64                      # doubles of NaN on both sides of every output
SPIN_TICKS = 120_000_000        # ~50 ms of vsc_debug_spin_ticks (profiles/abi_placement_delay.txt: 2.4e6 ticks per millisecond)
NAMES = ("pred_boxes", "pred_ptr", "pred_rank", "gt_boxes", "gt_ptr", "group_ends")


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def packed():
    """every case with predictions, packed by the contract, with the contract's results: computed once"""
    out = {}
    for name in WITH_PREDS:
        k = C.pack(*CASES[name])
        d, gt_len = C.deltas(k["pred_boxes"], k["pred_ptr"], k["pred_rank"], k["gt_boxes"], k["gt_ptr"], k["n_pairs"])
        out[name] = (k, d, gt_len, C.scan(d, k["group_ends"]))
    return out


def as_matches(gts, preds):
    return ([Match(q, r, 1.0, *box) for q, r, *box in gts], [Match(q, r, s, *box) for q, r, s, *box in preds])


def guarded(shape, dev):
    """(whole, body): a float64 tensor of NaN with GUARD elements before and after the body"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=dev)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def guards_intact(whole):
    w = whole.cpu().numpy()
    return bool(np.isnan(w[:GUARD]).all() and np.isnan(w[-GUARD:]).all())


def run_guarded(h, k, dev, ops=None):
    """both entries of handle `h` on packed case `k` with guarded outputs -> (deltas, gt_len, groups) as numpy; asserts the guards"""
    ops = ops or {n: torch.from_numpy(k[n]).to(dev) for n in NAMES}
    wd, d = guarded((len(k["pred_boxes"]), 4), dev)
    wl, gt_len = guarded((k["n_pairs"], 2), dev)
    wg, groups = guarded((len(k["group_ends"]), 4), dev)
    h.deltas(ops["pred_boxes"], ops["pred_ptr"], ops["pred_rank"], ops["gt_boxes"], ops["gt_ptr"], deltas=d, gt_len=gt_len)
    h.scan(d, ops["group_ends"], out=groups)
    torch.cuda.synchronize()
    assert guards_intact(wd) and guards_intact(wl) and guards_intact(wg), "a guard band changed"
    return d.cpu().numpy(), gt_len.cpu().numpy(), groups.cpu().numpy()


def assert_contract(got, want, name):
    for g, w, what in zip(got, want, ("deltas", "gt_len", "groups")):
        assert g.shape == w.shape and not np.isnan(g).any(), (name, what, "an element was left unwritten")
        assert np.array_equal(C.bits(g), C.bits(w)), (name, what, np.nonzero((C.bits(g) != C.bits(w)).reshape(len(g), -1).any(1))[0][:8])


@pytest.mark.parametrize("name", WITH_PREDS)
def test_entries_equal_the_contract_between_guard_bands(dev, packed, name):
    from vsc_hip.segment_metric import HipSegmentMetric
    k, d, gt_len, groups = packed[name]
    with HipSegmentMetric() as h:
        assert_contract(run_guarded(h, k, dev), (d, gt_len, groups), name)
        if k["n_gt_pairs"]:                                     # the ground-truth totals: a scan of two columns with one end
            wt, totals = guarded((1, 2), dev)
            h.scan(torch.from_numpy(gt_len[:k["n_gt_pairs"]].copy()).to(dev), torch.tensor([k["n_gt_pairs"] - 1], device=dev), out=totals)
            torch.cuda.synchronize()
            assert guards_intact(wt)
            assert np.array_equal(C.bits(totals.cpu().numpy()), C.bits(C.scan(gt_len[:k["n_gt_pairs"]], [k["n_gt_pairs"] - 1])))


@pytest.mark.parametrize("n,cols", [(1, 1), (511, 3), (512, 8), (513, 4), (70001, 4)])
def test_scan_tiles_columns_and_ends(dev, n, cols):
    """rows around the tile of 512 and over many tiles; ends: every row, a sparse set, repeated ends, the last row alone"""
    from vsc_hip.segment_metric import HipSegmentMetric
    rs = np.random.RandomState(n)
    rows = rs.uniform(-1, 1, (n, cols)) * 10.0 ** rs.randint(-8, 8, (n, cols))
    want = np.cumsum(rows, axis=0)                               # 1-D accumulation per column: strictly left to right
    assert n > 2000 or np.array_equal(C.bits(want), C.bits(C.scan(rows, np.arange(n))))
    with HipSegmentMetric() as h:
        for ends in (np.arange(n), np.unique(rs.randint(0, n, max(n // 7, 1))), np.sort(rs.randint(0, n, 10)).repeat(2), np.array([n - 1])):
            wo, out = guarded((len(ends), cols), dev)
            h.scan(torch.from_numpy(rows).to(dev), torch.from_numpy(ends.astype(np.int64)).to(dev), out=out)
            torch.cuda.synchronize()
            assert guards_intact(wo) and np.array_equal(C.bits(out.cpu().numpy()), C.bits(want[ends])), (n, cols, len(ends))


def test_refusals_and_empty_calls(dev):
    from vsc_hip import _lib
    from vsc_hip.segment_metric import HipSegmentMetric
    lib = _lib.load()
    x = torch.zeros((4, 9), dtype=torch.float64, device=dev)
    e = torch.tensor([3], device=dev)
    with HipSegmentMetric() as h:
        for cols in (0, 9, -1):
            assert lib.vsc_segment_metric_scan_f64(h._h, _lib.ptr(x), 4, cols, _lib.ptr(e), 1, _lib.ptr(x)) == -1
        assert lib.vsc_segment_metric_scan_f64(h._h, _lib.ptr(x), -1, 2, _lib.ptr(e), 1, _lib.ptr(x)) == -1
        assert lib.vsc_segment_metric_scan_f64(h._h, None, 0, 2, None, 0, None) == 0
        assert lib.vsc_segment_metric_scan_f64(h._h, None, 4, 2, None, 1, None) == -1
        assert lib.vsc_segment_metric_deltas_f64(h._h, None, None, None, -1, None, None, 0, 1, None, None) == -1
        assert lib.vsc_segment_metric_deltas_f64(h._h, None, None, None, 1 << 31, None, None, 0, 1, None, None) == -1
        assert lib.vsc_segment_metric_deltas_f64(h._h, None, None, None, 0, None, None, 5, 3, None, None) == 0
        assert lib.vsc_segment_metric_deltas_f64(h._h, None, None, None, 2, None, None, 0, 1, None, None) == -1
        assert lib.vsc_segment_metric_deltas_f64(None, None, None, None, 0, None, None, 0, 1, None, None) == -1
    torch.cuda.synchronize()


def test_handle_on_a_side_stream_runs_in_stream_order(dev, packed):
    """The handle is made on a side stream that is busy with a delay.  The operands hold a DECOY (another valid problem of the same
    shapes) when the calls are made; the real operands are copied in on the side stream before the calls and the decoy again
    after them.  Only work that runs on the side stream, in order, sees the real operands -- and the calls return while the delay
    still runs: they only enqueue."""
    from vsc_hip import _lib
    from vsc_hip.segment_metric import HipSegmentMetric
    lib = _lib.load()
    k, d, gt_len, groups = packed["sizes_grid_quarter"]
    real = {n: torch.from_numpy(k[n]).to(dev) for n in NAMES}
    decoy = {n: (v * 0.5 + 1.0 if v.dtype == torch.float64 else v.clone()) for n, v in real.items()}
    ops = {n: v.clone() for n, v in decoy.items()}
    wd, out_d = guarded(d.shape, dev)
    wl, out_l = guarded(gt_len.shape, dev)
    wg, out_g = guarded(groups.shape, dev)
    spin_out = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    started = torch.cuda.Event()
    with torch.cuda.stream(side):
        h = HipSegmentMetric()                                   # bound to `side`
        _lib.check(lib.vsc_debug_spin_ticks(SPIN_TICKS, ctypes.c_void_p(spin_out.data_ptr()), ctypes.c_void_p(side.cuda_stream)))
        started.record(side)
        for n in NAMES:
            ops[n].copy_(real[n], non_blocking=True)
    # the calls themselves are made with ANOTHER stream current: the handle's stream is the one it was made on
    h.deltas(ops["pred_boxes"], ops["pred_ptr"], ops["pred_rank"], ops["gt_boxes"], ops["gt_ptr"], deltas=out_d, gt_len=out_l)
    h.scan(out_d, ops["group_ends"], out=out_g)
    returned_in_time = not started.query()
    with torch.cuda.stream(side):
        for n in NAMES:
            ops[n].copy_(decoy[n], non_blocking=True)
    side.synchronize()
    torch.cuda.synchronize()
    h.close()
    assert guards_intact(wd) and guards_intact(wl) and guards_intact(wg)
    assert_contract((out_d.cpu().numpy(), out_l.cpu().numpy(), out_g.cpu().numpy()), (d, gt_len, groups), "side stream")
    assert returned_in_time, "the calls returned only after the delay had ended: they did not just enqueue"
    # and the decoy is a problem with another answer: a call that had read it would have failed above
    dk = dict(k, pred_boxes=decoy["pred_boxes"].cpu().numpy(), gt_boxes=decoy["gt_boxes"].cpu().numpy())
    assert not np.array_equal(C.deltas(dk["pred_boxes"], k["pred_ptr"], k["pred_rank"], dk["gt_boxes"], k["gt_ptr"], k["n_pairs"])[0], d)


def test_two_handles_in_a_row_reuse_freed_scratch(dev, packed):
    """a handle that grew its scratch on the largest case is destroyed; the next one allocates (what the allocator just got
    back) and runs other cases, then grows: nothing may depend on what the scratch held"""
    from vsc_hip.segment_metric import HipSegmentMetric
    big, small, other = packed["sizes_continuous"], packed["planted"], packed["many_pairs_grid_half"]
    with HipSegmentMetric() as h:
        assert_contract(run_guarded(h, big[0], dev), big[1:], "first handle")
    with HipSegmentMetric() as h:
        assert_contract(run_guarded(h, small[0], dev), small[1:], "second handle, small")
        assert_contract(run_guarded(h, other[0], dev), other[1:], "second handle, grown")
        assert_contract(run_guarded(h, big[0], dev), big[1:], "second handle, grown again")
        assert_contract(run_guarded(h, small[0], dev), small[1:], "second handle, small in the large scratch")


@pytest.mark.parametrize("name", list(CASES))
def test_match_metric_equals_the_reference_bit_for_bit(dev, tmp_path, name):
    """match_metric on the lists and evaluate_matching_track through a csv round trip: the reference's `.ap` and curve, or its
    ZeroDivisionError"""
    from vsc.metrics import evaluate_matching_track, match_metric
    G, P = as_matches(*CASES[name])
    Match.write_csv(G, tmp_path / "gt.csv")
    Match.write_csv(P, tmp_path / "pred.csv")
    g = GOLDEN[name]
    if g.get("raises"):
        with pytest.raises(ZeroDivisionError):
            match_metric(G, P)
        with pytest.raises(ZeroDivisionError):
            evaluate_matching_track(str(tmp_path / "gt.csv"), str(tmp_path / "pred.csv"))
        return
    both = evaluate_matching_track(str(tmp_path / "gt.csv"), str(tmp_path / "pred.csv"))
    for ap in (match_metric(G, P), both.segment_ap):
        assert float(ap.ap).hex() == g["ap"], (name, ap.ap, float.fromhex(g["ap"]))
        for field in ("precisions", "recalls", "scores"):
            assert [float(v).hex() for v in getattr(ap.pr_curve, field)] == g[field], (name, field)
    if P:
        assert 0.0 <= both.pairwise_micro_ap.ap <= 1.0


def test_repeat_run_gives_the_same_bytes_and_the_contract(dev):
    """20 000 predictions over 200 pairs, three ground truths each: twice on one handle, once on another"""
    from vsc_hip.segment_metric import HipSegmentMetric
    k = C.pack(*cases.workload(11, 200, 100, 3))
    d, gt_len = C.deltas(k["pred_boxes"], k["pred_ptr"], k["pred_rank"], k["gt_boxes"], k["gt_ptr"], k["n_pairs"])
    want = (d, gt_len, np.cumsum(d, axis=0)[k["group_ends"]])
    with HipSegmentMetric() as h:
        first, second = run_guarded(h, k, dev), run_guarded(h, k, dev)
    with HipSegmentMetric() as h:
        third = run_guarded(h, k, dev)
    for a, b, c in zip(first, second, third):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert_contract(first, want, "repeat")


def _planted_videos(seed=5, dim=64):
    """queries that copy a segment of a reference each (small noise), plus unrelated videos; the planted segments as ground truth"""
    from tools import synth
    from vsc.index import VideoFeature
    rs = np.random.RandomState(seed)
    refs = [VideoFeature(f"R{i:06d}", np.arange(60.0), synth.descriptor_bank(300 + i, 60, dim)) for i in range(12)]
    queries, planted = [], []
    for i in range(8):
        f = synth.descriptor_bank(600 + i, 40, dim)
        if i < 5:
            r, q0, r0, ln = 2 + i, 3 + i, 10 + 2 * i, 20 + i
            f[q0:q0 + ln] = refs[r].feature[r0:r0 + ln] + 0.02 * rs.randn(ln, dim).astype(np.float32)
            f[q0:q0 + ln] /= np.linalg.norm(f[q0:q0 + ln], axis=1, keepdims=True)
            planted.append(Match(f"Q{i:06d}", refs[r].video_id, 1.0, float(q0), float(q0 + ln), float(r0), float(r0 + ln)))
        queries.append(VideoFeature(f"Q{i:06d}", np.arange(40.0), f))
    return queries, refs, planted


def test_entry_point_prints_the_metric_only_when_asked(dev, tmp_path, capsys):
    """sscd_baseline.main with segment_metric = "hip" prints `Matching track metric` for the matches.csv it wrote -- the value of
    the naive contract on that file -- and without the option its output is what it was"""
    import vsc.baseline.sscd_baseline as entry
    from vsc.storage import store_features
    queries, refs, planted = _planted_videos()
    store_features(tmp_path / "q.npz", queries)
    store_features(tmp_path / "r.npz", refs)
    Match.write_csv(planted, tmp_path / "gt.csv")
    base = ["--query_features", str(tmp_path / "q.npz"), "--ref_features", str(tmp_path / "r.npz"), "--overwrite", "--alignment", "hip",
            "--ground_truth", str(tmp_path / "gt.csv")]
    capsys.readouterr()
    entry.main(entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "plain")]))
    plain = capsys.readouterr().out
    entry.main(entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "scored"), "--segment_metric", "hip"]))
    scored = capsys.readouterr().out
    assert (tmp_path / "plain" / "matches.csv").read_bytes() == (tmp_path / "scored" / "matches.csv").read_bytes()
    assert "Matching track" not in plain and "Candidate uAP: " in plain
    rows = Match.read_csv(tmp_path / "scored" / "matches.csv")
    assert rows
    want = C.match_metric([tuple(m)[:2] + tuple(m)[3:] for m in planted], [tuple(m) for m in rows])[0]
    assert want > 0.0, want                                      # some planted segment is found (0.884 when this was written)
    lines = scored.splitlines(keepends=True)
    assert "".join(lines[:-2]) == plain and lines[-2] == f"Matching track metric: {want:.4f}\n"
    assert lines[-1].startswith("Matching track pairwise uAP: ")
    ns = entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "old")])
    del ns.segment_metric                                        # a namespace from before the option: as "none"
    entry.main(ns)
    assert capsys.readouterr().out == plain
