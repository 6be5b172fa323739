"""The descriptor-track micro-AP on the device (csrc/uap.hip, vsc_hip/uap.py, average_precision(device="hip"),
`sscd_baseline --uap hip`): both entries through ctypes against the executable contract (tests/uap_contract.py) on uint64 views,
every case of tests/uap_cases.py including the one of 200 000 predictions; average_precision(device="hip") against what the
reference itself returned (tests/golden/uap_device.json) bit for bit; and the placement properties of the two entries -- outputs
between 0xFF guard bands, curve columns beyond n_pos untouched, stream order behind a delay with decoy operands, scratch reused
across sizes, the same bytes run to run, both builds of the library."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import uap_cases as cases  # noqa: E402
import uap_contract as C  # noqa: E402
from vsc.metrics import CandidatePair, Match  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(HERE, "golden", "uap_device.json")))["cases"]
GUARD = 512                     # bytes of 0xFF on both sides of every output
SPIN_TICKS = 120_000_000        # ~50 ms of vsc_debug_spin_ticks (profiles/abi_placement_delay.txt: 2.4e6 ticks per millisecond)
WITH_PREDS = [n for n in cases.names() if cases.get(n)["scores"].size]
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wants():
    """the contract's results of every case with predictions, computed once: (perm, ranked, correct, status, sums, counts, curve)"""
    out = {}
    for name in WITH_PREDS:
        case = cases.get(name)
        pk, gk = cases.keys(case)
        r = C.rank(case["scores"], pk, gk, case["key_bits"])
        out[name] = r + (C.curve(r[1], r[2], len(gk)) if len(gk) else (None, None, None))
    return out


def operands(case, dev):
    pk, gk = cases.keys(case)
    return {"scores": torch.from_numpy(np.array(case["scores"])).to(dev), "pk": torch.from_numpy(pk.view(np.int64)).to(dev),
            "gk": torch.from_numpy(gk.view(np.int64)).to(dev)}


def guarded(nbytes, dev):
    """(whole, body): uint8 tensors, every byte 0xFF (NaN as float64, -1 as int64), GUARD bytes before and after the body"""
    whole = torch.full((nbytes + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + nbytes]


def run_entries(lib, ops, n, g, key_bits, dev, stream=None, sync=True):
    """both entries with guarded outputs -> dict of (whole, body) tensors"""
    from vsc_hip import _lib
    out = {k: guarded(b, dev) for k, b in (("perm", 8 * n), ("ranked", 8 * n), ("correct", n), ("status", 32), ("sums", 16),
                                           ("counts", 16), ("curve", 24 * n))}
    p = {k: P(body.data_ptr()) for k, (_, body) in out.items()}
    h = P()
    _lib.check(lib.vsc_uap_create(stream, ctypes.byref(h)))          # the handle's stream: `stream`, or the null stream
    try:
        _lib.check(lib.vsc_uap_rank_f64(h, P(ops["scores"].data_ptr()), P(ops["pk"].data_ptr()), n, P(ops["gk"].data_ptr()) if g else None, g,
                                        key_bits, p["perm"], p["ranked"], p["correct"], p["status"]))
        if g:
            _lib.check(lib.vsc_uap_curve_f64(h, p["ranked"], p["correct"], n, g, p["sums"], p["counts"], p["curve"]))
    finally:
        lib.vsc_uap_destroy(h)                                       # host state only: what is enqueued does not refer to it
    if sync:
        torch.cuda.synchronize()
    return out


def assert_contract(out, want, n, g, name):
    for whole, body in out.values():
        w = whole.cpu().numpy()
        assert (w[:GUARD] == 0xFF).all() and (w[len(w) - GUARD:] == 0xFF).all(), (name, "a guard band changed")
    host = {k: body.cpu().numpy() for k, (_, body) in out.items()}
    perm, ranked, correct, status, sums, counts, curve = want
    assert np.array_equal(host["status"].view(np.int64), status), (name, host["status"].view(np.int64), status)
    assert np.array_equal(host["perm"].view(np.int64), perm), (name, "perm", np.nonzero(host["perm"].view(np.int64) != perm)[0][:8])
    assert np.array_equal(host["ranked"].view(np.uint64), C.bits(ranked)), (name, "ranked scores")
    assert np.array_equal(host["correct"], correct), (name, "correct")
    if not g:
        return
    n_pos = int(counts[0])
    got_sums, got_curve = host["sums"].view(np.float64), host["curve"].view(np.float64).reshape(3, n)
    print(f"{name}: n {n} g {g} n_pos {n_pos} groups {int(counts[1])} sums {got_sums.tolist()} contract {sums.tolist()}")
    assert np.array_equal(host["counts"].view(np.int64), counts), (name, host["counts"].view(np.int64), counts)
    assert np.array_equal(got_curve[:, :n_pos].view(np.uint64), C.bits(curve)), (name, "a quotient or a score of the curve differs",
                                                                                 np.nonzero((got_curve[:, :n_pos].view(np.uint64) != C.bits(curve)).any(0))[0][:8])
    assert (host["curve"].reshape(3, 8 * n)[:, 8 * n_pos:] == 0xFF).all(), (name, "curve columns beyond n_pos were written")
    assert np.array_equal(got_sums.view(np.uint64), C.bits(sums)), (name, got_sums.tolist(), sums.tolist())


@pytest.mark.parametrize("name", WITH_PREDS)
def test_entries_equal_the_contract_between_guard_bands(dev, wants, name):
    """every case, the refused ones included (their status counts what is wrong and the call completes), sizes around 8, 128,
    256, the tile of 2048, several tiles, 200 000 predictions against 8 000 pairs; 20 and 64 key bits"""
    from vsc_hip import _lib
    case = cases.get(name)
    n, g = len(case["pq"]), len(case["gq"])
    out = run_entries(_lib.load(), operands(case, dev), n, g, case["key_bits"], dev)
    assert_contract(out, wants[name], n, g, name)


@pytest.mark.parametrize("name", list(GOLDEN))
def test_average_precision_hip_equals_the_reference_bit_for_bit(dev, name):
    """`.ap`, `.simple_ap` and the curve the reference's own function returned, or the exception it raised"""
    from vsc.metrics import average_precision
    case, want = cases.get(name), GOLDEN[name]
    gt, preds = cases.pairs(case, CandidatePair)
    if "raises" in want:
        exc = {"KeyError": KeyError, "ValueError": ValueError, "AssertionError": AssertionError}[want["raises"]]
        with pytest.raises(exc) as info:
            average_precision(gt, preds, device="hip")
        if exc is not KeyError:
            assert str(info.value) == want["message"]
        return
    got = average_precision(gt, preds, device="hip")
    rows = [np.ascontiguousarray(v, np.float64) for v in (got.pr_curve.precisions, got.pr_curve.recalls, got.pr_curve.scores)]
    print(f"{name}: ap {got.ap!r} simple_ap {got.simple_ap!r} reference {np.array([want['ap'], want['simple_ap']], np.uint64).view(np.float64).tolist()}")
    assert C.bits([got.ap])[0] == want["ap"] and C.bits([got.simple_ap])[0] == want["simple_ap"]
    assert len(rows[0]) == want["n_pos"] and not any(np.isnan(v).any() for v in rows)
    if "curve" in want:
        assert [C.bits(v).tolist() for v in rows] == want["curve"]
    else:
        assert hashlib.sha256(b"".join(v.tobytes() for v in rows)).hexdigest() == want["curve_sha256"]
    if want["n_pos"] == 0:
        assert got.ap == 0.0 and got.simple_ap == 0.0


def test_hip_stays_within_the_mirrors_pin_of_the_host_path(dev):
    from vsc.metrics import average_precision
    for name in ("n2500_ties", "n1000_distinct", "one_group", "disjoint"):
        gt, preds = cases.pairs(cases.get(name), CandidatePair)
        host, hip = average_precision(gt, preds), average_precision(gt, preds, device="hip")
        assert abs(host.ap - hip.ap) <= 1e-12 and abs(host.simple_ap - hip.simple_ap) <= 1e-12, (name, host.ap, hip.ap)
        assert np.array_equal(host.pr_curve.scores, hip.pr_curve.scores)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_both_builds_of_the_library_run_the_entries(dev, wants, precision):
    from vsc_hip import _lib
    lib = _lib.load(precision)
    for name in ("n2049_ties", "wide_keys_ties"):
        case = cases.get(name)
        n, g = len(case["pq"]), len(case["gq"])
        assert_contract(run_entries(lib, operands(case, dev), n, g, case["key_bits"], dev), wants[name], n, g, f"{precision} {name}")


def test_refusals_and_empty_calls_launch_nothing(dev):
    """argument checks return an error code before any launch; n = 0 returns 0 and leaves every output as it was"""
    from vsc_hip import _lib
    lib = _lib.load()
    case = cases.get("n9_ties")
    ops = operands(case, dev)
    whole, body = guarded(512, dev)
    o = P(body.data_ptr())
    s, pk, gk = (P(ops[k].data_ptr()) for k in ("scores", "pk", "gk"))
    h = P()
    _lib.check(lib.vsc_uap_create(None, ctypes.byref(h)))
    rank, curve = lib.vsc_uap_rank_f64, lib.vsc_uap_curve_f64
    assert rank(h, s, pk, -1, gk, 4, 20, o, o, o, o) != 0 and rank(h, s, pk, 9, gk, -1, 20, o, o, o, o) != 0
    assert rank(h, s, pk, 9, gk, 4, 0, o, o, o, o) != 0 and rank(h, s, pk, 9, gk, 4, 65, o, o, o, o) != 0
    assert rank(h, s, pk, 1 << 31, gk, 4, 20, o, o, o, o) != 0
    assert rank(h, s, pk, 9, gk, 4, 20, None, o, o, o) != 0 and rank(h, s, pk, 9, None, 4, 20, o, o, o, o) != 0
    assert rank(None, s, pk, 9, gk, 4, 20, o, o, o, o) != 0
    assert b"uap_rank" in lib.vsc_last_error()
    assert curve(h, s, o, -1, 4, o, o, o) != 0 and curve(h, s, o, 9, 0, o, o, o) != 0
    assert curve(h, s, o, 9, 4, None, o, o) != 0 and curve(None, s, o, 9, 4, o, o, o) != 0
    assert b"uap_curve" in lib.vsc_last_error()
    assert rank(h, None, None, 0, gk, 4, 20, o, o, o, o) == 0
    assert curve(h, None, None, 0, 4, o, o, o) == 0
    assert lib.vsc_uap_create(None, None) != 0
    lib.vsc_uap_destroy(h)
    torch.cuda.synchronize()
    assert (whole.cpu().numpy() == 0xFF).all(), "a refused or empty call wrote"


def test_entries_on_a_side_stream_run_in_stream_order(dev, wants):
    """The handle is made on a side stream that is busy with a delay.  The operands hold a DECOY (another valid problem of the same
    shapes) when the calls are made; the real operands are copied in on the side stream before the calls and the decoy again after
    them.  Only work that runs on the side stream, in order, sees the real operands -- and the calls return while the delay still
    runs: they only enqueue (the scratch has its size from the plain call before)."""
    from vsc_hip import _lib
    lib = _lib.load()
    name = "n2500_ties"
    case = cases.get(name)
    n, g = len(case["pq"]), len(case["gq"])
    real = operands(case, dev)
    assert_contract(run_entries(lib, real, n, g, case["key_bits"], dev), wants[name], n, g, "plain")
    decoy = {"scores": -real["scores"], "pk": real["pk"].roll(7), "gk": real["gk"].flip(0)}
    ops = {k: v.clone() for k, v in decoy.items()}
    spin_out = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    sp = P(side.cuda_stream)
    started = torch.cuda.Event()
    _lib.check(lib.vsc_debug_spin_ticks(SPIN_TICKS, P(spin_out.data_ptr()), sp))
    started.record(side)
    with torch.cuda.stream(side):
        for k in ops:
            ops[k].copy_(real[k], non_blocking=True)
    out = run_entries(lib, ops, n, g, case["key_bits"], dev, stream=sp, sync=False)
    returned_in_time = not started.query()
    with torch.cuda.stream(side):
        for k in ops:
            ops[k].copy_(decoy[k], non_blocking=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert_contract(out, wants[name], n, g, "side stream")
    assert returned_in_time, "the calls returned only after the delay had ended: they did not just enqueue"
    d = C.rank(decoy["scores"].cpu().numpy(), decoy["pk"].cpu().numpy().view(np.uint64), decoy["gk"].cpu().numpy().view(np.uint64), 64)
    assert not np.array_equal(d[0], wants[name][0]) and not np.array_equal(d[2], wants[name][2])      # the decoy has another answer


def test_scratch_is_reused_across_sizes_back_to_back(dev, wants):
    """released scratch, then a small call, a larger one (every slot grows between two calls) and the small one again -- with no
    synchronisation between the calls of a pair: nothing may depend on what the scratch held or on its size"""
    from vsc_hip import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.vsc_search_release_scratch()
    order = ["n257_ties", "n6149_distinct", "n129_ties", "n2049_ties", "n9_distinct"]
    prepared = [(nm, cases.get(nm), operands(cases.get(nm), dev)) for nm in order]
    outs = [run_entries(lib, ops, len(c["pq"]), len(c["gq"]), c["key_bits"], dev, sync=False) for _, c, ops in prepared]
    torch.cuda.synchronize()
    for (nm, c, _), out in zip(prepared, outs):
        assert_contract(out, wants[nm], len(c["pq"]), len(c["gq"]), nm)


def test_repeat_run_gives_the_same_bytes(dev, wants):
    """200 000 predictions twice: identical bytes in every output (and the contract's)"""
    from vsc_hip import _lib
    case = cases.get(cases.BIG)
    n, g = len(case["pq"]), len(case["gq"])
    ops = operands(case, dev)
    first = run_entries(_lib.load(), ops, n, g, case["key_bits"], dev)
    second = run_entries(_lib.load(), ops, n, g, case["key_bits"], dev)
    for k in first:
        assert torch.equal(first[k][0], second[k][0]), k
    assert_contract(second, wants[cases.BIG], n, g, "repeat")


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


def test_entry_point_prints_the_same_candidate_uap(dev, tmp_path, capsys):
    """sscd_baseline.main with uap = "hip" prints what it prints with "host", to the printed digits, and writes the same files;
    on the candidates it wrote, `.ap` of the two paths differs by at most the mirror's pin of 1e-12"""
    import vsc.baseline.sscd_baseline as entry
    from vsc.metrics import average_precision
    from vsc.storage import store_features
    queries, refs, planted = _planted_videos()
    store_features(tmp_path / "q.npz", queries)
    store_features(tmp_path / "r.npz", refs)
    Match.write_csv(planted, tmp_path / "gt.csv")
    base = ["--query_features", str(tmp_path / "q.npz"), "--ref_features", str(tmp_path / "r.npz"), "--overwrite", "--alignment", "hip",
            "--ground_truth", str(tmp_path / "gt.csv"), "--segment_metric", "hip"]
    capsys.readouterr()
    entry.main(entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "host")]))
    host = capsys.readouterr().out
    entry.main(entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "hip"), "--uap", "hip"]))
    hip = capsys.readouterr().out
    assert "Candidate uAP: " in host and "Matching track pairwise uAP: " in host and hip == host
    assert (tmp_path / "host" / "candidates.csv").read_bytes() == (tmp_path / "hip" / "candidates.csv").read_bytes()
    gt = entry.read_ground_truth_pairs(str(tmp_path / "gt.csv"))
    cands = CandidatePair.read_csv(tmp_path / "hip" / "candidates.csv")
    a, b = average_precision(gt, cands), average_precision(gt, cands, device="hip")
    assert a.ap > 0.0 and abs(a.ap - b.ap) <= 1e-12 and f"Candidate uAP: {b.ap:.4f}\n" in hip
    ns = entry.build_parser().parse_args(base + ["--output_path", str(tmp_path / "old")])
    del ns.uap                                                   # a namespace from before the option: as "host"
    entry.main(ns)
    assert capsys.readouterr().out == host
    ns.uap = "device"
    with pytest.raises(ValueError, match="host"):
        entry.main(ns)
