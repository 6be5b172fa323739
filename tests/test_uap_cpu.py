"""The descriptor-track micro-AP without a GPU: the executable contract of the two device entries (tests/uap_contract.py) plus
what the caller does with their sums equals what the REFERENCE's own average_precision returned on every case of
tests/uap_cases.py (tests/golden/uap_device.json: `.ap`, `.simple_ap`, the curve or its hash, bit for bit) -- this is where "equal
to the reference" is established; the emulated kernels and the device are held against the contract.  Also: the contract's
summation tree is np.sum's, its ranking is sorted(reverse=True)'s, the refusals raise the recorded types, and the host logic of the
new options."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import uap_cases as cases  # noqa: E402
import uap_contract as C  # noqa: E402
from vsc.metrics import CandidatePair  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "uap_device.json")))["cases"]
SCORED = [n for n in cases.names() if "raises" not in GOLDEN[n]]


def contract_run(case):
    pk, gk = cases.keys(case)
    perm, ranked, correct, status = C.rank(case["scores"], pk, gk, case["key_bits"])
    sums, counts, curve = C.curve(ranked, correct, len(gk))
    return perm, ranked, correct, status, sums, counts, curve


def test_golden_covers_every_case_and_stays_small():
    assert set(GOLDEN) == set(cases.names())
    assert os.path.getsize(os.path.join(HERE, "golden", "uap_device.json")) < 128 * 1024
    sizes = {len(c["scores"]) for c in cases.cases()}
    assert set(cases.SIZES) <= sizes and 200000 in sizes and {cases.TILE - 1, cases.TILE, cases.TILE + 1, 3 * cases.TILE + 5} <= sizes
    assert {c["key_bits"] for c in cases.cases()} == {20, 64}
    assert max(int(c["pq"].max()) for c in cases.cases() if c["key_bits"] == 64) == 2 ** 32 - 1


@pytest.mark.parametrize("name", SCORED)
def test_contract_and_finish_equal_the_reference_bit_for_bit(name):
    case, want = cases.get(name), GOLDEN[name]
    perm, ranked, correct, status, sums, counts, curve = contract_run(case)
    ap, simple = C.finish(sums, counts, len(case["gq"]))
    assert status[:3].tolist() == [0, 0, 0] and int(counts[0]) == want["n_pos"] == int(status[3])
    assert C.bits([ap])[0] == want["ap"] and C.bits([simple])[0] == want["simple_ap"], (ap, simple)
    if "curve" in want:
        assert C.bits(curve).tolist() == want["curve"]
    else:
        assert hashlib.sha256(b"".join(np.ascontiguousarray(r).tobytes() for r in curve)).hexdigest() == want["curve_sha256"]
    if want["n_pos"] == 0:
        assert ap == 0.0 and simple == 0.0 and not np.isnan(sums).any()


@pytest.mark.parametrize("name", SCORED)
def test_contract_ranking_is_the_stable_descending_sort(name):
    """the order of the 64-bit score image = argsort(-s, kind="stable") = sorted(reverse=True) on Python floats, ties in input
    order, -0.0 beside +0.0 included"""
    s = cases.get(name)["scores"]
    perm = C.rank(s, np.arange(len(s), dtype=np.uint64), np.zeros(0, np.uint64))[0]
    assert np.array_equal(perm, np.argsort(-s, kind="stable"))
    if len(s) <= 6149:
        assert perm.tolist() == sorted(range(len(s)), key=s.tolist().__getitem__, reverse=True)


def test_score_image_orders_zeros_denormals_and_neighbours():
    x = np.float32(0.41)
    s = np.array([0.0, -0.0, 1e-45, -1e-45, x, np.nextafter(x, np.float32(1)), -3.5, 2.0, -np.inf, np.inf], np.float32).astype(np.float64)
    k = C.score_keys(s)
    assert k[0] == k[1] and len(np.unique(k)) == len(s) - 1
    for i in range(len(s)):
        for j in range(len(s)):
            assert (k[i] < k[j]) == (s[i] > s[j]), (s[i], s[j])


@pytest.mark.parametrize("name", SCORED)
def test_pairwise_is_numpys_sum_on_every_case(name):
    """both term vectors of the case, as the reference's libraries build them: contiguous float64"""
    case = cases.get(name)
    perm, ranked, correct, status, sums, counts, curve = contract_run(case)
    if not len(ranked):
        return
    c = correct.astype(bool)
    cum = np.cumsum(c)
    precision = cum / (np.arange(len(c)) + 1)
    assert C.bits([np.sum(precision * c)])[0] == C.bits(sums)[1]
    last = np.nonzero(np.r_[ranked[1:] != ranked[:-1], True])[0]
    tps = cum[last]
    if counts[0]:
        recall = tps / tps[-1]
        terms = (np.diff(np.r_[0.0, recall]) * (tps / (last + 1)))[::-1].copy()
        assert C.bits([np.sum(terms)])[0] == C.bits(sums)[0]
        assert C.bits([-np.sum(-terms)])[0] == C.bits(sums)[0]          # what sklearn sums is the negated vector


def test_pairwise_is_numpys_sum_at_every_threshold_of_the_tree():
    rs = np.random.RandomState(3)
    lengths = list(range(0, 300)) + [1000, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 8200, 16383, 16384, 16385, 16520, 24577, 70001]
    for n in lengths:
        a = rs.standard_normal(n) * 10.0 ** rs.randint(-6, 6, n)
        assert C.bits([C.pairwise(a)])[0] == C.bits([np.sum(a)])[0], n
    assert C.bits([C.pairwise([-0.0, -0.0])])[0] == C.bits([np.sum(np.array([-0.0, -0.0]))])[0]


def test_summing_the_groups_forward_is_not_the_reference():
    """the finding behind the device path's order: on some cases the forward sum of the same terms differs in the last bits"""
    differs = 0
    for name in SCORED:
        case = cases.get(name)
        perm, ranked, correct, status, sums, counts, curve = contract_run(case)
        if not counts[0]:
            continue
        cum = np.cumsum(correct.astype(bool))
        last = np.nonzero(np.r_[ranked[1:] != ranked[:-1], True])[0]
        tps = cum[last]
        forward = np.sum(np.diff(np.r_[0.0, tps / tps[-1]]) * (tps / (last + 1)))
        differs += C.bits([forward])[0] != C.bits(sums)[0]
        assert abs(forward - sums[0]) <= 1e-12
    assert differs > 0


@pytest.mark.parametrize("name", [n for n in cases.names() if "raises" in GOLDEN[n]])
def test_refusals_raise_what_the_reference_raised(name):
    """the status the rank entry counts, through the wrapper's check: the recorded exception type, and for the reference's own
    refusals its message"""
    from vsc_hip.uap import check_status
    case, want = cases.get(name), GOLDEN[name]
    pk, gk = cases.keys(case)
    status = C.rank(case["scores"], pk, gk, case["key_bits"])[3]
    exc = {"KeyError": KeyError, "ValueError": ValueError, "AssertionError": AssertionError}[want["raises"]]
    with pytest.raises(exc) as info:
        check_status(status, len(pk), len(gk))
    if exc is not KeyError:
        assert str(info.value) == want["message"]


def test_check_status_keeps_the_references_order_of_refusals():
    from vsc_hip.uap import check_status
    check_status([0, 0, 0, 5], 9, 3)
    with pytest.raises(AssertionError, match="ground truth"):
        check_status([1, 1, 1, 0], 9, 3)
    with pytest.raises(AssertionError, match="predictions"):
        check_status([1, 1, 0, 0], 9, 3)
    with pytest.raises(KeyError):
        check_status([1, 0, 0, 0], 9, 0)
    with pytest.raises(ValueError, match="finite"):
        check_status([1, 0, 0, 0], 9, 3)


def test_interned_keys_are_equal_exactly_where_the_pairs_are():
    from vsc_hip.uap import intern_pairs
    case = cases.get("n1000_ties")
    gt, preds = cases.pairs(case, CandidatePair)
    pk, gk, key_bits = intern_pairs(gt, preds)
    assert pk.dtype == gk.dtype == np.uint64 and 2 <= key_bits <= 64 and int(max(pk.max(), gk.max())) < 1 << key_bits
    assert len(np.unique(pk)) == len(preds) and len(np.unique(gk)) == len(gt)
    mine, theirs = cases.keys(case)
    assert np.array_equal(np.isin(pk, gk), np.isin(mine, theirs))
    pk, gk, key_bits = intern_pairs([], [CandidatePair("Q1", "R1", 0.5)])
    assert len(gk) == 0 and pk.tolist() == [0] and key_bits == 2


def test_device_option_of_the_metrics_and_entry_points():
    """device="host" is the default and returns exactly what the function returned before the option; unknown values are refused
    naming the choices; the entry points parse --uap and eval.sh passes UAP on"""
    import vsc.baseline.sscd_baseline as entry
    from vsc.metrics import average_precision, evaluate_matching_track, micro_average_precision
    gt, preds = cases.pairs(cases.get("n257_ties"), CandidatePair)
    a, b = average_precision(gt, preds), average_precision(gt, preds, device="host")
    assert C.bits([a.ap, a.simple_ap]).tolist() == C.bits([b.ap, b.simple_ap]).tolist()
    assert all(np.array_equal(C.bits(getattr(a.pr_curve, f)), C.bits(getattr(b.pr_curve, f))) for f in ("precisions", "recalls", "scores"))
    want = GOLDEN["n257_ties"]
    ref = np.array([want["ap"], want["simple_ap"]], np.uint64).view(np.float64)
    assert abs(a.ap - ref[0]) <= 1e-12 and abs(a.simple_ap - ref[1]) <= 1e-12          # the mirror's pin
    assert micro_average_precision(gt, preds) == micro_average_precision(gt, preds, device="host") == a.simple_ap
    for call in (lambda: average_precision(gt, preds, device="cuda"), lambda: micro_average_precision(gt, preds, device="cuda"),
                 lambda: evaluate_matching_track("no.csv", "no.csv", uap="cuda")):
        with pytest.raises(ValueError, match=r"host.*hip"):
            call()
    p = entry.build_parser()
    base = ["--query_features", "q", "--ref_features", "r", "--output_path", "o"]
    assert p.parse_args(base).uap == "host" and p.parse_args(base + ["--uap", "hip"]).uap == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--uap", "cuda"])
    assert entry.UAPS == ("host", "hip")
    sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd"))
    import infer_matching
    args = ["--query_features", "q", "--norm_refs", "n", "--refs", "r", "--sn_refs", "s", "--cls_models", "c", "--refine_models", "m",
            "--output", "o"]
    assert infer_matching.build_parser().parse_args(args).uap == "host"
    assert infer_matching.build_parser().parse_args(args + ["--uap", "hip"]).uap == "hip"
    assert '--uap "${UAP:-host}"' in open(os.path.join(ROOT, "vsc22-submission_amd", "eval.sh")).read()
